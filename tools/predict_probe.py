"""Times of the tiled predictive variances (InterpolatedLLGP(variance_batch=...),
runlmc_amd/approx/quadforms.py), one JSON line per measurement on stdout:

    python tools/predict_probe.py [--parts e2e,tile,precompute] [--record profiles/predict]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/predict_probe.py --parts kernels

Problems: runlmc_amd/util/synth.py, rbf family (the direct solve applies): C2 (n = 20 000), ten
outputs of 30 000 points (n = 3 10^5) and C5 (n = 10^6).
  e2e         seconds of predict() with prediction='on-the-fly' on 1 024 seeded test points for
              variance_batch in {32, 128, 512}, and of the host path (variance_batch=None, same
              model, same points) where its (n_test, n) host arrays fit (C2 and 3 10^5); median
              of --repeats calls after one warm-up call, each ended by a device synchronisation.
  tile        one tile of 128 rows at C5 taken apart: assembly (rl_exact_cross_dev), solve,
              reduction (rl_row_dots), seconds each (median) and their shares.
  precompute  the whole nu at C2 (Dm = 20 016) with variance_batch = 128; at C5 (Dm = 1 000 040) the
              seconds of a tile of 128 grid columns and the total extrapolated from it.
  kernels     one launch sequence for a kernel trace, no timing here: the 128 x 10^6, Q = 5 rows
              through k_ex_cross_rows (rl_exact_cross_dev) and through k_ex_assemble
              (rl_exact_cross_host, which takes the rows in chunks of 33), then one tile of the
              engine.  Run under rocprofv3 --kernel-trace --stats in a run of its own.
--record DIR appends every line to DIR/predict_probe.jsonl and sends stderr to
DIR/predict_probe.stderr; the script fails when it has written no line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {'c2': (4, 3, 1, 5000), 'n3e5': (10, 5, 1, 30000), 'c5': (10, 5, 1, 100000)}
_LINES = 0
_RECORD = None


def emit(rec):
    global _LINES
    line = json.dumps(rec)
    print(line, flush=True)
    if _RECORD is not None:
        _RECORD.write(line + '\n')
        _RECORD.flush()
    _LINES += 1


def sync():
    import torch
    torch.cuda.synchronize()


def median_time(f, repeats):
    f()                                   # warm-up: code objects, allocator, workspaces
    sync()
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        f()
        sync()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), ts


def model_for(name, prediction='on-the-fly'):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    from runlmc_amd.util import synth
    p = synth.make_problem(*SIZES[name])
    np.random.seed(5)
    model = InterpolatedLLGP(p.Xs, p.Ys, normalize=False, functional_kernel=synth.functional_kernel(p),
                             prediction=prediction, variance_batch=128)
    model.parameters_changed()
    M = model._K.preconditioner
    solver = 'direct' if M is not None and M.exact else ('pcg' if M is not None else 'minres')
    return p, model, solver


def test_points(p, total, seed=81):
    rng = np.random.RandomState(seed)
    counts = np.bincount(rng.randint(0, p.D, total), minlength=p.D)
    return [rng.rand(int(c), 1) * 0.98 + 0.01 for c in counts]


def part_e2e(repeats):
    for name in ('c2', 'n3e5', 'c5'):
        p, model, solver = model_for(name)
        Xt = test_points(p, 1024)
        base = dict(part='e2e', problem=name, n=p.n, n_test=1024, solver=solver, repeats=repeats)
        for vb in (32, 128, 512):
            model.variance_batch = vb
            med, ts = median_time(lambda: model.predict(Xt), repeats)
            st = model.variance_stats
            emit(dict(base, variance_batch=vb, predict_s=med, all_s=ts,
                      max_residual=float(st.residuals.max()), max_iterations=int(st.iterations.max())))
        if name != 'c5':                  # (1 024 x 10^6 doubles: 8 GB per host array, several of them)
            model.variance_batch = None
            med, ts = median_time(lambda: model.predict(Xt), repeats)
            emit(dict(base, variance_batch=None, predict_s=med, all_s=ts))
        del model


def part_tile(repeats):
    from runlmc_amd.approx.iterative import Iterative
    from runlmc_amd.approx.quadforms import CrossRows
    from runlmc_amd._native import row_dots
    p, model, solver = model_for('c5')
    Xt = test_points(p, 128)
    rows = CrossRows(model._light_exact(), np.vstack(Xt), [len(x) for x in Xt])
    lib = rows.op.lib
    B = rows.fill(0, 128)
    X = Iterative.solve_device(model._K, B, tol=1e-4)[0]
    t_a, _ = median_time(lambda: rows.fill(0, 128), repeats)
    t_s, _ = median_time(lambda: Iterative.solve_device(model._K, B, tol=1e-4), repeats)
    t_r, _ = median_time(lambda: row_dots(lib, B, X), repeats)
    total = t_a + t_s + t_r
    emit(dict(part='tile', problem='c5', n=p.n, rows=128, Q=p.Q, solver=solver, assembly_s=t_a,
              solve_s=t_s, reduction_s=t_r, assembly_share=t_a / total, solve_share=t_s / total,
              reduction_share=t_r / total,
              assembly_gb_per_s=128 * p.n * 8 / t_a / 1e9,
              reduction_gb_per_s=2 * 128 * p.n * 8 / t_r / 1e9))


def part_precompute(repeats):
    from runlmc_amd.approx import quadforms as qf
    p, model, solver = model_for('c2', 'precompute')
    t = time.perf_counter()
    nu = model._precomputed_nu()
    sync()
    st = model.variance_stats
    emit(dict(part='precompute', problem='c2', n=p.n, Dm=len(nu), variance_batch=128, solver=solver,
              tiles=-(-len(nu) // 128), total_s=time.perf_counter() - t,
              max_residual=float(st.residuals.max())))
    del model
    p, model, solver = model_for('c5', 'precompute')
    (gk,) = model._grid_kernels.values()
    idx = np.random.RandomState(82).permutation(p.D * p.m)[:128]
    med, ts = median_time(lambda: qf.quad_forms(model._K, qf.GridColumnRows(gk, idx), 128, 128, 1e-4),
                          repeats)
    tiles = -(-(p.D * p.m) // 128)
    emit(dict(part='precompute', problem='c5', n=p.n, Dm=p.D * p.m, variance_batch=128, solver=solver,
              tile_s=med, all_s=ts, tiles=tiles, extrapolated_total_s=med * tiles))


def part_kernels():
    from runlmc_amd.approx import quadforms as qf
    p, model, solver = model_for('c5')
    Xt = test_points(p, 128)
    op = model._light_exact()
    X, lens = np.vstack(Xt), [len(x) for x in Xt]
    op.cross_device(X, lens, 0, 128)
    sync()
    op.cross(X, lens)
    rows = qf.CrossRows(op, X, lens)
    out = qf.quad_forms(model._K, rows, 128, 128, 1e-4)
    sync()
    emit(dict(part='kernels', problem='c5', n=p.n, rows=128, Q=p.Q, solver=solver,
              max_residual=float(out.residuals.max())))


def main():
    global _RECORD
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='e2e,tile,precompute')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--record', default=None)
    a = ap.parse_args()
    if a.record:
        os.makedirs(a.record, exist_ok=True)
        _RECORD = open(os.path.join(a.record, 'predict_probe.jsonl'), 'a')
        err = open(os.path.join(a.record, 'predict_probe.stderr'), 'a')
        sys.stderr.flush()
        os.dup2(err.fileno(), 2)
    import torch
    assert torch.cuda.is_available(), 'predict_probe.py measures the GPU: no GPU visible'
    from runlmc_amd import _lib
    assert _lib.get_library().is_hip
    for part in a.parts.split(','):
        if part == 'kernels':
            part_kernels()
        else:
            {'e2e': part_e2e, 'tile': part_tile, 'precompute': part_precompute}[part](a.repeats)
    if _LINES == 0:
        sys.exit('predict_probe.py: no measurement was written')


if __name__ == '__main__':
    main()
