"""Times of leave-one-out cross-validation (InterpolatedLLGP.loo_predict, runlmc_amd/approx/loo.py,
csrc/rl_loo.h), one JSON line per measurement on stdout:

    python tools/loo_probe.py [--size c5] [--parts direct,probes] [--record profiles/loo]

Problems: runlmc_amd/util/synth.py at C5 (n = 10^6, D = 10, Q = 5) or C2 (n = 20 000).
  direct   family rbf (the factorisation is K~^-1): seconds (median of --repeats after a warm-up,
           each ended by a device synchronisation) of rl_ski_inverse_diag alone, of the whole
           loo_predict and loo_log_likelihood, and of the solve for alpha (Iterative.solve_device
           on y) on the same handle in the same run.
  probes   family matern, 32 probes drawn on the device, solves at 1e-4: seconds of
           inverse_diagonal(method='probes') and the median over the rows of sem / d, with and
           without the control variate, on the 48-function preconditioner (RUNLMC_NO_PRECOND_HI=1:
           rl_ski_factor available = 2) -- and on the handle's own choice at this size (the
           96-function basis, available = 3, which has no diagonal and so no control variate).
--record DIR appends every line to DIR/loo_probe.jsonl and sends stderr to DIR/loo_probe.stderr;
the script fails when it has written no line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {'c2': (4, 3, 1, 5000), 'c5': (10, 5, 1, 100000)}
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
    f()
    sync()
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        f()
        sync()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def model_for(size, family):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    from runlmc_amd.util import synth
    p = synth.make_problem(*SIZES[size], kern=family)
    np.random.seed(5)
    model = InterpolatedLLGP(p.Xs, p.Ys, normalize=False, functional_kernel=synth.functional_kernel(p))
    model.parameters_changed()
    return p, model


def part_direct(size, repeats):
    import torch
    from runlmc_amd.approx.iterative import Iterative
    from runlmc_amd.approx.quadforms import _solver_name
    p, model = model_for(size, 'rbf')
    K = model._K
    ski = K.device_operator()
    ski.factor()
    y = torch.from_numpy(np.ascontiguousarray(model.y))[None, :].to(K.device)
    _, iters, resid, _ = Iterative.solve_device(K, y, tol=1e-4)[:4]
    rec = dict(part='direct', problem=size, family='rbf', n=p.n, D=p.D, Q=p.Q, factor_mode=ski.factor_mode,
               rank=model._grid_kernels[(0,)]._op.form()[0], solver=_solver_name(K),
               alpha_iterations=int(iters[0]), alpha_residual=float(resid[0]))
    rec['inverse_diag_s'] = median_time(lambda: ski.inverse_diag(), repeats)
    rec['alpha_solve_s'] = median_time(lambda: Iterative.solve_device(K, y, tol=1e-4), repeats)
    rec['loo_predict_s'] = median_time(lambda: model.loo_predict(), repeats)
    rec['loo_log_likelihood_s'] = median_time(lambda: model.loo_log_likelihood(), repeats)
    means, variances = model.loo_predict()
    rec['method'] = model.loo_stats['method']
    rec['nonpositive'] = model.loo_stats['nonpositive']
    rec['loo_log_likelihood'] = model.loo_log_likelihood()
    rec['loo_rmse'] = float(np.sqrt(np.mean((np.concatenate(means) - model.y) ** 2)))
    rec['median_variance'] = float(np.median(np.concatenate(variances)))
    # bytes of the diagonal's pass: the table twice (registers, then row by row), 1 / eps, the result
    rec['inverse_diag_gb_per_s'] = 8.0 * p.n * (2 * rec['rank'] + 2) / rec['inverse_diag_s'] / 1e9
    emit(rec)


def part_probes(size, repeats, n_probes=32):
    from runlmc_amd.approx import loo
    from runlmc_amd.approx.quadforms import _solver_name
    for env in ({'RUNLMC_NO_PRECOND_HI': '1'}, {}):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            p, model = model_for(size, 'matern')
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        K = model._K
        ski = K.device_operator()
        ski.factor()
        for cv in (True, False):
            if cv and ski.factor_mode not in (1, 2):
                continue
            run = lambda: loo.inverse_diagonal(K, method='probes', n_probes=n_probes, seed=0, batch=16,
                                               tol=1e-4, control_variate=cv)
            secs = median_time(run, repeats)
            res = run()
            d, sem = res.d.cpu().numpy(), res.sem.cpu().numpy()
            emit(dict(part='probes', problem=size, family='matern', n=p.n, D=p.D, Q=p.Q, env=env,
                      factor_mode=ski.factor_mode, solver=_solver_name(K), n_probes=n_probes,
                      control_variate=bool(res.stats.control_variate), seconds=secs,
                      iterations_max=int(res.stats.iterations.max()),
                      residual_max=float(res.stats.residuals.max()),
                      median_sem_over_d=float(np.median(sem / np.abs(d))),
                      max_sem_over_d=float(np.max(sem / np.abs(d))),
                      nonpositive=int(np.sum(~(d > 0)))))
        del model


def main():
    global _RECORD
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='direct,probes')
    ap.add_argument('--size', default='c5')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--record', default=None)
    a = ap.parse_args()
    if a.record:
        os.makedirs(a.record, exist_ok=True)
        _RECORD = open(os.path.join(a.record, 'loo_probe.jsonl'), 'a')
        err = open(os.path.join(a.record, 'loo_probe.stderr'), 'a')
        sys.stderr.flush()
        os.dup2(err.fileno(), 2)
    import torch
    assert torch.cuda.is_available(), 'loo_probe.py measures the GPU: no GPU visible'
    from runlmc_amd import _lib
    assert _lib.get_library().is_hip
    for part in a.parts.split(','):
        if part == 'direct':
            part_direct(a.size, a.repeats)
        else:
            part_probes(a.size, a.repeats)
    if _LINES == 0:
        sys.exit('loo_probe.py: no measurement was written')


if __name__ == '__main__':
    main()
