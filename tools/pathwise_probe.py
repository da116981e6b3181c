"""Times of the function draws (InterpolatedLLGP.posterior_draws, runlmc_amd/approx/pathwise.py,
csrc/rl_sample.h), one JSON line per measurement on stdout:

    python tools/pathwise_probe.py [--sizes c2,c5] [--families rbf,matern,mix] [--record profiles/pathwise]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pathwise_probe.py --parts kernels

Problems: runlmc_amd/util/synth.py at C2 (n = 20 000) and C5 (n = 10^6), 16 draws per tile.
  tile     per (size, family): what the sampler chose per row (form, Ls, rank, clipped), seconds
           (median of --repeats after a warm-up, each ended by a device synchronisation) of
           the noise of a tile (rl_normal_fill: the grid noise and e), of the prior tile
           (rl_sampler_draw from a filled buffer), of rl_gridop_mvm on 16 vectors of the same
           handle in the same run, and of the posterior tile's solve (Iterative.solve_device on
           the tile's residuals) and back-projection (W^T, K_UU, the sum); bytes read and
           written per draw by the prior tile -- algorithmic (noise read once) and as launched
           (the embedding rows' noise read once per output) -- and their shares of 8 TB/s.
  kernels  one posterior tile per (size, family) for a kernel trace, no timing here.
--record DIR appends every line to DIR/pathwise_probe.jsonl and sends stderr to
DIR/pathwise_probe.stderr; the script fails when it has written no line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {'c2': (4, 3, 1, 5000), 'c5': (10, 5, 1, 100000)}
DRAWS = 16
HBM_BYTES_PER_S = 8e12
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


def tile_pieces(model):
    import torch
    from runlmc_amd.approx import pathwise as pw
    from runlmc_amd._native import pathwise_residual
    K = model._K
    ski = K.device_operator()
    t = time.perf_counter()
    (s,) = model._pathwise_samplers(16)
    sync()
    set_s = time.perf_counter() - t
    n = len(model.y)
    y = torch.from_numpy(np.ascontiguousarray(model.y)).to(K.device)
    sq = torch.from_numpy(np.sqrt(K.Ks[-1].v)).to(K.device)
    noise = lambda: (s.noise(pw.stream_seed(0, pw.STREAM_TERM0), 0, DRAWS),
                     pw.normal_fill(ski.lib, pw.stream_seed(0, pw.STREAM_E), 0, DRAWS, n, K.device))
    Z, E = noise()
    U = s.draw(Z, DRAWS)
    R = pathwise_residual(ski.lib, y, ski.apply_w(U), E, sq)
    from runlmc_amd.approx.iterative import Iterative
    solve = lambda: Iterative.solve_device(K, R, tol=1e-4)
    V, iters, resid, _ = solve()[:4]
    back = lambda: U + s.grid.mvm(ski.apply_wt(V))
    return dict(s=s, set_s=set_s, noise=noise, Z=Z, U=U, solve=solve, back=back,
                iters=int(np.max(iters)), resid=float(np.max(resid)),
                residual=lambda: pathwise_residual(ski.lib, y, ski.apply_w(U), E, sq))


def part_tile(sizes, families, repeats):
    from runlmc_amd.approx.quadforms import _solver_name
    for size in sizes:
        for family in families:
            p, model = model_for(size, family)
            t = tile_pieces(model)
            s = t['s']
            Dm = s.grid.width
            rec = dict(part='tile', problem=size, family=family, n=p.n, D=p.D, Q=p.Q, m=s.grid.m, draws=DRAWS,
                       rows=[st._asdict() for st in s.stats], zlen=s.zlen, sampler_set_s=t['set_s'],
                       solver=_solver_name(model._K), solve_iterations=t['iters'], solve_residual=t['resid'])
            rec['noise_s'] = median_time(t['noise'], repeats)
            rec['prior_s'] = median_time(lambda: s.draw(t['Z'], DRAWS), repeats)
            rec['gridop_mvm16_s'] = median_time(lambda: s.grid.mvm(t['U']), repeats)
            rec['residual_s'] = median_time(t['residual'], repeats)
            rec['solve_s'] = median_time(t['solve'], repeats)
            rec['back_projection_s'] = median_time(t['back'], repeats)
            # bytes of the prior tile per draw.  Algorithmic: the noise read once, the draws written,
            # the two-pass path's intermediates written and read.  As launched: the D workgroups
            # of a tile each read the noise of the embedding rows (measured: they do not share an
            # L2), so that part counts D times.
            two_pass = any(st.form == 'embedding' and np.prod(st.Ls) > 2048 for st in s.stats)
            Ltot = max([int(np.prod(st.Ls)) for st in s.stats if st.form == 'embedding'], default=0)
            inter = 2 * 8 * p.D * Ltot if two_pass else 0
            emb_noise = 8 * sum(int(np.prod(st.Ls)) * c for st, c in zip(s.stats, s.channels)
                                if st.form == 'embedding')
            rec['prior_bytes_per_draw_algorithmic'] = 8 * s.zlen + 8 * Dm + inter
            rec['prior_bytes_per_draw_as_launched'] = 8 * s.zlen + (p.D - 1) * emb_noise + 8 * Dm + inter
            for kind in ('algorithmic', 'as_launched'):
                rec['prior_share_of_8TBs_' + kind] = (rec['prior_bytes_per_draw_' + kind] * DRAWS /
                                                      rec['prior_s'] / HBM_BYTES_PER_S)
            rec['noise_gb_per_s'] = 8 * DRAWS * (s.zlen + p.n) / rec['noise_s'] / 1e9
            emit(rec)
            del model, t


def part_kernels(sizes, families):
    for size in sizes:
        for family in families:
            p, model = model_for(size, family)
            draws = model.posterior_draws(DRAWS, seed=0)
            sync()
            emit(dict(part='kernels', problem=size, family=family, n=p.n, draws=DRAWS,
                      max_residual=max(i.max_residual for i in draws.info)))
            del model


def main():
    global _RECORD
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='tile')
    ap.add_argument('--sizes', default='c2,c5')
    ap.add_argument('--families', default='rbf,matern,mix')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--record', default=None)
    a = ap.parse_args()
    if a.record:
        os.makedirs(a.record, exist_ok=True)
        _RECORD = open(os.path.join(a.record, 'pathwise_probe.jsonl'), 'a')
        err = open(os.path.join(a.record, 'pathwise_probe.stderr'), 'a')
        sys.stderr.flush()
        os.dup2(err.fileno(), 2)
    import torch
    assert torch.cuda.is_available(), 'pathwise_probe.py measures the GPU: no GPU visible'
    from runlmc_amd import _lib
    assert _lib.get_library().is_hip
    sizes, families = a.sizes.split(','), a.families.split(',')
    for part in a.parts.split(','):
        if part == 'kernels':
            part_kernels(sizes, families)
        else:
            part_tile(sizes, families, a.repeats)
    if _LINES == 0:
        sys.exit('pathwise_probe.py: no measurement was written')


if __name__ == '__main__':
    main()
