"""Which kernels a product or a solve runs, and what it computes, as one JSON line.

    python tools/route_digest.py --list
    python tools/route_digest.py --case NAME [--emu]

One case per process (the library's RUNLMC_TRACE lines are printed once per process).  A case
builds a seeded operator on a small system, with the switches that force the route it is
named after, runs the product or the solve and prints

    {"case": ..., "sha256": <of the output bytes>, "trace": [sorted "[runlmc] ..." lines]}

Two builds of the library that take the same routes and compute the same bits print the same
line: the lines of a refactor are held against its parent's (profiles/routes/).  Shapes are
those of the checks that force these routes onto small systems (tests/parity_suite.py:
check_row_polynomial_form, check_staged_wt_product, check_w_poly_product,
check_polynomial_rounds; the matern52, grid2d, grid3d and pivchol suites).
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGED = dict(RUNLMC_STAGED_WT='1')
UNFUSED = dict(RUNLMC_STAGED_WT='1', RUNLMC_NO_FUSE_W='1', RUNLMC_NO_FUSE_WT='1')


def _np():
    import numpy as np
    return np


def _problem(D, Q, m_data, kern='rbf', sort=False, lens=None):
    """synth.make_problem, optionally with sorted inputs (the handle keeps the caller's row
    order) or outputs cut to `lens` rows (ragged, an empty output)."""
    np = _np()
    from runlmc_amd.util import synth
    from runlmc_amd.approx.interpolation import multi_interpolant
    p = synth.make_problem(D, Q, 1, m_data, eps=1.0, kern=kern)
    if sort or lens is not None:
        lens = list(lens) if lens is not None else p.lens
        p.Xs = [np.sort(x[:l], axis=0) if sort else x[:l] for x, l in zip(p.Xs, lens)]
        p.lens = lens
        p.n = int(sum(lens))
        p.W = multi_interpolant(p.Xs, p.grid)
        p.WT = p.W.transpose().tocsr()
    return p


def _grid(p, gate=None):
    from runlmc_amd.util import synth
    from runlmc_amd._native import GridOp
    g = GridOp(p.D, p.m, p.Q)
    g.set_lmc(synth.tops(p), list(p.coreg_vecs), list(p.coreg_diags))
    if gate is not None:
        g.set_form_gate(gate)
    return g


def _ski(p, gate=None, W=None):
    from runlmc_amd._native import SkiOp
    g = _grid(p, gate)
    W = p.W if W is None else W
    s = SkiOp(g, W, W.transpose().tocsr())
    s.set_noise(p.noise + 0.5, p.lens)
    return s


def _vectors(k, width, seed=29):
    return _np().random.RandomState(seed).randn(k, width)


def grid_case(D, Q, m_data, k, kern='rbf', gate=None, top=None):
    def run():
        p = _problem(D, Q, m_data, kern)
        g = _grid(p, gate)
        return g.matmat_host(_vectors(k, g.width), top=top)
    return run


def lattice_case(sizes, D, Q, k):
    """A 2-D or 3-D grid product: anisotropic top rows that differ per q."""
    def run():
        np = _np()
        from runlmc_amd._native import GridOp
        rng = np.random.RandomState(7)
        idx = np.meshgrid(*[np.arange(s, dtype=float) for s in sizes], indexing='ij')
        r = np.sqrt(sum(((1.0 + 0.3 * a) * i) ** 2 for a, i in enumerate(idx)))
        tops = np.array([np.exp(-(0.05 + 0.11 * q) * r).ravel() for q in range(Q)])
        g = GridOp(D, int(np.prod(sizes)), Q, sizes=sizes)
        g.set_lmc(tops, [rng.randn(1, D) for _ in range(Q)],
                  [np.abs(rng.randn(D)) + 0.1 for _ in range(Q)])
        return g.matmat_host(_vectors(k, g.width))
    return run


def ski_case(D, Q, m_data, k, kern='rbf', gate=None, sort=False, lens=None, interleave=False):
    def run():
        np = _np()
        p = _problem(D, Q, m_data, kern, sort=sort, lens=lens)
        W = p.W
        if interleave:
            W = W[np.random.RandomState(3).permutation(p.n)].tocsr()
        s = _ski(p, gate, W)
        return s.matmat_host(_vectors(k, p.n))
    return run


def two_term_case(k):
    """A second term on a grid of its own (another length)."""
    def run():
        np = _np()
        from runlmc_amd.util import synth
        from runlmc_amd.approx.interpolation import autogrid, multi_interpolant
        from runlmc_amd._native import GridOp
        p = _problem(3, 2, 300)
        s = _ski(p)
        grid2 = autogrid(p.Xs, lo=None, hi=None, m=[200])[0]
        g2 = GridOp(p.D, len(grid2), 1)
        g2.set_lmc(np.array([np.exp(-3.0 * (grid2 - grid2[0]))]), [p.coreg_vecs[0]],
                   [p.coreg_diags[1]])
        W2 = multi_interpolant(p.Xs, grid2)
        s.add_term(g2, W2, W2.transpose().tocsr())
        return s.matmat_host(_vectors(k, p.n))
    return run


def solve_case(D, Q, m_data, k, kern='rbf', gate=None, lens=None, method=0, how='batch'):
    def run():
        np = _np()
        import torch
        from runlmc_amd import _native as nat
        p = _problem(D, Q, m_data, kern, lens=lens)
        s = _ski(p, gate)
        B = torch.from_numpy(_vectors(k, p.n)).to(s.device)
        if how == 'pcg':
            out = nat.solve_pcg(s, B, tol=1e-6, maxiter=6)
        elif how == 'direct':
            out = nat.solve_direct(s, B, tol=1e-6)
        else:
            out = nat.solve_batch(s, B, method=method, tol=1e-6, maxiter=6)
        return np.concatenate([out[0].cpu().numpy().ravel(), np.asarray(out[1], dtype=float),
                               np.asarray(out[3], dtype=float)])
    return run


def pivchol_2d_case(k):
    """solve_pcg on a two-input operator (RBF + Matern-3/2 on a 20 x 260 grid) with the
    pivoted-Cholesky preconditioner of rank 32."""
    def run():
        np = _np()
        import torch
        from runlmc_amd import _native as nat
        from runlmc_amd.approx.interpolation import autogrid, multi_interpolant
        from runlmc_amd.kern.stationary import RBF, Matern32
        rng = np.random.RandomState(40)
        D, shape, lens = 2, (20, 260), (150, 17)
        Xs = [rng.rand(n, 2) for n in lens]
        axes = autogrid(Xs, lo=None, hi=None, m=np.array([shape[0] - 4, shape[1] - 4]))
        dists = np.sqrt((axes[0][:, None] - axes[0][0]) ** 2 + (axes[1][None, :] - axes[1][0]) ** 2)
        W = multi_interpolant(Xs, *axes)
        g = nat.GridOp(D, dists.size, 2, sizes=dists.shape)
        g.set_lmc(np.array([RBF(3.0).from_dist(dists).ravel(), Matern32(2.0).from_dist(dists).ravel()]),
                  [rng.uniform(-1, 1, size=(r, D)) for r in (1, 2)],
                  [0.2 + rng.rand(D) for _ in range(2)])
        s = nat.SkiOp(g, W, W.transpose().tocsr())
        s.set_noise(0.1 + 0.4 * rng.rand(D), lens)
        s.set_pivchol(32)
        out = nat.solve_pcg(s, torch.from_numpy(_vectors(k, sum(lens))).to(s.device), tol=1e-6, maxiter=6)
        return np.concatenate([out[0].cpu().numpy().ravel(), np.asarray(out[1], dtype=float),
                               np.asarray(out[3], dtype=float)])
    return run


RAGGED3 = (2600, 2600 // 3 + 5, 2600 - 131)

# name -> (environment switches, function that returns the output array)
CASES = {
    # grid products
    'grid_transform': ({}, grid_case(3, 2, 296, 3, gate=1 << 62)),
    'grid_k1_product': ({}, grid_case(2, 2, 96, 4, gate=1 << 62)),
    'grid_2d': ({}, lattice_case((5, 7), 2, 1, 3)),
    'grid_3d': ({}, lattice_case((2, 5, 7), 2, 2, 3)),
    'grid_poly_all': ({}, grid_case(3, 2, 2596, 3, gate=0)),
    'grid_poly_top': ({}, grid_case(3, 2, 2596, 3, gate=0, top=1)),
    'grid_filter': ({}, grid_case(3, 2, 1500, 3, kern='matern', gate=0)),
    'grid_filter_top': ({}, grid_case(3, 2, 1500, 3, kern='matern', gate=0, top=1)),
    'grid_filter_poly': ({}, grid_case(2, 3, 1200, 3, kern='mix', gate=0)),
    'grid_poly_small': ({}, grid_case(3, 2, 2596, 2)),
    # K~ products
    'ski_plain': ({}, ski_case(3, 2, 400, 5)),
    'ski_staged': (dict(STAGED, RUNLMC_NO_RP='1'), ski_case(3, 2, 400, 37)),
    'ski_w_poly': (dict(STAGED, RUNLMC_NO_RP='1'), ski_case(3, 2, 2600, 37, gate=0)),
    'ski_rp_internal': (STAGED, ski_case(3, 2, 2600, 37, gate=0, sort=True, lens=RAGGED3)),
    'ski_rp_caller': (STAGED, ski_case(3, 2, 2600, 37, gate=0, lens=RAGGED3)),
    'ski_rp_interleaved': (STAGED, ski_case(3, 2, 2600, 17, gate=0, lens=RAGGED3, interleave=True)),
    'ski_rp_k5': (STAGED, ski_case(3, 2, 2600, 5, gate=0, lens=RAGGED3)),
    'ski_rp_k17': (STAGED, ski_case(3, 2, 2600, 17, gate=0, lens=RAGGED3)),
    'ski_rp_k33': (STAGED, ski_case(3, 2, 2600, 33, gate=0, lens=RAGGED3)),
    'ski_rp_rank_above_24': (STAGED, ski_case(2, 2, 2600, 11, kern='periodic', gate=0,
                                              lens=(2600 - 77, 129))),
    'ski_two_terms': ({}, two_term_case(5)),
    # solve_batch, six iterations
    'solve_small_fused': ({}, solve_case(3, 2, 300, 3)),
    'solve_poly_rounds': (dict(RUNLMC_POLY_ROUND='1'), solve_case(3, 2, 300, 5)),
    'solve_cg': ({}, solve_case(3, 2, 300, 3, method=1)),
    'solve_matern_staged_w': (UNFUSED, solve_case(3, 2, 700, 11, kern='matern', gate=0)),
    # other solves
    'pcg_matern': (dict(RUNLMC_PRECOND_HI_MIN='0'), solve_case(2, 2, 1000, 3, kern='matern', how='pcg')),
    'pcg_2d_pivchol': ({}, pivchol_2d_case(3)),
    'direct_rbf': ({}, solve_case(2, 2, 400, 3, how='direct')),
}
for _k in (3, 17, 37):
    for _tag, _env in (('', {}), ('_no_pfuse', dict(RUNLMC_NO_RP_PFUSE='1')),
                       ('_no_fuse', dict(RUNLMC_NO_RP_FUSE='1'))):
        CASES['solve_rp%s_k%d' % (_tag, _k)] = (dict(UNFUSED, **_env),
                                                solve_case(3, 2, 2600, _k, gate=0, lens=RAGGED3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--case')
    ap.add_argument('--list', action='store_true')
    ap.add_argument('--emu', action='store_true', help='the emulator build instead of the device')
    args = ap.parse_args()
    if args.list or not args.case:
        print('\n'.join(CASES))
        return 0
    env, run = CASES[args.case]
    for name in [n for n in os.environ if n.startswith('RUNLMC_')]:
        del os.environ[name]
    os.environ.update(env, RUNLMC_TRACE='1', RUNLMC_DEBUG='1')
    from runlmc_amd import _lib, build
    if args.emu:
        _lib.use_library(build.build_emu())
    # the library writes its trace to the process's stderr: into a file for the run
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode='w+b') as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = run()
        finally:
            sys.stderr.flush()
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        lines = tmp.read().decode(errors='replace').splitlines()
    trace = sorted(l for l in lines if l.startswith('[runlmc]'))
    for l in lines:
        if not l.startswith('[runlmc]'):
            print(l, file=sys.stderr)
    out = _np().ascontiguousarray(out, dtype=_np().float64)
    print(json.dumps({'case': args.case, 'sha256': hashlib.sha256(out.tobytes()).hexdigest(),
                      'trace': trace}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
