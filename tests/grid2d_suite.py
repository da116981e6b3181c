"""Two-dimensional (BTTB) grids across the transform kernels' plans, limits and routes.

Shared by the GPU run (tests/test_grid2d_gpu.py, librunlmc_hip.so on an MI355X) and the CPU
run (tests/test_grid2d_emu.py, the same kernel source under the thread-level emulator).
Every function uses whichever native library is active.

A 2-D grid has one device path -- k_cols_fwd -> k_rows_mix -> k_cols_inv and their second- and
third-generation forms -- planned per shape in gridop_create_impl and per launch in
choose_tiles (csrc/rl_gridop.hip).  The polynomial, filter, single-tile and pair-affine forms
are off when m1 != 0.

References.  Every grid product is held to two independent ones:
  1. the oracle: ops.grid_sum_matvec over ops.BTTBOracle(top, sizes) (NumPy rfftn), every
     vector, every entry;
  2. the plain double sum in np.longdouble,
         y[a, (i1,i2)] = sum_b B[a,b] sum_{j1,j2} top[|i1-j1|, |i2-j2|] x[b, (j1,j2)],
     on sampled entries of every output block: the four corners, one point on each edge, the
     centre and 24 seeded random points.
Tolerance: the transform kernels' stated bar (tests/test_gpu_mvm.py), 1e-11 of max|y| (per
vector), against both.  The tops are anisotropic and differ per q, so a swap of the axes or a
mirror on the wrong axis changes the answer; A_q has ranks 1, 2, 0 across q.

Not covered, because it does not exist: an LDS-staged W^T / W product of a bicubic W.  The
staged kernels take rows of at most four consecutive entries (cubic W on a 1-D grid), so
RUNLMC_STAGED_WT is inert on a 2-D model; check_ski_2d_operator pins that and says what the
knobs of the issue do exercise (the solver's unfused rounds).

Each check prints the worst error it measured (pytest -s shows them; profiles/grid2d/README.md
holds those of the GPU run).
"""
import functools
import os

import numpy as np
import torch

from oracle import operators as ops
from oracle import likelihood as olik
from oracle import interp as ointerp
from oracle.kernels import KernelSpec, RBFSpec, Matern32Spec

REL = 1e-11

# m1, m2, D, Q, nvec, N1, N2 -- what each row reaches is in the comment
LATTICE = [
    (1, 1, 1, 1, 3, 4, 4),              # degenerate axes: the floor of 4 on both
    (1, 7, 2, 1, 3, 4, 16),             # ... on the first
    (5, 1, 3, 1, 3, 16, 4),             # ... on the second
    (32, 64, 2, 2, 3, 64, 128),         # mirror with no gap (N = 2 m on both axes)
    (33, 65, 2, 2, 3, 128, 256),        # mirror with the largest gap (N = 4 m - 4)
    (2, 600, 1, 2, 3, 4, 2048),         # generic row plan 8.8.8.4, first-generation kernels
    (600, 2, 2, 1, 3, 2048, 4),         # long columns, narrow tile
    (1100, 2, 1, 1, 2, 4096, 4),        # longest admitted axis, columns
    (2, 1100, 1, 1, 2, 4, 4096),        # longest admitted axis, rows
    (20, 40, 3, 2, 5, 64, 128),         # third-generation rows (8, 8)
    (40, 70, 16, 2, 2, 128, 256),       # third-generation rows at D = 16
    (70, 40, 5, 3, 17, 256, 128),       # 9 pairs, tiles shrunk for small launches
    (40, 130, 7, 2, 3, 128, 512),       # third-generation rows (16, 16)
    (130, 300, 2, 2, 3, 512, 1024),     # second-generation rows at 1024
    (300, 130, 2, 2, 3, 1024, 512),     # three-pass columns
    (300, 300, 1, 1, 2, 1024, 1024),    # largest L in the table (16 MB per pair)
    (520, 33, 3, 1, 3, 2048, 128),      # no fused column code: first-generation kernels
    (1025, 40, 1, 2, 3, 4096, 128),     # second-generation kernels with C = 1
    (40, 70, 17, 2, 3, 128, 256),       # wide operator in 2-D
    (2, 600, 20, 2, 3, 4, 2048),        # wide operator on the generic row plan
]


def lattice_id(row):
    return '%dx%d-D%d-Q%d-v%d' % row[:5]


def _say(name, **errs):
    print('grid2d %s: %s' % (name, '  '.join('%s %.2e' % kv for kv in errs.items())), flush=True)


def make_tops(m1, m2, Q):
    """Anisotropic top rows, different per q: exp(-a_q sqrt(i1^2 + (0.7 i2)^2)) (1 + 0.1 i2 / m2)."""
    i1, i2 = np.meshgrid(np.arange(m1, dtype=float), np.arange(m2, dtype=float), indexing='ij')
    r = np.sqrt(i1 ** 2 + (0.7 * i2) ** 2)
    return np.array([(np.exp(-(0.05 + 0.11 * q) * r) * (1 + 0.1 * i2 / m2)).ravel()
                     for q in range(Q)])


def make_coreg(rng, D, Q):
    """A_q of ranks 1, 2, 0 across q (B_q = A_q^T A_q + diag kappa_q)."""
    A = [rng.randn((1, 2, 0)[q % 3], D) for q in range(Q)]
    kap = [np.abs(rng.randn(D)) + 0.1 for _ in range(Q)]
    return A, kap


def sample_points(rng, m1, m2, D):
    """Per output block: corners, one point on each edge, the centre, 24 random points."""
    fixed = [(0, 0), (0, m2 - 1), (m1 - 1, 0), (m1 - 1, m2 - 1),
             (0, m2 // 2), (m1 - 1, m2 // 3), (m1 // 2, 0), (m1 // 3, m2 - 1),
             (m1 // 2, m2 // 2)]
    out = []
    for _ in range(D):
        rnd = list(zip(rng.randint(0, m1, 24), rng.randint(0, m2, 24)))
        out.append(np.array(fixed + rnd, dtype=np.int64))
    return out


def direct_samples(tops, sizes, Bs, X, points):
    """The double sum in np.longdouble at points[a] of output block a, for every vector:
    list over a of (nvec, npts) arrays."""
    m1, m2 = sizes
    m = m1 * m2
    D = len(points)
    Xl = np.asarray(X, dtype=np.longdouble).reshape(-1, D, m)
    j1, j2 = np.arange(m1), np.arange(m2)
    out = []
    for a in range(D):
        p = points[a]
        l1 = np.abs(p[:, 0, None] - j1[None, :])           # (npts, m1)
        l2 = np.abs(p[:, 1, None] - j2[None, :])           # (npts, m2)
        val = np.zeros((Xl.shape[0], len(p)), dtype=np.longdouble)
        for q, top in enumerate(tops):
            t = np.asarray(top, dtype=np.longdouble).reshape(m1, m2)
            T = t[l1[:, :, None], l2[:, None, :]].reshape(len(p), m)
            xm = np.tensordot(np.asarray(Bs[q][a], dtype=np.longdouble), Xl, axes=(0, 1))
            val += xm.dot(T.T)
        out.append(val)
    return out


def _vs_oracle(got, ref):
    """worst over vectors of max|got - ref| / max|ref|"""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    scale = np.maximum(np.abs(ref).max(axis=1), 1e-300)
    return float((np.abs(got - ref).max(axis=1) / scale).max())


def _vs_direct(got, ref, sizes, direct, points):
    m = sizes[0] * sizes[1]
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    scale = np.maximum(np.abs(ref).max(axis=1), 1e-300)
    worst = 0.0
    for a, (p, val) in enumerate(zip(points, direct)):
        idx = a * m + p[:, 0] * sizes[1] + p[:, 1]
        err = np.abs(got[:, idx].astype(np.longdouble) - val).max(axis=1) / scale
        worst = max(worst, float(err.max()))
    return worst


def product_errors(g, tops, sizes, Bs, X, seed=0, vectors=None):
    """(Y, error vs the oracle, error vs the direct sum) of g's product of X; `vectors`
    restricts the references to some of the batch."""
    Y = g.matmat_host(X)
    sel = list(range(len(X))) if vectors is None else sorted(set(vectors))
    toeps = [ops.BTTBOracle(t, sizes) for t in tops]
    ref = np.array([ops.grid_sum_matvec(Bs, toeps, X[v]) for v in sel])
    points = sample_points(np.random.RandomState(1000 + seed), sizes[0], sizes[1], g.D)
    direct = direct_samples(tops, sizes, Bs, X[sel], points)
    # the two references against each other (the direct sum is the more exact one)
    assert _vs_direct(ref, ref, sizes, direct, points) < 1e-14
    return Y, _vs_oracle(Y[sel], ref), _vs_direct(Y[sel], ref, sizes, direct, points), ref


def embedded_spectrum(top, sizes, N1, N2):
    """Real spectrum of the N1 x N2 circulant embedding, (N1, N2 // 2 + 1)."""
    m1, m2 = sizes
    if (N1, N2) == (ops.next_pow2(2 * m1), ops.next_pow2(2 * m2)):
        return ops.bttb_spectrum(top, sizes).real
    # a degenerate axis (one point: the reference's length is 2, the device's floor is 4):
    # the same embedding rule at the device's lengths
    col = np.zeros((N1, N2))
    col[:m1, :m2] = np.reshape(top, sizes)
    if m2 > 1:
        col[:, N2 - m2 + 1:] = col[:, m2 - 1:0:-1]
    if m1 > 1:
        col[N1 - m1 + 1:, :] = col[m1 - 1:0:-1, :]
    return np.fft.rfft2(col).real


def check_unit_columns(g, tops, sizes, Bs):
    """K e_j for e_j at grid points (0,0), (m1-1,m2-1), (0,m2-1) of one output equals the dense
    column -- top indexed at the per-axis lags -- to 1e-13 of its maximum."""
    m1, m2 = sizes
    m, D = m1 * m2, g.D
    b0 = D // 2
    i1, i2 = np.meshgrid(np.arange(m1), np.arange(m2), indexing='ij')
    pts = [(0, 0), (m1 - 1, m2 - 1), (0, m2 - 1)]
    E = np.zeros((len(pts), D * m))
    want = np.zeros_like(E)
    for k, (j1, j2) in enumerate(pts):
        E[k, b0 * m + j1 * m2 + j2] = 1.0
        lag = [np.reshape(t, sizes)[np.abs(i1 - j1), np.abs(i2 - j2)].ravel() for t in tops]
        for a in range(D):
            want[k, a * m:(a + 1) * m] = sum(B[a, b0] * l for B, l in zip(Bs, lag))
    got = g.matmat_host(E)
    err = float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max())
    assert err < 1e-13, 'unit columns: %.3e' % err
    return err


def _new_grid(m1, m2, D, Q):
    from runlmc_amd._native import GridOp
    return GridOp(D, m1 * m2, Q, sizes=(m1, m2))


# --- 1. the plan lattice -------------------------------------------------------------------
def check_plan_lattice(m1, m2, D, Q, nvec, N1=None, N2=None):
    sizes = (m1, m2)
    rng = np.random.RandomState(7919 * m1 + 31 * m2 + D)
    tops = make_tops(m1, m2, Q)
    A, kap = make_coreg(rng, D, Q)
    Bs = ops.coreg_mats(A, kap)
    g = _new_grid(m1, m2, D, Q)
    if N1 is not None:      # (guards the coverage the table claims; not a tolerance)
        assert (g.N1, g.N2) == (N1, N2), (g.N1, g.N2)
    if g.N1 == 4096:        # a column tile of one column is all that fits the LDS
        assert g.colsA == 1, g.colsA
    assert g.N2 % g.colsA == 0 and g.N1 % g.rowsB == 0, (g.colsA, g.rowsB)
    assert g.L == g.N1 * g.N2
    g.set_lmc(tops, A, kap)
    X = rng.randn(nvec, D * m1 * m2)
    Y, e_or, e_dir, ref = product_errors(g, tops, sizes, Bs, X, seed=m1 + m2)
    e_col = check_unit_columns(g, tops, sizes, Bs)
    # <x, K y> = <K x, y>
    lhs, rhs = float(X[0].dot(Y[1])), float(Y[0].dot(X[1]))
    e_sym = abs(lhs - rhs) / max(abs(lhs), 1.0)
    # single top
    Y1 = g.matmat_host(X, top=Q - 1)
    T = ops.BTTBOracle(tops[Q - 1], sizes)
    ref1 = np.array([np.concatenate([T.matvec(r) for r in x.reshape(D, -1)]) for x in X])
    e_top = _vs_oracle(Y1, ref1)
    # spectra, natural order: entry (k1, k2) at k1 N2 + k2
    e_spec = 0.0
    for q in range(Q):
        want = embedded_spectrum(tops[q], sizes, g.N1, g.N2)
        got = g.spectrum(q).reshape(g.N1, g.N2)[:, :g.N2 // 2 + 1]
        e_spec = max(e_spec, float(np.abs(got - want).max() / np.abs(want).max()))
    # the dense-B entry point is the same operator
    g.set_dense(tops, np.array(Bs))
    Yd = g.matmat_host(X)
    e_dense = _vs_oracle(Yd, Y)
    _say('lattice %s N %dx%d' % (lattice_id((m1, m2, D, Q, nvec)), g.N1, g.N2), oracle=e_or,
         direct=e_dir, unit=e_col, top=e_top, spectrum=e_spec, dense=e_dense, symmetry=e_sym)
    assert e_or < REL, e_or
    assert e_dir < REL, e_dir
    assert e_top < REL, e_top
    assert e_spec < REL, e_spec
    assert e_dense < REL and _vs_oracle(Yd, ref) < REL, e_dense
    assert e_sym < 1e-10, e_sym


# --- 2. limits -----------------------------------------------------------------------------
# gridop_create_impl: N_k = pow2 >= 2 m_k (floor 4); a column tile of one column and a row
# tile of one row of one output must fit 156 KiB of LDS, (N + N) * 16 bytes <= 159744, so
# N <= 4096 per axis; a row tile of D outputs, (N2 (D | 1) + N2) * 16 bytes, fits for
# D <= 7 / 3 / 1 at N2 = 1024 / 2048 / 4096 -- beyond, and for D > 16, the handle is the wide
# operator (a child with D = 1 and k_wide_mix).
ADMITTED = [(40, 300, 7), (40, 300, 17), (40, 600, 3), (40, 1100, 1)]       # always were
WIDE_ROUTE = [(40, 300, 8), (40, 300, 16), (40, 600, 4), (40, 1100, 2)]     # refused before
REFUSED = [(40, 2049, 1), (2049, 2, 1)]                                     # N = 8192


def check_limit_shape(m1, m2, D, Q=2, nvec=3):
    """One admitted shape: correct against both references."""
    sizes = (m1, m2)
    rng = np.random.RandomState(101 * m2 + D)
    tops = make_tops(m1, m2, Q)
    A, kap = make_coreg(rng, D, Q)
    Bs = ops.coreg_mats(A, kap)
    g = _new_grid(m1, m2, D, Q)
    g.set_lmc(tops, A, kap)
    X = rng.randn(nvec, D * m1 * m2)
    Y, e_or, e_dir, ref = product_errors(g, tops, sizes, Bs, X, seed=D)
    Y1 = g.matmat_host(X[:1], top=0)
    T = ops.BTTBOracle(tops[0], sizes)
    e_top = _vs_oracle(Y1, np.concatenate([T.matvec(r) for r in X[0].reshape(D, -1)]))
    _say('limits %dx%d D=%d N %dx%d' % (m1, m2, D, g.N1, g.N2), oracle=e_or, direct=e_dir,
         top=e_top)
    assert e_or < REL and e_dir < REL and e_top < REL, (e_or, e_dir, e_top)


def check_refusals():
    """More than 2048 points on an axis: NotImplementedError from the host check, before any
    launch; the process stays usable."""
    import pytest
    for m1, m2, D in REFUSED:
        with pytest.raises(NotImplementedError, match='LDS'):
            _new_grid(m1, m2, D, 1)
    with pytest.raises(NotImplementedError, match='LDS'):
        _new_grid(40, 2049, 8, 1)       # (the wide route's child meets the same limit)
    check_plan_lattice(5, 7, 2, 2, 3, 16, 16)


def check_wide_consumers():
    """What takes a wide 2-D handle and what refuses it: the SKI operator and the Krylov solver
    take it (the fused W^T gather and the polynomial forms step aside: rl_ski.hip, rl_solve.hip
    test g->wide), the direct solve refuses with NotImplementedError naming the reason, the
    sampler reads the grid's geometry only (rl_sampler_create: a handle is made on it; its
    polynomial rows are refused on any 2-D grid)."""
    import scipy.sparse
    from runlmc_amd._native import SkiOp, Sampler, solve_batch
    m1, m2, D, Q = 4, 1030, 2, 2             # N2 = 4096: D = 2 is wide
    m = m1 * m2
    rng = np.random.RandomState(9)
    tops = make_tops(m1, m2, Q)
    A, kap = make_coreg(rng, D, Q)
    Bs = ops.coreg_mats(A, kap)
    g = _new_grid(m1, m2, D, Q)
    g.set_lmc(tops, A, kap)
    n_o = 12
    rows = []
    for d in range(D):
        Wd = scipy.sparse.random(n_o, m, density=4.0 / m, random_state=rng, format='csr')
        rows.append(Wd)
    W = scipy.sparse.block_diag(rows, format='csr')
    W.sort_indices()
    WT = W.transpose().tocsr()
    WT.sort_indices()
    s = SkiOp(g, W, WT)
    noise = np.array([0.3, 0.4])
    s.set_noise(noise, [n_o] * D)
    toeps = [ops.BTTBOracle(t, (m1, m2)) for t in tops]
    mv = lambda v: ops.full_matvec(W, WT, lambda u: ops.grid_sum_matvec(Bs, toeps, u),
                                   np.repeat(noise, n_o), v)
    V = rng.randn(3, D * n_o)
    ref = np.array([mv(v) for v in V])
    e_ski = _vs_oracle(s.matmat_host(V), ref)
    Xs, it, res = solve_batch(s, torch.from_numpy(V).to(s.device), tol=1e-8)[:3]
    Xs = Xs.cpu().numpy()
    for i in range(len(V)):
        true = np.linalg.norm(V[i] - mv(Xs[i]))
        assert abs(true - res[i]) <= 1e-9 + 1e-6 * true, (true, res[i])
        assert true < 1e-3 * np.linalg.norm(V[i])     # (a solve took place)
    ok, _, _ = s.factor()
    assert not ok and 'LDS row tile' in s.factor_reason, s.factor_reason
    import pytest
    from runlmc_amd._native import solve_direct
    with pytest.raises(NotImplementedError, match='LDS row tile'):
        solve_direct(s, torch.from_numpy(V).to(s.device))
    smp = Sampler(g)
    assert smp.handle.value
    with pytest.raises(ValueError, match='1-D grids only'):
        smp.set([np.ones((D, 1))], [1], poly_rank=24, poly_sqrt=[np.eye(24)])
    _say('wide consumers %dx%d D=%d' % (m1, m2, D), ski=e_ski, residual=float(np.max(res)))
    assert e_ski < REL, e_ski


# --- 3. the 2-D model on the fused kernels -------------------------------------------------
SKI_CASES = {
    # D, grid, embedding, lens
    'A': (3, (36, 70), (128, 256), (150, 17, 120)),     # third-generation rows
    'B': (2, (20, 260), (64, 1024), (150, 17)),         # second-generation rows
    'C': (2, (520, 6), (2048, 16), (17, 150)),          # first-generation kernels
}


class _Problem:
    pass


@functools.lru_cache(maxsize=None)
def ski_problem(case):
    """Seeded two-input problem and its references (computed once, shared by the tests)."""
    from runlmc_amd.approx.interpolation import autogrid, multi_interpolant
    D, shape, emb, lens = SKI_CASES[case]
    rng = np.random.RandomState(40 + ord(case))
    p = _Problem()
    p.D, p.Q, p.lens, p.shape, p.emb, p.ad = D, 2, list(lens), shape, emb, (0, 1)
    p.n = sum(lens)
    p.Xs = [rng.rand(n, 2) for n in lens]
    p.Ys = [np.sin(4 * X[:, 0] + d) * np.cos(3 * X[:, 1]) + 0.1 * rng.randn(len(X))
            for d, X in enumerate(p.Xs)]
    p.y = np.hstack(p.Ys)
    p.axes = autogrid(p.Xs, lo=None, hi=None, m=np.array([shape[0] - 4, shape[1] - 4]))
    assert tuple(len(a) for a in p.axes) == shape
    d0 = p.axes[0][:, None] - p.axes[0][0]
    d1 = p.axes[1][None, :] - p.axes[1][0]
    p.dists = np.sqrt(d0 ** 2 + d1 ** 2)                 # distances to grid point (0, 0)
    p.W = multi_interpolant(p.Xs, *p.axes)
    p.WT = p.W.transpose().tocsr()
    p.gammas = (3.0, 2.0)
    p.coreg_vecs = [rng.uniform(-1, 1, size=(r, D)) for r in (1, 2)]
    p.coreg_diags = [0.2 + rng.rand(D) for _ in range(2)]
    p.noise = 0.1 + 0.4 * rng.rand(D)
    p.spec = KernelSpec(D, [RBFSpec(p.gammas[0]), Matern32Spec(p.gammas[1])], p.coreg_vecs,
                        p.coreg_diags, p.noise)
    p.spec.set_input_dim(2)
    p.oracle = olik.LMCOperatorOracle(p.spec, p.dists, p.W, p.WT, p.lens, ktype='sum',
                                      active_dim=p.ad)
    Kd = p.oracle.as_numpy()
    p.Kd = 0.5 * (Kd + Kd.T)
    p.lam_min = float(np.linalg.eigvalsh(p.Kd)[0])
    p.rs = rng.randint(0, 2, (4, p.n)) * 2 - 1
    p.B = np.vstack([p.y] + [r.astype(float) for r in p.rs[:2]])
    p.V = rng.randn(5, p.n)
    p.refV = np.array([p.oracle.matvec(v) for v in p.V])
    return p


def _ski_operator(p):
    from runlmc_amd.kern.stationary import RBF, Matern32
    from runlmc_amd.lmc.functional_kernel import FunctionalKernel
    from runlmc_amd.lmc.grid_kernel import gen_grid_kernel
    fk = FunctionalKernel(D=p.D, lmc_kernels=[RBF(p.gammas[0]), Matern32(p.gammas[1])],
                          lmc_ranks=[1, 2])
    fk.coreg_vecs = p.coreg_vecs
    fk.coreg_diags = p.coreg_diags
    fk.noise = p.noise
    fk.set_input_dim(2)
    K, gks = gen_grid_kernel(fk, {p.ad: p.dists}, {p.ad: (p.W, p.WT)}, p.lens)
    return fk, K, gks[p.ad]


def check_ski_2d_operator(case):
    """W against the oracle's bicubic rows, the embedding the case is there for, K~ products of
    1, 2 and 5 vectors, and the solver's unfused rounds.

    RUNLMC_STAGED_WT, RUNLMC_NO_FUSE_W and RUNLMC_NO_FUSE_WT are set together, as the issue
    asks.  On a 2-D model the first is INERT: the LDS-staged W^T / W products
    (k_spmv_wt_staged, k_spmv_w_staged) exist only for rows of at most four consecutive
    entries (rl_ski.hip builds W4_base / WT_lo for cubic W alone; ski_wt_int and w_staged_ok
    require them), and a bicubic row has 16.  The other two are read by the solver only.  So
    the product under the knobs runs the launches of the default one -- the comparison pins
    that (equal bits), it is no coverage of a staged kernel -- and what the knobs do change
    is the solve: W^T and W as CSR products of their own instead of the gather fused into
    the column transforms and W inside MINRES's P kernel.  That solve is held to the rules
    of check_ski_2d_solve."""
    p = ski_problem(case)
    start = 0
    Wd = p.W.toarray()
    m = p.shape[0] * p.shape[1]
    e_w = 0.0
    for d, X in enumerate(p.Xs):
        want = ointerp.bicubic_rows(p.axes[0], p.axes[1], X)
        got = Wd[start:start + len(X), d * m:(d + 1) * m]
        e_w = max(e_w, float(np.abs(got - want).max()))
        assert np.count_nonzero(Wd[start:start + len(X)]) == np.count_nonzero(got)
        start += len(X)
    assert e_w < 1e-13, e_w
    fk, K, gk = _ski_operator(p)
    gop = K.device_operator().grid
    assert (gop.N1, gop.N2) == p.emb, (gop.N1, gop.N2)
    e_k = 0.0
    for k in (1, 2, 5):
        e_k = max(e_k, _vs_oracle(K.matmat(p.V[:k].T).T, p.refV[:k]))
    e_k = max(e_k, _vs_oracle(K.matvec(p.V[0]), p.refV[0]))
    base = K.matmat(p.V.T).T
    knobs = ('RUNLMC_STAGED_WT', 'RUNLMC_NO_FUSE_W', 'RUNLMC_NO_FUSE_WT')
    saved = {k: os.environ.pop(k, None) for k in knobs}
    try:
        for k in knobs:
            os.environ[k] = '1'
        _, K2, _ = _ski_operator(p)
        knobbed = K2.matmat(p.V.T).T
        from runlmc_amd.approx.iterative import Iterative
        xs, _, rs_ = Iterative.solve(K2, p.B, verbose=True, tol=1e-8)
    finally:
        for k in knobs:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    e_st = _vs_oracle(knobbed, base)
    e_so = _vs_oracle(knobbed, p.refV)
    e_sr, e_sx = _solve_rules(p, xs, rs_)
    _say('ski %s operator N %dx%d' % (case, gop.N1, gop.N2), W=e_w, product=e_k,
         product_under_knobs_vs_default=e_st, product_under_knobs_vs_oracle=e_so,
         unfused_solve_residual_rule_used=e_sr, unfused_solve_error_bound_used=e_sx)
    assert e_k < REL, e_k
    assert e_st < 1e-12, e_st
    assert e_so < REL, e_so
    # the staged products do not exist for bicubic rows: the same launches, the same bits (a
    # staged bicubic form, when one arrives, has to revisit this check)
    assert np.array_equal(knobbed, base)


def _solve_rules(p, X, resid):
    """Asserts both rules of check_ski_2d_solve for the solutions X of p.B with reported
    residuals resid; returns the largest used fraction of each bound."""
    worst_r, worst_x = 0.0, 0.0
    for i in range(len(p.B)):
        true = float(np.linalg.norm(p.B[i] - p.oracle.matvec(X[i])))
        xd = np.linalg.solve(p.Kd, p.B[i])
        dx = float(np.linalg.norm(X[i] - xd))
        bound = 1.01 * true / p.lam_min + 1e-12 * float(np.linalg.norm(X[i]))
        worst_r = max(worst_r, abs(true - resid[i]) / (1e-9 + 1e-6 * true))
        worst_x = max(worst_x, dx / bound)
        assert abs(true - resid[i]) <= 1e-9 + 1e-6 * true, (i, true, resid[i])
        assert dx <= bound, (i, dx, bound)
    return worst_r, worst_x


def check_ski_2d_solve(case, minres=True):
    """Iterative.solve at tol 1e-8: every reported residual is ||b - K~ x|| through the oracle
    (the fuzz test's rule) and x is as close to K~^-1 b as that residual allows,
    ||x - K~^-1 b|| <= 1.01 res / lambda_min + 1e-12 ||x||."""
    from runlmc_amd.approx.iterative import Iterative
    p = ski_problem(case)
    fk, K, gk = _ski_operator(p)
    X, iters, resid = Iterative.solve(K, p.B, verbose=True, minres=minres, tol=1e-8)
    worst_r, worst_x = _solve_rules(p, X, resid)
    _say('ski %s %s iterations %s' % (case, 'minres' if minres else 'cg', list(map(int, iters))),
         residual=float(np.max(resid)), residual_rule_used=worst_r, error_bound_used=worst_x,
         lambda_min=p.lam_min)


def check_ski_2d_gradients(case):
    """Gradient assembly with fixed (dense) solves against the reference's loops on the oracle."""
    from parity_suite import _FixedDeriv
    from runlmc_amd.lmc.likelihood import ApproxLMCLikelihood
    import scipy.linalg as la
    p = ski_problem(case)
    fk, K, gk = _ski_operator(p)
    c = la.cho_factor(p.Kd)
    alpha = la.cho_solve(c, p.y)
    inv_rs = la.cho_solve(c, p.rs.T.astype(float)).T
    want = olik.stochastic_gradients(p.spec, p.dists, p.W, p.WT, p.lens, alpha, p.rs, inv_rs,
                                     active_dim=p.ad)
    lik = ApproxLMCLikelihood(fk, K, {p.ad: p.dists}, {p.ad: (p.W, p.WT)}, p.Ys,
                              _FixedDeriv(alpha, p.rs, inv_rs, K.device))
    gv, gd = lik.coreg_vec_gradients(), lik.coreg_diags_gradients()
    gkk, gn = lik.kernel_gradients(), lik.noise_gradient()
    scale = max(max(np.abs(a).max() for a in want['coreg_vec']), 1.0)
    err = float(np.abs(gn - want['noise']).max())
    for q in range(p.Q):
        assert gv[q].shape == want['coreg_vec'][q].shape
        err = max(err, float(np.abs(gv[q] - want['coreg_vec'][q]).max()),
                  float(np.abs(gd[q] - want['coreg_diag'][q]).max()),
                  float(np.abs(np.array(gkk[q]) - np.array(want['kernel'][q])).max()))
    _say('ski %s gradients' % case, error=err / scale)
    assert err < 1e-9 * scale, err / scale


# --- 4. smaller items ----------------------------------------------------------------------
def check_chunked_product_2d():
    """A 2-D batch split into chunks of intermediates on two streams (RUNLMC_CHUNK_MB,
    RUNLMC_TWO_STREAMS): 40 x 130, D = 7, 9 vectors -- 5 chunks of one pair."""
    m1, m2, D, Q, nvec = 40, 130, 7, 2, 9
    rng = np.random.RandomState(23)
    tops = make_tops(m1, m2, Q)
    A, kap = make_coreg(rng, D, Q)
    Bs = ops.coreg_mats(A, kap)
    X = rng.randn(nvec, D * m1 * m2)
    knobs = ('RUNLMC_CHUNK_MB', 'RUNLMC_TWO_STREAMS')
    saved = {k: os.environ.pop(k, None) for k in knobs}
    try:
        g = _new_grid(m1, m2, D, Q)
        g.set_lmc(tops, A, kap)
        whole, e_or, e_dir, ref = product_errors(g, tops, (m1, m2), Bs, X)
        os.environ['RUNLMC_CHUNK_MB'] = '1'
        os.environ['RUNLMC_TWO_STREAMS'] = '1'
        g2 = _new_grid(m1, m2, D, Q)
        # chunk_pairs = max(1, 1 MiB / (D L 16 B)) (gridop_create_impl): a pair's intermediates
        # alone exceed the chunk, so the 5 pairs are 5 chunks
        assert D * g2.L * 16 > (1 << 20) and (nvec + 1) // 2 > 1, g2.L
        g2.set_lmc(tops, A, kap)
        e_ch = e_co = 0.0
        for _ in range(2):                       # the second call reuses both workspaces
            got = g2.matmat_host(X)
            e_ch = max(e_ch, _vs_oracle(got, whole))
            e_co = max(e_co, _vs_oracle(got, ref))
    finally:
        for k in knobs:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    _say('chunked 40x130 D=7', oracle=e_or, direct=e_dir, chunked_vs_whole=e_ch,
         chunked_vs_oracle=e_co)
    assert e_or < REL and e_dir < REL
    assert e_ch < 1e-12, e_ch
    assert e_co < REL, e_co


def check_nd_reduction():
    """BTTB of three and four dimensions over inner grids that take the fused kernels."""
    from runlmc_amd.linalg.bttb import BTTB
    rng = np.random.RandomState(13)
    for sizes in ((3, 20, 40), (2, 2, 33, 70)):
        n = int(np.prod(sizes))
        idx = np.indices(sizes).reshape(len(sizes), -1).astype(float)
        w = np.array([1.0, 0.8, 0.6, 0.45][:len(sizes)])[::-1]
        top = np.exp(-0.07 * np.sqrt(((idx * w[:, None]) ** 2).sum(axis=0))) * \
            (1 + 0.1 * idx[-1] / sizes[-1])
        M = BTTB(top, np.array(sizes))
        O = ops.BTTBOracle(top, sizes)
        x = rng.randn(n)
        X = rng.randn(n, 3)
        e_v = _vs_oracle(M.matvec(x), O.matvec(x))
        e_m = _vs_oracle(M.matmat(X).T, O.matmat(X).T)
        _say('n-d reduction %s' % (sizes,), matvec=e_v, matmat=e_m)
        assert e_v < REL and e_m < REL, (e_v, e_m)


def _pow2_axis(s):
    return max(4, ops.next_pow2(2 * s))


def random_2d_draws(draws=30, seed=2024):
    """Seeded random 2-D shapes (m1, m2, D, Q, nvec): m1, m2 log-uniform on 1...1100 (the
    larger halved while D N1 N2 > 2^22), D from 1...16, 17 and 20, Q from 1...3."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(draws):
        m1, m2 = (int(round(np.exp(rng.uniform(0, np.log(1100))))) for _ in range(2))
        D = int(rng.choice(list(range(1, 17)) + [17, 20]))
        Q = int(rng.randint(1, 4))
        nvec = int(rng.choice([1, 2, 3, 5, 9]))
        while D * _pow2_axis(m1) * _pow2_axis(m2) > (1 << 22):
            if m1 >= m2:
                m1 = max(1, m1 // 2)
            else:
                m2 = max(1, m2 // 2)
        out.append((m1, m2, D, Q, nvec))
    return out


RANDOM_DRAWS = random_2d_draws()


def check_random_coverage():
    """The draws reach at least 8 distinct (N1, N2) (check_random_2d_shape holds every handle
    to these lengths)."""
    seen = {(_pow2_axis(m1), _pow2_axis(m2)) for m1, m2, _, _, _ in RANDOM_DRAWS}
    assert len(RANDOM_DRAWS) == 30 and len(seen) >= 8, sorted(seen)


def check_random_2d_shape(it):
    """Draw `it`: not refused, the embedding the rule gives, first, middle and last vector
    against both references."""
    m1, m2, D, Q, nvec = RANDOM_DRAWS[it]
    rng = np.random.RandomState(5000 + it)
    tops = make_tops(m1, m2, Q)
    A, kap = make_coreg(rng, D, Q)
    Bs = ops.coreg_mats(A, kap)
    try:
        g = _new_grid(m1, m2, D, Q)
    except NotImplementedError as e:
        raise AssertionError('draw %d (%d x %d, D = %d) refused: %s' % (it, m1, m2, D, e))
    assert (g.N1, g.N2) == (_pow2_axis(m1), _pow2_axis(m2))
    g.set_lmc(tops, A, kap)
    X = rng.randn(nvec, D * m1 * m2)
    _, e_or, e_dir, _ = product_errors(g, tops, (m1, m2), Bs, X, seed=it,
                                       vectors=(0, nvec // 2, nvec - 1))
    _say('random draw %d: %s N %dx%d' % (it, lattice_id(RANDOM_DRAWS[it]), g.N1, g.N2),
         oracle=e_or, direct=e_dir)
    assert e_or < REL and e_dir < REL, (e_or, e_dir)
