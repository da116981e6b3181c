"""Three-dimensional grids: the tricubic interpolant, the 3-D grid product (csrc/rl_lead.h:
k_lead_fwd -> one 2-D product per leading frequency -> k_lead_inv), its refusals, the SKI
operator, solves, gradients and the model on a 9 x 10 x 11 grid.

Shared by the GPU run (tests/test_grid3d_gpu.py, librunlmc_hip.so on an MI355X) and the CPU run
(tests/test_grid3d_emu.py, the same kernel source under the thread-level emulator).  Every
function uses whichever native library is active.

References.  Every grid product is held to two independent ones, as in grid2d_suite:
  1. the oracle: ops.grid_sum_matvec over ops.BTTBOracle(top, (m0, m1, m2)) (NumPy rfftn), every
     vector, every entry;
  2. the plain triple sum in np.longdouble,
         y[a, i] = sum_b B[a,b] sum_j top[|i0-j0|, |i1-j1|, |i2-j2|] x[b, j],
     at the eight corners, the centre and 24 seeded random points of every output block.
The two must agree below 1e-14.  The bar is the transform kernels' stated one, REL = 1e-11 of
max|y| per vector.  The tops are anisotropic in all three axes and differ per q, so swapped or
mirrored axes change the answer; A_q has ranks 1, 2, 0 across q.

Dense matrices of the model checks are assembled entry by entry from the closed forms of
separable_suite._Sep; W is np.kron of the three oracle.interp.cubic_rows rows of each sample.

Each check prints the worst error it measured (pytest -s shows them; profiles/grid3d/README.md
holds those of the GPU run).
"""
import functools
import os
import types

import numpy as np
import scipy.linalg as la

from oracle import operators as ops
from oracle import interp as ointerp
from oracle.kernels import RBFSpec, Matern32Spec, StdPeriodicSpec

import grid2d_suite as g2
import loo_suite
from separable_suite import _Sep, _raises, _dense_cross

from runlmc_amd.kern import RBF, Matern32, StdPeriodic, Separable
from runlmc_amd.lmc.functional_kernel import FunctionalKernel

REL = g2.REL

# m0, m1, m2, D, Q, nvec, N0 -- what each row reaches is in the comment
LATTICE = [
    (1, 1, 1, 1, 1, 3, 4),          # the floor N0 = 4 on a single point
    (1, 5, 7, 2, 1, 3, 4),          # ... on a single leading slab
    (2, 5, 7, 2, 2, 3, 4),          # N0 = 4, one complex frequency
    (3, 4, 6, 3, 2, 1, 8),          # a single vector (odd pair in the children)
    (4, 5, 7, 2, 2, 3, 8),          # N0 = 2 m0, no gap
    (5, 7, 5, 2, 3, 5, 16),         # largest gap, all three ranks
    (16, 5, 7, 1, 1, 2, 32),        # N0 = 32
    (17, 6, 5, 2, 2, 3, 64),        # N0 = 64
    (64, 4, 5, 1, 1, 2, 128),       # the limit N0 = 128
    (5, 33, 20, 3, 2, 17, 16),      # 34 child vectors
    (5, 6, 7, 17, 2, 3, 16),        # wide children
    (3, 2, 600, 1, 1, 2, 8),        # the children's generic row plan
    (6, 40, 70, 2, 2, 3, 16),       # third-generation rows
]


def lattice_id(row):
    return '%dx%dx%d-D%d-Q%d-v%d' % row[:6]


def _say(name, **errs):
    print('grid3d %s: %s' % (name, '  '.join('%s %.2e' % kv for kv in errs.items())), flush=True)


def make_tops(m0, m1, m2, Q):
    """grid2d_suite.make_tops with a third factor: exp(-a_q sqrt((1.3 i0)^2 + i1^2 + (0.7 i2)^2))
    (1 + 0.1 i2 / m2) (1 - 0.07 i0 / m0), different per q and per axis."""
    i0, i1, i2 = np.meshgrid(*[np.arange(s, dtype=float) for s in (m0, m1, m2)], indexing='ij')
    r = np.sqrt((1.3 * i0) ** 2 + i1 ** 2 + (0.7 * i2) ** 2)
    return np.array([(np.exp(-(0.05 + 0.11 * q) * r) * (1 + 0.1 * i2 / m2) * (1 - 0.07 * i0 / m0)).ravel()
                     for q in range(Q)])


def sample_points(rng, sizes, D):
    """Per output block: the eight corners, the centre, 24 random points."""
    m0, m1, m2 = sizes
    fixed = [(a, b, c) for a in (0, m0 - 1) for b in (0, m1 - 1) for c in (0, m2 - 1)]
    fixed.append((m0 // 2, m1 // 2, m2 // 2))
    out = []
    for _ in range(D):
        rnd = list(zip(rng.randint(0, m0, 24), rng.randint(0, m1, 24), rng.randint(0, m2, 24)))
        out.append(np.array(fixed + rnd, dtype=np.int64))
    return out


def direct_samples(tops, sizes, Bs, X, points):
    """The triple sum in np.longdouble at points[a] of output block a, for every vector: list
    over a of (nvec, npts) arrays."""
    m0, m1, m2 = sizes
    m = m0 * m1 * m2
    D = len(points)
    Xl = np.asarray(X, dtype=np.longdouble).reshape(-1, D, m)
    j0, j1, j2 = np.arange(m0), np.arange(m1), np.arange(m2)
    out = []
    for a in range(D):
        p = points[a]
        l0 = np.abs(p[:, 0, None] - j0[None, :])
        l1 = np.abs(p[:, 1, None] - j1[None, :])
        l2 = np.abs(p[:, 2, None] - j2[None, :])
        val = np.zeros((Xl.shape[0], len(p)), dtype=np.longdouble)
        for q, top in enumerate(tops):
            t = np.asarray(top, dtype=np.longdouble).reshape(sizes)
            T = t[l0[:, :, None, None], l1[:, None, :, None], l2[:, None, None, :]].reshape(len(p), m)
            xm = np.tensordot(np.asarray(Bs[q][a], dtype=np.longdouble), Xl, axes=(0, 1))
            val += xm.dot(T.T)
        out.append(val)
    return out


def _vs_direct(got, ref, sizes, direct, points):
    m = sizes[0] * sizes[1] * sizes[2]
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    scale = np.maximum(np.abs(ref).max(axis=1), 1e-300)
    worst = 0.0
    for a, (p, val) in enumerate(zip(points, direct)):
        idx = a * m + (p[:, 0] * sizes[1] + p[:, 1]) * sizes[2] + p[:, 2]
        err = np.abs(got[:, idx].astype(np.longdouble) - val).max(axis=1) / scale
        worst = max(worst, float(err.max()))
    return worst


def product_errors(g, tops, sizes, Bs, X, seed=0, top=None):
    """(Y, error vs the oracle, error vs the direct sum) of g's product of X (of top row `top`
    alone, B = I, when given)."""
    Y = g.matmat_host(X, top=top)
    if top is not None:
        tops, Bs = [tops[top]], [np.identity(g.D)]
    toeps = [ops.BTTBOracle(t, sizes) for t in tops]
    ref = np.array([ops.grid_sum_matvec(Bs, toeps, x) for x in X])
    points = sample_points(np.random.RandomState(1000 + seed), sizes, g.D)
    direct = direct_samples(tops, sizes, Bs, X, points)
    e_refs = _vs_direct(ref, ref, sizes, direct, points)
    assert e_refs < 1e-14, e_refs
    return Y, g2._vs_oracle(Y, ref), _vs_direct(Y, ref, sizes, direct, points)


def _new_grid(m0, m1, m2, D, Q):
    from runlmc_amd._native import GridOp
    return GridOp(D, m0 * m1 * m2, Q, sizes=(m0, m1, m2))


def _lattice_setup(row):
    m0, m1, m2, D, Q, nvec, N0 = row
    rng = np.random.RandomState(7 + m0 * 131 + m1 * 17 + m2 + D)
    tops = make_tops(m0, m1, m2, Q)
    A, kap = g2.make_coreg(rng, D, Q)
    Bs = ops.coreg_mats(A, kap)
    X = rng.randn(nvec, D * m0 * m1 * m2)
    return rng, tops, A, kap, Bs, X


def check_plan_lattice3(row):
    """One row of LATTICE: the reported embedding, the product against both references."""
    m0, m1, m2, D, Q, nvec, N0 = row
    _, tops, A, kap, Bs, X = _lattice_setup(row)
    g = _new_grid(m0, m1, m2, D, Q)
    assert (g.m0, g.N0, g.F) == (m0, N0, N0 // 2 + 1), (g.m0, g.N0, g.F)
    n1 = max(4, ops.next_pow2(2 * m1))
    n2 = max(4, ops.next_pow2(2 * m2))
    assert (g.N1, g.N2, g.L) == (n1, n2, n1 * n2), (g.N1, g.N2, g.L)
    g.set_lmc(tops, A, kap)
    assert g.form()[0] == 0 and g.top_forms() == ([0] * Q, False)
    _, e_or, e_dir = product_errors(g, tops, (m0, m1, m2), Bs, X)
    _say('lattice %s' % lattice_id(row), oracle=e_or, direct=e_dir, bar=REL)
    assert e_or < REL and e_dir < REL, (e_or, e_dir)


def check_top_products(row):
    """rl_gridop_mvm_top(q) against the single-top oracle."""
    m0, m1, m2, D, Q, nvec, N0 = row
    _, tops, A, kap, Bs, X = _lattice_setup(row)
    g = _new_grid(m0, m1, m2, D, Q)
    g.set_lmc(tops, A, kap)
    for q in range(Q):
        _, e_or, e_dir = product_errors(g, tops, (m0, m1, m2), Bs, X, seed=q, top=q)
        _say('top %d of %s' % (q, lattice_id(row)), oracle=e_or, direct=e_dir, bar=REL)
        assert e_or < REL and e_dir < REL, (q, e_or, e_dir)


def check_unit_columns3():
    """K e_j for e_j at three grid points of one output equals the dense column -- top indexed at
    the per-axis lags -- to 1e-13 of its maximum (grid2d_suite.check_unit_columns on (3, 4, 6))."""
    sizes, D, Q = (3, 4, 6), 3, 2
    m = int(np.prod(sizes))
    rng = np.random.RandomState(5)
    tops = make_tops(*sizes, Q)
    A, kap = g2.make_coreg(rng, D, Q)
    Bs = ops.coreg_mats(A, kap)
    g = _new_grid(*sizes, D, Q)
    g.set_lmc(tops, A, kap)
    b0 = D // 2
    I = np.meshgrid(*[np.arange(s) for s in sizes], indexing='ij')
    pts = [(0, 0, 0), (2, 3, 5), (0, 3, 0), (2, 0, 5), (1, 2, 3)]
    E = np.zeros((len(pts), D * m))
    want = np.zeros_like(E)
    for k, j in enumerate(pts):
        E[k, b0 * m + (j[0] * sizes[1] + j[1]) * sizes[2] + j[2]] = 1.0
        lag = [np.reshape(t, sizes)[np.abs(I[0] - j[0]), np.abs(I[1] - j[1]), np.abs(I[2] - j[2])].ravel()
               for t in tops]
        for a in range(D):
            want[k, a * m:(a + 1) * m] = sum(B[a, b0] * l for B, l in zip(Bs, lag))
    got = g.matmat_host(E)
    err = float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max())
    _say('unit columns 3x4x6', err=err, bar=1e-13)
    assert err < 1e-13, err


def check_update_bits():
    """A parameter update on a live handle gives the bits of a fresh handle at those parameters
    (set_lmc and set_dense)."""
    row = (5, 7, 5, 2, 3, 5, 16)
    m0, m1, m2, D, Q, nvec, _ = row
    rng, tops, A, kap, Bs, X = _lattice_setup(row)
    tops2 = make_tops(m0, m1, m2, Q)[::-1] * 1.3
    A2, kap2 = g2.make_coreg(rng, D, Q)
    g = _new_grid(m0, m1, m2, D, Q)
    g.set_lmc(tops, A, kap)
    g.matmat_host(X)
    g.set_lmc(tops2, A2, kap2)
    walked = g.matmat_host(X)
    fresh = _new_grid(m0, m1, m2, D, Q)
    fresh.set_lmc(tops2, A2, kap2)
    np.testing.assert_array_equal(walked, fresh.matmat_host(X))
    # dense couplings: the same operator to the bar (another factorisation of B)
    g.set_dense(tops2, np.array(ops.coreg_mats(A2, kap2)))
    err = g2._vs_oracle(g.matmat_host(X), walked)
    _say('update: set_dense against set_lmc', err=err, bar=REL)
    assert err < REL, err
    # fewer top rows than the handle holds
    g.set_lmc(tops[:1], A[:1], kap[:1])
    _, e_or, e_dir = product_errors(g, tops[:1], (m0, m1, m2), Bs[:1], X)
    assert e_or < REL and e_dir < REL, (e_or, e_dir)


def check_refusals():
    """What a 3-D grid refuses, from host checks, and that the process stays usable."""
    import ctypes
    from runlmc_amd import _lib
    from runlmc_amd._native import GridOp, SkiOp, Sampler
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    _raises(NotImplementedError, lambda: GridOp(1, 65 * 4 * 4, 1, sizes=(65, 4, 4)), 'leading')
    _raises(NotImplementedError, lambda: GridOp(1, 2 * 2 * 2049, 1, sizes=(2, 2, 2049)), 'LDS')
    _raises(ValueError, lambda: GridOp(1, 61, 1, sizes=(3, 4, 5)), 'multiply')
    _raises(NotImplementedError, lambda: GridOp(1, 16, 1, sizes=(2, 2, 2, 2)))
    lib = _lib.get_library()
    h = ctypes.c_void_p()
    _raises(ValueError, lambda: lib.call('rl_gridop_create_3d', 0, 1, 0, 4, 4, 1, ctypes.byref(h)), 'm0')
    assert not h.value
    sizes, D = (3, 4, 5), 2
    m = int(np.prod(sizes))
    g = _new_grid(*sizes, D, 1)
    _raises(ValueError, lambda: g.matmat_host(np.zeros(D * m)), 'no parameters')
    g.set_lmc(make_tops(*sizes, 1), [None], [np.ones(D)])
    _raises(NotImplementedError, lambda: Sampler(g), '3-D')
    _raises(NotImplementedError, lambda: g.spectrum(0), '3-D')
    _raises(NotImplementedError, lambda: g.project(g.mvm(_dev(g, np.zeros((1, D * m)))), 24))
    assert g.poly_coeffs(0) == (0, None) and g.form_stats(0) == (0.0, 0.0, 0.0, 0.0)
    # the operator's factorisation
    rng = np.random.RandomState(2)
    axes = [np.linspace(-0.5, 1.5, s + 4) for s in sizes]
    from runlmc_amd.approx.interpolation import multi_interpolant
    Xs = [rng.rand(9, 3) for _ in range(D)]
    sizes7 = tuple(len(a) for a in axes)
    g7 = _new_grid(*sizes7, D, 1)
    g7.set_lmc(make_tops(*sizes7, 1), [None], [np.ones(D)])
    W = multi_interpolant(Xs, *axes)
    s = SkiOp(g7, W, W.T.tocsr())
    s.set_noise(np.full(D, 0.1), [9] * D)
    available, _, _ = s.factor()
    assert not available and '3-D' in s.factor_reason, s.factor_reason
    # the model without grid sizes
    fk = FunctionalKernel(D=D, lmc_kernels=[RBF.ard([1, 2, 3], [0, 1, 2])], lmc_ranks=[1])
    _raises(NotImplementedError,
            lambda: InterpolatedLLGP(Xs, [x[:, 0] for x in Xs], functional_kernel=fk),
            'ExactLMCLikelihood', 'm=[m0, m1, m2]')
    # the process stays usable
    check_plan_lattice3(LATTICE[2])


def _dev(g, X):
    import torch
    return torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(g.device)


# --- interpolant -------------------------------------------------------------------------------
def tricubic_rows(axes, samples):
    """Dense n x (m0 m1 m2) matrix: np.kron of the three cubic rows of each sample."""
    R = [ointerp.cubic_rows(a, samples[:, i]) for i, a in enumerate(axes)]
    return np.array([np.kron(np.kron(R[0][k], R[1][k]), R[2][k]) for k in range(len(samples))])


def check_tricubic():
    from runlmc_amd.approx.interpolation import interp_tricubic, interp_bicubic, multi_interpolant
    rng = np.random.RandomState(11)
    axes = [np.linspace(0.0, 1.0, 9), np.linspace(-1.0, 2.0, 7), np.linspace(3.0, 4.0, 12)]
    lo, step = np.array([a[0] for a in axes]), np.array([a[1] - a[0] for a in axes])
    span = np.array([a[-1] - a[0] for a in axes])
    interior = lo + 2 * step + rng.rand(20, 3) * (span - 4 * step)
    first = lo + rng.rand(6, 3) * step * 0.98 + 0.01 * step
    last = lo + span - rng.rand(6, 3) * step * 0.98 - 0.01 * step
    mixed = np.where(rng.rand(8, 3) < 0.5, first[:6][rng.randint(0, 6, 8)], interior[:8])
    samples = np.vstack([interior, first, last, mixed])
    W = interp_tricubic(*axes, samples)
    want = tricubic_rows(axes, samples)
    err = float(np.abs(W.toarray() - want).max())
    nnz = np.diff(W.indptr)
    sums = np.abs(np.asarray(W.sum(axis=1)).ravel() - 1).max()
    assert np.all(nnz[:20] == 64) and np.all(nnz <= 64) and np.all(nnz[20:32] < 64), nnz
    # a trilinear function on the grid is reproduced at the samples
    G = np.meshgrid(*axes, indexing='ij')
    f = lambda x, y, z: 1 + 2 * x - y + 0.5 * z + x * y - 0.3 * y * z + 0.2 * x * z + 0.7 * x * y * z
    # (where no tap is clamped: a clamped tap stands for a grid value beyond the end)
    e_lin = float(np.abs(W.dot(f(*G).ravel()) - f(*samples.T))[:20].max())
    _say('tricubic', kron=err, rowsum=sums, trilinear=e_lin)
    assert err < 1e-13 and sums < 1e-13 and e_lin < 1e-12, (err, sums, e_lin)
    # argument errors as interp_bicubic's
    assert interp_tricubic(*axes, np.zeros((0, 3))).shape == (0, 9 * 7 * 12)
    _raises(ValueError, lambda: interp_tricubic(axes[0][:3], axes[1], axes[2], samples), 'must be >=4')
    _raises(ValueError, lambda: interp_bicubic(axes[0][:3], axes[1], samples[:, :2]), 'must be >=4')
    _raises(ValueError, lambda: interp_tricubic(axes[0], axes[1][None, :], axes[2], samples), 'should be 1')
    _raises(ValueError, lambda: interp_tricubic(*axes, samples[:, :2]), 'expecting 3d samples')
    # the block-diagonal interpolant dispatches on three columns
    M = multi_interpolant([samples[:5], samples[5:9]], *axes)
    m = 9 * 7 * 12
    assert M.shape == (9, 2 * m) and M.indices.dtype == np.int32
    np.testing.assert_allclose(M.toarray()[5:, m:], want[5:9], rtol=0, atol=1e-13)
    _raises(NotImplementedError, lambda: multi_interpolant([np.zeros((2, 4))], *axes, axes[0]))


# --- model --------------------------------------------------------------------------------------
GAM = (1.7, 2.3, 1.1)
M32, PER, PLEN, RB = 1.4, 1.5, 0.6, 2.0
# The model problem: the full one (9 x 10 x 11 grid, N0 = 32, 17 leading frequencies) runs on the
# device; the emulator walks every thread of every child's transforms, so its runner takes the
# same checks on a 5 x 6 x 7 grid (N0 = 16, 9 leading frequencies) -- use_problem('small').
PROBLEMS = {'full': dict(lens=[70, 66], m=[5, 6, 7], shape=(9, 10, 11), N0=32),
            'small': dict(lens=[30, 26], m=[1, 2, 3], shape=(5, 6, 7), N0=16)}
PROBLEM = 'full'


def use_problem(name):
    global PROBLEM
    assert name in PROBLEMS
    PROBLEM = name


def _bttb3(top):
    """Dense three-level block-Toeplitz matrix of a top row laid out (m0, m1, m2)."""
    s = top.shape
    d = [np.abs(np.subtract.outer(np.arange(k), np.arange(k))) for k in s]
    T = top[d[0][:, None, None, :, None, None], d[1][None, :, None, None, :, None],
            d[2][None, None, :, None, None, :]]
    m = s[0] * s[1] * s[2]
    return T.reshape(m, m)


class _Case:
    pass


KERNEL_SETS = {
    'iso': (lambda: [RBF(RB, active_dims=[0, 1, 2])],
            lambda: [_Sep([(RBFSpec(RB), [0, 1, 2])])]),
    'mix': (lambda: [Separable(RBF(GAM[0], active_dims=[0]), Matern32(M32, active_dims=[1]),
                               StdPeriodic(PER, PLEN, active_dims=[2])),
                     RBF(RB, active_dims=[0, 1, 2])],
            lambda: [_Sep([(RBFSpec(GAM[0]), [0]), (Matern32Spec(M32), [1]),
                           (StdPeriodicSpec(PER, PLEN), [2])]),
                     _Sep([(RBFSpec(RB), [0, 1, 2])])]),
    'ard': (lambda: [RBF.ard(GAM, [0, 1, 2])],
            lambda: [_Sep([(RBFSpec(g), [i]) for i, g in enumerate(GAM)])]),
}


def _case(kind='mix'):
    return _case_of(kind, PROBLEM)


@functools.lru_cache(maxsize=None)
def _case_of(kind, problem):
    """The seeded three-input problem and its dense references (computed once, left unchanged)."""
    from runlmc_amd.approx.interpolation import autogrid
    rng = np.random.RandomState(303)
    c = _Case()
    c.kind = kind
    c.spec = PROBLEMS[problem]
    c.D, c.lens = 2, list(c.spec['lens'])
    c.n = sum(c.lens)
    c.Xs = [rng.rand(l, 3) for l in c.lens]
    c.Ys = [np.sin(4 * X[:, 0] + d) * np.cos(5 * X[:, 1]) + 0.5 * X[:, 2] + 0.1 * rng.randn(len(X))
            for d, X in enumerate(c.Xs)]
    c.y = np.hstack(c.Ys)
    c.refs = KERNEL_SETS[kind][1]()
    Q = len(c.refs)
    c.A = [rng.uniform(-1, 1, size=(1, c.D)) for _ in range(Q)]
    c.kappa = [0.2 + rng.rand(c.D) for _ in range(Q)]
    c.noise = 0.05 + 0.1 * rng.rand(c.D)
    c.Bs = [a.T @ a + np.diag(k) for a, k in zip(c.A, c.kappa)]
    c.axes = autogrid(c.Xs, None, None, np.array(c.spec['m']))
    c.shape = tuple(len(a) for a in c.axes)
    assert c.shape == c.spec['shape']
    m = int(np.prod(c.shape))
    W = np.zeros((c.n, c.D * m))
    start = 0
    for d, X in enumerate(c.Xs):
        W[start:start + len(X), d * m:(d + 1) * m] = tricubic_rows(c.axes, X)
        start += len(X)
    c.W = W
    c.mesh = np.meshgrid(*[a - a[0] for a in c.axes], indexing='ij')
    c.Kd = _ski_dense(c, c.refs)
    c.Xt = [rng.rand(5 + d, 3) * 0.9 + 0.05 for d in range(c.D)]
    c.rs = rng.randint(0, 2, (4, c.n)) * 2 - 1
    return c


def _grid_tops(c, refs, grads=False):
    if grads:
        return [[_bttb3(g) for g in r.grads(c.mesh)] for r in refs]
    return [_bttb3(r.value(c.mesh)) for r in refs]


def _ski_dense(c, refs, Bs=None, noise=None):
    """W (sum_q B_q (x) T_q) W^T + diag eps."""
    Bs = c.Bs if Bs is None else Bs
    noise = c.noise if noise is None else noise
    Kuu = sum(np.kron(B, T) for B, T in zip(Bs, _grid_tops(c, refs)))
    K = c.W @ Kuu @ c.W.T + np.diag(np.repeat(noise, c.lens))
    return 0.5 * (K + K.T)


def _model(kind='mix', prediction='on-the-fly', metrics=False, variance_batch=None, tolerance=1e-4):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    c = _case(kind)
    kerns = KERNEL_SETS[kind][0]()
    fk = FunctionalKernel(D=c.D, lmc_kernels=kerns, lmc_ranks=[1] * len(kerns))
    fk.coreg_vecs, fk.coreg_diags, fk.noise = c.A, c.kappa, c.noise
    np.random.seed(5)
    return InterpolatedLLGP(c.Xs, c.Ys, normalize=False, m=c.spec['m'], functional_kernel=fk,
                            prediction=prediction, metrics=metrics, trace_iterations=4,
                            tolerance=tolerance, variance_batch=variance_batch)


def check_ski_operator(kind):
    """K~ of the model's operator against the dense W (sum B (x) T) W^T + diag eps: the identity
    and batches of 1, 2 and 5 vectors at 1e-11; equal bits with RUNLMC_STAGED_WT set (a tricubic
    row has 64 entries: no staged kernel takes it)."""
    c = _case(kind)
    model = _model(kind)
    model._ensure()
    (ad,) = model.dists
    assert ad == (0, 1, 2) and model.dists[ad].shape == c.shape and len(model.lags[ad].lags) == 3
    gk = model._grid_kernels[ad]
    assert gk._op.sizes == c.shape and (gk._op.m0, gk._op.N0) == (c.shape[0], c.spec['N0'])
    Wm = model.interpolants[ad][0]
    e_w = float(np.abs(Wm.toarray() - c.W).max())
    got = model._K.matmat(np.identity(c.n))
    scale = np.abs(c.Kd).max()
    err = float(np.abs(got - c.Kd).max() / scale)
    rng = np.random.RandomState(9)
    e_b = 0.0
    for k in (1, 2, 5):
        V = rng.randn(c.n, k)
        ref = c.Kd @ V
        e_b = max(e_b, g2._vs_oracle(model._K.matmat(V).T, ref.T))
    V = rng.randn(c.n, 5)
    base = model._K.matmat(V)
    knobs = ('RUNLMC_STAGED_WT',)
    saved = {k: os.environ.pop(k, None) for k in knobs}
    try:
        for k in knobs:
            os.environ[k] = '1'
        other = _model(kind)
        other._ensure()
        knobbed = other._K.matmat(V)
    finally:
        for k in knobs:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    _say('ski operator (%s)' % kind, W=e_w, identity=err, batches=e_b, bar=1e-11)
    assert e_w < 1e-13 and err <= 1e-11 and e_b <= 1e-11, (e_w, err, e_b)
    np.testing.assert_array_equal(knobbed, base)


def check_ski_solve(kind='mix'):
    """Iterative.solve at tol = 1e-8, MINRES and CG, under both rules of grid2d_suite._solve_rules:
    the reported residual is the true one, the error is bounded by it over lambda_min."""
    from runlmc_amd.approx.iterative import Iterative
    c = _case(kind)
    model = _model(kind)
    model._ensure()
    K = model._K
    p = types.SimpleNamespace(
        B=np.vstack([c.y, c.rs[:2].astype(float)]), Kd=c.Kd,
        oracle=types.SimpleNamespace(matvec=lambda v: c.Kd @ v),
        lam_min=float(np.linalg.eigvalsh(c.Kd)[0]))
    for minres in (True, False):
        X, _, resid = Iterative.solve(K, p.B, verbose=True, tol=1e-8, minres=minres)
        wr, wx = g2._solve_rules(p, np.atleast_2d(X), np.atleast_1d(resid))
        _say('ski solve (%s, %s)' % (kind, 'minres' if minres else 'cg'), residual_rule=wr, error_rule=wx)


def check_model_params():
    c = _case()
    model = _model()
    x = model.param_array.copy()
    want = sum(a.size for a in c.A) + 2 * c.D + (1 + 1 + 2 + 1) + c.D
    assert x.shape == (want,), (x.shape, want)
    (ad,) = model.dists
    for i in range(3):
        idx = [0, 0, 0]
        idx[i] = slice(None)
        np.testing.assert_array_equal(model.lags[ad].lags[i][tuple(idx)], c.axes[i] - c.axes[i][0])
    rng = np.random.RandomState(3)
    x1 = x + 0.05 * rng.randn(len(x))
    model.param_array = x1
    np.testing.assert_allclose(model.param_array, x1, rtol=0, atol=1e-12)
    assert model.gradient.shape == x.shape and np.all(np.isfinite(model.gradient))
    assert np.isfinite(model.log_likelihood())


def check_model_solve():
    """The model's own alpha at tolerance 1e-12 against the dense solve (separable_suite's rule)."""
    c = _case()
    xref = la.solve(c.Kd, c.y, assume_a='pos')
    with loo_suite._tight_krylov():
        model = _model(tolerance=1e-12)
        model._ensure()
        alpha = model.kernel.alpha()
    r = np.linalg.norm(c.y - c.Kd @ alpha)
    e = np.abs(alpha - xref).max()
    _say('model alpha', residual=r, error=e)
    assert r < 1e-8 * np.linalg.norm(c.y), r
    assert e <= r / c.noise.min() + 1e-12 * np.abs(xref).max()
    assert model._K.preconditioner is None


def check_model_gradients(kind='mix'):
    """Gradient assembly with fixed probes and dense solves against the reference's loops, one
    dense dK = W (dB (x) T) W^T per parameter (separable_suite.check_model_gradients), 1e-9 of
    the scale."""
    from parity_suite import _FixedDeriv
    from runlmc_amd.lmc.likelihood import ApproxLMCLikelihood
    c = _case(kind)
    model = _model(kind)
    model._ensure()
    fk, K = model._functional_kernel, model._K
    Q = len(c.refs)
    cf = la.cho_factor(c.Kd)
    alpha = la.cho_solve(cf, c.y)
    inv_rs = la.cho_solve(cf, c.rs.T.astype(float)).T
    lik = ApproxLMCLikelihood(fk, K, model.lags, model.interpolants, c.Ys,
                              _FixedDeriv(alpha, c.rs, inv_rs, K.device))
    m = int(np.prod(c.shape))
    Wd = [c.W[:, d * m:(d + 1) * m] for d in range(c.D)]

    def loop(dB, T):
        WT = [w @ T for w in Wd]
        dK = sum(dB[a, b] * WT[a] @ Wd[b].T for a in range(c.D) for b in range(c.D) if dB[a, b] != 0.0)
        tr = np.mean([s @ dK @ r for s, r in zip(inv_rs, c.rs)])
        return 0.5 * (alpha @ dK @ alpha - tr)
    tops, dtops = _grid_tops(c, c.refs), _grid_tops(c, c.refs, grads=True)
    want = dict(coreg_vec=[], coreg_diag=[], kernel=[])
    eye = np.identity(c.D)
    for q in range(Q):
        gA = np.zeros_like(c.A[q])
        for i in range(gA.shape[0]):
            for j in range(c.D):
                dB = np.outer(eye[j], c.A[q][i])
                gA[i, j] = loop(dB + dB.T, tops[q])
        want['coreg_vec'].append(gA)
        want['coreg_diag'].append(np.array([loop(np.outer(eye[d], eye[d]), tops[q]) for d in range(c.D)]))
        want['kernel'].append([loop(c.Bs[q], dT) for dT in dtops[q]])
    ends = np.cumsum(c.lens)
    begins = ends - np.asarray(c.lens)
    want['noise'] = np.array([0.5 * (alpha[b:e] @ alpha[b:e] - np.mean([s[b:e] @ r[b:e] for s, r in zip(inv_rs, c.rs)]))
                              for b, e in zip(begins, ends)])
    gv, gd = lik.coreg_vec_gradients(), lik.coreg_diags_gradients()
    gkk, gn = lik.kernel_gradients(), lik.noise_gradient()
    assert [len(g) for g in gkk] == [len(w) for w in want['kernel']]
    scale = max(max(np.abs(a).max() for a in want['coreg_vec']), 1.0)
    err = float(np.abs(gn - want['noise']).max())
    for q in range(Q):
        err = max(err, float(np.abs(gv[q] - want['coreg_vec'][q]).max()),
                  float(np.abs(gd[q] - want['coreg_diag'][q]).max()),
                  float(np.abs(np.array(gkk[q]) - np.array(want['kernel'][q])).max()))
    _say('model gradients (%s)' % kind, err=err / scale, bar=1e-9)
    assert err < 1e-9 * scale, err / scale


def _native_variance(c):
    coreg = np.column_stack([np.square(a).sum(axis=0) for a in c.A]) + np.column_stack(c.kappa)
    return np.repeat(coreg @ np.ones(len(c.refs)) + c.noise, [len(v) for v in c.Xt])


def check_model_exact_prediction():
    """prediction='exact' against the dense conditional formula on the kernel itself."""
    c = _case()
    model = _model(prediction='exact')
    _, var = model.predict(c.Xt)
    tl = [len(v) for v in c.Xt]
    X = np.vstack(c.Xs)
    Kx = _dense_cross(c.refs, c.Bs, np.vstack(c.Xt), tl, X, c.lens)
    Kd = _dense_cross(c.refs, c.Bs, X, c.lens, X, c.lens) + np.diag(np.repeat(c.noise, c.lens))
    native = _native_variance(c)
    ref = np.clip(native - np.einsum('ij,ji->i', Kx, la.solve(Kd, Kx.T)), 0, None)
    err = np.abs(np.concatenate(var) - ref).max()
    _say('model exact variances', err=err, atol=1e-8 * native.max())
    np.testing.assert_allclose(np.concatenate(var), ref, rtol=0, atol=1e-8 * native.max())


def check_model_variances(precompute=True):
    """predict's mean against the dense SKI conditional mean; the tiled variances against the
    host-assembled ones at separable_suite's bar; 'on-the-fly' variances within [0, prior] and
    'precompute' ones finite and not negative.  The bounds are deliberately not separable_suite's
    strict ones: see the comments below and DESIGN section 11.  `precompute=False` leaves out the
    'precompute' mode (the emulator's run: one solve per grid point)."""
    c = _case()
    model = _model()
    mu0, var0 = model.predict(c.Xt)
    mu1, var1 = _model(variance_batch=5).predict(c.Xt)
    native = _native_variance(c)
    atol = 1e-5 * max(native.max(), 1.0)
    err = np.abs(np.concatenate(var1) - np.concatenate(var0)).max()
    _say('model tiled against host-assembled variances', err=err, atol=atol)
    np.testing.assert_allclose(np.concatenate(var1), np.concatenate(var0), rtol=0, atol=atol)
    np.testing.assert_array_equal(np.concatenate(mu1), np.concatenate(mu0))
    v0 = np.concatenate(var0)
    # (on this coarse grid the SKI quadratic form overshoots the prior at some test points and the
    # variance is clipped at zero there, in the host-assembled and the tiled path alike)
    assert np.all(np.isfinite(v0)) and np.all(v0 >= 0) and np.all(v0 <= native), (v0, native)
    # ('precompute' interpolates a stochastic estimate of the variance on the grid: finite and
    # not negative is what it promises)
    # (one solve per grid point, 1980 right-hand sides: device work, not the emulator's)
    if precompute:
        v2 = np.concatenate(_model(prediction='precompute').predict(c.Xt)[1])
        assert np.all(np.isfinite(v2)) and np.all(v2 >= 0), v2
    # the mean: W* K_UU W^T alpha on the dense matrices, alpha solved to 1e-12
    m = int(np.prod(c.shape))
    Wt = np.zeros((sum(len(x) for x in c.Xt), c.D * m))
    start = 0
    for d, X in enumerate(c.Xt):
        Wt[start:start + len(X), d * m:(d + 1) * m] = tricubic_rows(c.axes, X)
        start += len(X)
    Kuu = sum(np.kron(B, T) for B, T in zip(c.Bs, _grid_tops(c, c.refs)))
    want = Wt @ Kuu @ c.W.T @ la.solve(c.Kd, c.y, assume_a='pos')
    with loo_suite._tight_krylov():
        mu = _model(tolerance=1e-12).predict(c.Xt)[0]
    e_mu = np.abs(np.concatenate(mu) - want).max() / np.abs(want).max()
    _say('model predictive mean', err=e_mu, bar=1e-8)
    assert e_mu <= 1e-8, e_mu


def check_model_loo():
    """loo_predict(method='solve') on a subset (separable_suite.check_model_loo's bars);
    method='direct' refuses with the 3-D reason."""
    c = _case()
    with loo_suite._tight_krylov():
        model = _model(tolerance=1e-12)
        model._ensure()
        Kinv = la.inv(c.Kd)
        alpha, d = Kinv @ c.y, np.diag(Kinv)
        mean_ref, var_ref = c.y - alpha / d, 1.0 / d
        mean_tol = 1e-8 * np.abs(c.y).max()
        var_tol = loo_suite.DIAG_REL * np.max(1.0 / c.noise) / d ** 2
        ends = np.cumsum(c.lens)[:-1]
        sel = np.concatenate([[0, c.n - 1], ends - 1, ends, [7, 23]])
        means, vars_ = model.loo_predict(indices=sel, method='solve', tol=1e-12)
    assert model.loo_stats['method'] == 'solve' and model.loo_stats['nonpositive'] == 0
    em, ev = np.abs(means - mean_ref[sel]).max(), (np.abs(vars_ - var_ref[sel]) / var_tol[sel]).max()
    _say('model loo', mean=em, mean_tol=mean_tol, variance_over_tol=ev)
    assert em <= mean_tol and ev <= 1.0, (em, mean_tol, ev)
    _raises(NotImplementedError, lambda: model.loo_predict(indices=sel, method='direct'), '3-D')


def check_model_update():
    """A model walked through three parameter updates on its live handles against a model built
    at the last parameters: equal bits of the operator, and the dense operator at 1e-11."""
    c = _case()
    walked = _model()
    x = walked.param_array.copy()
    rng = np.random.RandomState(8)
    for _ in range(3):
        x = x + 0.1 * rng.randn(len(x))
        np.random.seed(5)
        walked.param_array = x
    fresh = _model()
    fk, src = fresh._functional_kernel, walked._functional_kernel
    fk.coreg_vecs, fk.coreg_diags, fk.noise = src.coreg_vecs, src.coreg_diags, src.noise
    for k, s in zip(fk.kernels, src.kernels):
        k.set_params(s.param_array)
    np.random.seed(5)
    fresh._ensure()
    np.testing.assert_allclose(fresh.param_array, x, rtol=0, atol=1e-12)
    V = np.random.RandomState(4).randn(c.n, 3)
    np.testing.assert_array_equal(walked._K.matmat(V), fresh._K.matmat(V))
    sep, rbf = src.kernels
    f0, f1, f2 = sep.factors
    refs = [_Sep([(RBFSpec(f0.inv_lengthscale), [0]), (Matern32Spec(f1.inv_lengthscale), [1]),
                  (StdPeriodicSpec(f2.inv_lengthscale, f2.period), [2])]),
            _Sep([(RBFSpec(rbf.inv_lengthscale), [0, 1, 2])])]
    Kd = _ski_dense(c, refs, src.coreg_mats(), src.noise)
    got = walked._K.matmat(np.identity(c.n))
    err = np.abs(got - Kd).max() / np.abs(Kd).max()
    _say('model update walk', err=err, bar=1e-11)
    assert err <= 1e-11, err


def check_model_optimize():
    """A few AdaDelta steps raise the log-likelihood."""
    model = _model('ard')
    np.random.seed(5)
    l0 = model.log_likelihood()
    x0 = model.param_array.copy()
    model.optimize(max_it=5)
    np.random.seed(5)
    l1 = model.log_likelihood()
    _say('model optimize', before=l0, after=l1)
    assert np.all(np.isfinite(model.param_array)) and np.all(np.isfinite(model.gradient))
    assert not np.array_equal(model.param_array, x0) and l1 > l0, (l0, l1)


def check_model_draws_refuse():
    c = _case()
    model = _model()
    model._ensure()
    _raises(NotImplementedError, lambda: model.posterior_draws(2, seed=1), '3-D')
    _raises(NotImplementedError, lambda: model.prior_draws(2, seed=1), '3-D')
    _raises(NotImplementedError, lambda: model.posterior_samples(c.Xt, size=2, seed=1), '3-D')
    # ... and the model still predicts
    mu, _ = model.predict(c.Xt)
    assert all(np.all(np.isfinite(v)) for v in mu)


def check_two_terms():
    """A kernel over [0, 1, 2] beside one over [0] (rl_ski_add_term): the operator against the
    dense sum of the two SKI terms at 1e-11, and the gradients of both terms with fixed dense
    solves against one dense dK per parameter at 1e-9 of the scale."""
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    c = _case('iso')
    rng = np.random.RandomState(21)
    A = c.A + [rng.uniform(-1, 1, size=(1, c.D))]
    kappa = c.kappa + [0.2 + rng.rand(c.D)]
    fk = FunctionalKernel(D=c.D, lmc_kernels=[RBF(RB, active_dims=[0, 1, 2]), Matern32(M32, active_dims=[0])],
                          lmc_ranks=[1, 1])
    fk.coreg_vecs, fk.coreg_diags, fk.noise = A, kappa, c.noise
    np.random.seed(5)
    model = InterpolatedLLGP(c.Xs, c.Ys, normalize=False, m=c.spec['m'], functional_kernel=fk,
                             trace_iterations=4)
    model._ensure()
    assert set(model.dists) == {(0, 1, 2), (0,)}
    ax = model.grid_axes[(0,)][0]
    m1 = len(ax)
    W1 = np.zeros((c.n, c.D * m1))
    start = 0
    for d, X in enumerate(c.Xs):
        W1[start:start + len(X), d * m1:(d + 1) * m1] = ointerp.cubic_rows(ax, X[:, 0])
        start += len(X)
    B1 = A[1].T @ A[1] + np.diag(kappa[1])
    K1 = W1 @ np.kron(B1, la.toeplitz(Matern32Spec(M32).from_dist(ax - ax[0]))) @ W1.T
    Kd = c.Kd + 0.5 * (K1 + K1.T)
    got = model._K.matmat(np.identity(c.n))
    err = np.abs(got - Kd).max() / np.abs(Kd).max()
    _say('two-term operator', err=err, bar=1e-11)
    assert err <= 1e-11, err
    # gradients with fixed probes and dense solves, one dense dK per parameter of either term
    # (check_model_gradients' loops and bar): a wrong term offset in the gradient path shows here
    from parity_suite import _FixedDeriv
    from runlmc_amd.lmc.likelihood import ApproxLMCLikelihood
    cf = la.cho_factor(Kd)
    alpha = la.cho_solve(cf, c.y)
    inv_rs = la.cho_solve(cf, c.rs.T.astype(float)).T
    lik = ApproxLMCLikelihood(model._functional_kernel, model._K, model.lags, model.interpolants, c.Ys,
                              _FixedDeriv(alpha, c.rs, inv_rs, model._K.device))
    m = int(np.prod(c.shape))
    Ws = [[c.W[:, d * m:(d + 1) * m] for d in range(c.D)], [W1[:, d * m1:(d + 1) * m1] for d in range(c.D)]]
    d1 = ax - ax[0]
    tops = [_grid_tops(c, c.refs)[0], la.toeplitz(Matern32Spec(M32).from_dist(d1))]
    dtops = [_grid_tops(c, c.refs, grads=True)[0],
             [la.toeplitz(g) for g in Matern32Spec(M32).kernel_gradient(d1)]]
    Bs = [c.Bs[0], B1]

    def loop(q, dB, T):
        WT = [w @ T for w in Ws[q]]
        dK = sum(dB[a, b] * WT[a] @ Ws[q][b].T for a in range(c.D) for b in range(c.D) if dB[a, b] != 0.0)
        tr = np.mean([s @ dK @ r for s, r in zip(inv_rs, c.rs)])
        return 0.5 * (alpha @ dK @ alpha - tr)
    eye = np.identity(c.D)
    gv, gd, gkk = lik.coreg_vec_gradients(), lik.coreg_diags_gradients(), lik.kernel_gradients()
    assert [len(g) for g in gkk] == [1, 1]
    gerr, scale = 0.0, 1.0
    for q in range(2):
        want_v = np.array([[loop(q, np.outer(eye[j], A[q][i]) + np.outer(A[q][i], eye[j]), tops[q])
                            for j in range(c.D)] for i in range(A[q].shape[0])])
        want_d = np.array([loop(q, np.outer(eye[d], eye[d]), tops[q]) for d in range(c.D)])
        want_k = np.array([loop(q, Bs[q], dT) for dT in dtops[q]])
        scale = max(scale, float(np.abs(want_v).max()))
        gerr = max(gerr, float(np.abs(gv[q] - want_v).max()), float(np.abs(gd[q] - want_d).max()),
                   float(np.abs(np.array(gkk[q]) - want_k).max()))
    _say('two-term gradients', err=gerr / scale, bar=1e-9)
    assert gerr < 1e-9 * scale, gerr / scale
    assert np.all(np.isfinite(model.gradient)) and np.isfinite(model.log_likelihood())
    mu, var = model.predict(c.Xt)
    assert all(np.all(np.isfinite(v)) for v in mu + var)
