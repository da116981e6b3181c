"""Checks of the function draws (runlmc_amd.approx.pathwise, InterpolatedLLGP.posterior_draws,
include/runlmc_hip.h: rl_sampler_*, rl_normal_fill, rl_pathwise_residual) shared by the CPU run
on the emulator (tests/test_pathwise_emu.py) and the GPU run (tests/test_pathwise_gpu.py).  Every
function uses whichever native library is active.

The reference has no sampler, so every yardstick is dense linear algebra in NumPy, written here:
a sampler is LINEAR in its noise, so feeding it the unit vectors of a pair's noise space gives
the matrices G_a, G_b of draws 2p and 2p + 1, and G G^T is held against the dense K_UU."""
import functools
import logging

import numpy as np
import torch

from runlmc_amd import _lib
from runlmc_amd._native import GridOp, normal_fill
from runlmc_amd.approx import pathwise as pw
from runlmc_amd.approx.pathwise import GridSampler
from runlmc_amd.kern.stationary import RBF, Matern32
from runlmc_amd.lmc.functional_kernel import FunctionalKernel

PRODUCT_TOL = 1e-10        # the project's product tolerance
POLY_TOL = 1e-9            # the polynomial form's acceptance bound 2e-13 m max|T| with a margin


# --- helpers --------------------------------------------------------------------------------------
def _coreg(rng, D, Q, R):
    A = [rng.randn(r, D) if r else None for r in R]
    kap = [np.abs(rng.randn(D)) + 0.1 for _ in range(Q)]
    Bs = [(np.zeros((D, D)) if a is None else a.T @ a) + np.diag(k) for a, k in zip(A, kap)]
    return A, kap, Bs


def _dense_kuu(kernels, Bs, axes):
    pts = np.stack([g.reshape(-1) for g in np.meshgrid(*axes, indexing='ij')], axis=1)
    dist = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    return sum(np.kron(B, k.from_dist(dist)) for B, k in zip(Bs, kernels))


def _grid_op(kernels, A, kap, axes, D):
    sizes = [len(a) for a in axes]
    g = GridOp(D, int(np.prod(sizes)), len(kernels), sizes=sizes if len(sizes) > 1 else None)
    mesh = np.meshgrid(*[a - a[0] for a in axes], indexing='ij')
    d0 = np.sqrt(sum(np.square(x) for x in mesh)).reshape(-1)
    g.set_lmc(np.array([k.from_dist(d0) for k in kernels]), A, kap)
    return g


def _pair_maps(draw, zlen, device, chunk=256):
    """(G_a, G_b): draws 2p and 2p + 1 as matrices over the pair's 2 zlen noise values (row 2p's
    first), from unit vectors fed `chunk` pairs at a time."""
    cols = []
    for half in (0, 1):
        for k0 in range(0, zlen, chunk):
            npair = min(zlen, k0 + chunk) - k0
            Z = torch.zeros((2 * npair, zlen), dtype=torch.float64, device=device)
            Z[2 * torch.arange(npair) + half, torch.arange(k0, k0 + npair)] = 1.0
            cols.append(draw(Z).cpu().numpy())
    U = np.concatenate(cols)
    return U[0::2].T, U[1::2].T


def _check_cov(s, K, tol, what):
    Ga, Gb = _pair_maps(s.draw, s.zlen, s.grid.device)
    sc = np.abs(K).max()
    ea, eb = np.abs(Ga @ Ga.T - K).max(), np.abs(Gb @ Gb.T - K).max()
    ex = np.abs(Ga @ Gb.T).max()
    print('%s: max|Ga Ga^T - K| %.3e, max|Gb Gb^T - K| %.3e, max|Ga Gb^T| %.3e (bound %.3e)'
          % (what, ea, eb, ex, tol * sc))
    assert ea <= tol * sc and eb <= tol * sc, (what, ea, eb, tol * sc)
    assert ex <= tol * sc, (what, ex, tol * sc)
    return Ga, Gb


def _numpy_spectrum(kernel, steps, lengths):
    """The real spectrum of the circulant of the extended, mirrored row (any dimension)."""
    lags = np.meshgrid(*[h * np.minimum(np.arange(n), n - np.arange(n)) for h, n in zip(steps, lengths)],
                       indexing='ij')
    return np.fft.fftn(kernel.from_dist(np.sqrt(sum(np.square(g) for g in lags)))).real


def _numpy_clipped(kernel, steps, lengths):
    lam = _numpy_spectrum(kernel, steps, lengths)
    return -lam[lam < 0].sum() / np.abs(lam).sum()


X12 = np.arange(12) / 7.0
X128 = np.arange(128) / 123.0


# --- 1. embedding map, 1-D, one launch --------------------------------------------------------------
def check_embedding_1d():
    rng = np.random.RandomState(0)
    D, kernels = 2, [RBF(30.0), Matern32(10.0)]
    A, kap, Bs = _coreg(rng, D, 2, (1, 0))
    for k in kernels:
        assert _numpy_clipped(k, [1 / 7.0], [24]) == 0.0
    s = GridSampler(_grid_op(kernels, A, kap, [X12], D), kernels, A, kap, [X12])
    assert [st.form for st in s.stats] == ['embedding'] * 2
    assert [st.Ls for st in s.stats] == [24, 24] and all(st.clipped == 0.0 for st in s.stats), s.stats
    assert s.zlen == (3 + 2) * 24
    _check_cov(s, _dense_kuu(kernels, Bs, [X12]), PRODUCT_TOL, 'embedding m 12')


# --- 2. the ladder ----------------------------------------------------------------------------------
def check_ladder(case):
    rng = np.random.RandomState(2)
    if case == 'A':
        kernel, x, D, first = RBF(10.0), X12, 2, 24
    else:
        kernel, x, D, first = Matern32(3.0), X128, 1, 256
    h = x[1] - x[0]
    assert _numpy_clipped(kernel, [h], [first]) > pw.CLIP_TOL          # the first rung clips
    assert _numpy_clipped(kernel, [h], [2 * first]) <= pw.CLIP_TOL     # the second does not
    A, kap, Bs = _coreg(rng, D, 1, (1 if case == 'A' else 0,))
    s = GridSampler(_grid_op([kernel], A, kap, [x], D), [kernel], A, kap, [x], forms='embedding')
    (st,) = s.stats
    assert st.Ls > first and st.clipped <= pw.CLIP_TOL, st
    _check_cov(s, _dense_kuu([kernel], Bs, [x]), PRODUCT_TOL, 'ladder ' + case)


class _Catch(logging.Handler):
    def __init__(self):
        super().__init__()
        self.records = []

    def emit(self, record):
        self.records.append(record)


def check_ladder_exhausted():
    """Case C: max_embed = 2 on case A keeps Ls = 24, warns, reports what it clipped; the draws'
    covariance is off by at most the largest clipped eigenvalue (the error is B (x) E with E a
    principal submatrix of the circulant whose eigenvalues are the clipped ones; max|B| = 1 here)."""
    rng = np.random.RandomState(2)
    kernel, x, D = RBF(10.0), X12, 2
    A, kap, Bs = _coreg(rng, D, 1, (1,))
    scale = np.abs(Bs[0]).max()             # max|B| = 1: the error B (x) E is then at most max|E|
    A, kap, Bs = [A[0] / np.sqrt(scale)], [kap[0] / scale], [Bs[0] / scale]
    catch = _Catch()
    log = logging.getLogger(pw.__name__)
    log.addHandler(catch)
    try:
        s = GridSampler(_grid_op([kernel], A, kap, [x], D), [kernel], A, kap, [x], max_embed=2)
    finally:
        log.removeHandler(catch)
    assert any(r.levelno >= logging.WARNING and 'clips' in r.getMessage() for r in catch.records)
    (st,) = s.stats
    want = _numpy_clipped(kernel, [x[1] - x[0]], [24])
    assert st.Ls == 24 and want / 2 <= st.clipped <= want * 2, (st, want)
    lam = _numpy_spectrum(kernel, [x[1] - x[0]], [24])
    worst = -lam.min()
    K = _dense_kuu([kernel], Bs, [x])
    Ga, Gb = _pair_maps(s.draw, s.zlen, s.grid.device)
    err = max(np.abs(Ga @ Ga.T - K).max(), np.abs(Gb @ Gb.T - K).max())
    print('exhausted ladder: clipped %.3e (NumPy %.3e), max|G G^T - K| %.3e <= %.3e' % (st.clipped, want, err, worst))
    assert 0 < err <= worst, (err, worst)


# --- 3. polynomial form -----------------------------------------------------------------------------
def check_polynomial():
    rng = np.random.RandomState(3)
    D, kernels = 2, [RBF(1.0), RBF(10.0)]
    A, kap, Bs = _coreg(rng, D, 2, (1, 1))
    g = _grid_op(kernels, A, kap, [X128], D)
    s = GridSampler(g, kernels, A, kap, [X128])
    assert g.top_forms()[0] == [1, 1], g.top_forms()
    assert [st.form for st in s.stats] == ['polynomial'] * 2 and s.stats[0].rank in (24, 32, 36, 40, 48)
    assert s.zlen == 2 * 3 * s.stats[0].rank
    _check_cov(s, _dense_kuu(kernels, Bs, [X128]), POLY_TOL, 'polynomial m 128')


def check_mixed_forms():
    """One polynomial, one filter and one transform row in one operator."""
    rng = np.random.RandomState(4)
    D, kernels = 1, [RBF(10.0), Matern32(10.0), RBF(300.0)]
    A, kap, Bs = _coreg(rng, D, 3, (0, 0, 0))
    g = _grid_op(kernels, A, kap, [X128], D)
    s = GridSampler(g, kernels, A, kap, [X128])
    assert g.top_forms()[0] == [1, 2, 0], g.top_forms()
    assert [st.form for st in s.stats] == ['polynomial', 'embedding', 'embedding'], s.stats
    assert all(st.clipped <= pw.CLIP_TOL for st in s.stats), s.stats
    _check_cov(s, _dense_kuu(kernels, Bs, [X128]), POLY_TOL, 'mixed forms m 128')


# --- 4. two passes ----------------------------------------------------------------------------------
TWO_PASS = ((128, 'rbf'), (1200, 'matern'), (2000, 'matern'))


def check_transform_paths(m, kind, D):
    """3 draws from explicit noise against np.fft.ifft of the scaled, mixed noise.  m = 128:
    the RBF row of inv_lengthscale 1 forced to embed, whose ladder ends at Ls = 2048 (the longest
    transform of the one-launch kernel); m = 1200 / 2000: Ls = 2560 = 5 * 512 (an odd first
    pass) and 4096, both past it.

    The Matern rows take their scale sqrt(lambda / Ls) from NumPy's own spectrum.  The RBF row
    cannot: most of its spectrum lies below the rounding of its transform (1e-16 of the largest
    eigenvalue), where two correct transforms return unrelated values and the square roots of
    those differ by sqrt(1e-16) = 1e-8 of the largest scale -- in the draw, not in its covariance.
    There the restatement scales with the spectrum the sampler reports (rl_sampler_spectrum_host),
    after holding that spectrum against NumPy's at the transform's rounding, 1e-13 max|lambda|;
    the transform, the mix and the crop are held to 1e-10 either way."""
    from runlmc_amd._native import sampler_length
    rng = np.random.RandomState(m + D)
    x = np.arange(m) / (m - 5.0)
    kernel = RBF(1.0) if kind == 'rbf' else Matern32(30.0)
    A, kap, _ = _coreg(rng, D, 1, (1,))
    g = _grid_op([kernel], A, kap, [x], D)
    s = GridSampler(g, [kernel], A, kap, [x], forms='embedding')
    (st,) = s.stats
    Ls = st.Ls
    if kind == 'rbf':
        assert Ls == 2048, st
    else:
        assert Ls == sampler_length(g.lib, 2 * m) > 2048 and st.clipped <= pw.CLIP_TOL, st
    F = pw.channel_matrix(A[0], kap[0], D)
    C = F.shape[1]
    assert s.zlen == C * Ls
    Z = rng.randn(4, s.zlen)
    U = s.draw(torch.from_numpy(Z).to(g.device), 3).cpu().numpy()
    assert U.shape == (3, D * m)
    lam = np.clip(_numpy_spectrum(kernel, [x[1] - x[0]], [Ls]), 0, None)
    if kind == 'rbf':
        own = s.spectrum(0)
        assert own.min() >= 0.0
        assert np.abs(own - lam).max() <= 1e-13 * lam.max(), np.abs(own - lam).max() / lam.max()
        lam = own
    ref = np.zeros((4, D * m))
    for p in range(2):
        xi = (Z[2 * p] + 1j * Z[2 * p + 1]).reshape(C, Ls)
        y = Ls * np.fft.ifft(np.sqrt(lam / Ls)[None] * (F @ xi), axis=1)[:, :m]
        ref[2 * p], ref[2 * p + 1] = y.real.reshape(-1), y.imag.reshape(-1)
    err = np.abs(U - ref[:3]).max() / np.abs(ref).max()
    print('m %d D %d Ls %d: relative error %.3e' % (m, D, Ls, err))
    assert err <= PRODUCT_TOL, err


# --- 5. 2-D grid ------------------------------------------------------------------------------------
def check_grid_2d():
    rng = np.random.RandomState(5)
    axes = [np.arange(6) / 5.0, np.arange(5) / 4.0]
    D, kernels = 2, [RBF(100.0), Matern32(30.0)]
    steps = [0.2, 0.25]
    for k in kernels:
        assert min(_numpy_clipped(k, steps, [2 * e * 6, 2 * e * 5]) for e in (1, 2, 4, 8)) <= pw.CLIP_TOL
    A, kap, Bs = _coreg(rng, D, 2, (1, 1))
    s = GridSampler(_grid_op(kernels, A, kap, axes, D), kernels, A, kap, axes)
    assert all(st.form == 'embedding' and st.clipped <= pw.CLIP_TOL for st in s.stats), s.stats
    _check_cov(s, _dense_kuu(kernels, Bs, axes), PRODUCT_TOL, '2-D grid 6 x 5')


def check_grid_2d_limit():
    """A 2-D grid with an axis of 130 points and a Matern row of long length scale: the ladder
    wants 16 x 130 points on that axis, more than the device code's 2048 per axis.  It stops at
    the last length the device accepts, warns, reports what that length clips, and draws."""
    rng = np.random.RandomState(6)
    axes = [np.arange(130) / 129.0, np.arange(3) / 2.0]
    D, kernels = 1, [Matern32(1.0)]
    A, kap, Bs = _coreg(rng, D, 1, (0,))
    g = _grid_op(kernels, A, kap, axes, D)
    catch = _Catch()
    log = logging.getLogger(pw.__name__)
    log.addHandler(catch)
    try:
        s = GridSampler(g, kernels, A, kap, axes)
    finally:
        log.removeHandler(catch)
    assert any(r.levelno >= logging.WARNING and 'clips' in r.getMessage() for r in catch.records)
    (st,) = s.stats
    assert st.form == 'embedding' and 1040 <= st.Ls[0] <= 2048 and s.embed == 8, st
    want = _numpy_clipped(kernels[0], [1 / 129.0, 0.5], st.Ls)
    assert pw.CLIP_TOL < st.clipped and want / 2 <= st.clipped <= want * 2, (st, want)
    Z = s.noise(3, 0, 3)
    U = s.draw(Z, 3).cpu().numpy()
    assert U.shape == (3, 390) and np.all(np.isfinite(U)) and U.std() > 0.1
    # ... against the NumPy restatement of the two passes without the twiddle; 1e-7: eigenvalues
    # within rounding of zero fall on either side of the clip in two transforms, and their square
    # roots differ by sqrt(2^-52) = 1.5e-8 of the largest scale
    lam = np.clip(_numpy_spectrum(kernels[0], [1 / 129.0, 0.5], st.Ls), 0, None)
    Zh = Z.cpu().numpy()
    xi = (Zh[0] + 1j * Zh[1]).reshape(st.Ls)
    y = np.prod(st.Ls) * np.fft.ifft2(np.sqrt(lam / np.prod(st.Ls)) * np.sqrt(kap[0][0]) * xi)[:130, :3]
    err = max(np.abs(U[0] - y.real.reshape(-1)).max(), np.abs(U[1] - y.imag.reshape(-1)).max())
    print('2-D grid 130 x 3 at the per-axis limit: Ls %s clipped %.3e, error %.3e' % (st.Ls, st.clipped, err))
    assert err <= 1e-7 * np.abs(y).max(), err


# --- 6. posterior map -------------------------------------------------------------------------------
SOLVE_TOL = 1e-9


@functools.lru_cache(maxsize=None)
def _small_model(kind, normalize=False):
    """Small models, smallest noise 0.1.  '1d': two outputs, two smooth RBF rows on a 128-point
    grid, 62 data points -- the operator is in the polynomial form, so the solver is the direct one
    (Woodbury with refinement) and the sampler takes the polynomial rows.  'split': two outputs,
    rank-one couplings plus kappa, one kernel per input column on two grids, 13 data points,
    embedding rows, Krylov solves.  '2d': a Matern row on a 2-D grid, ONE output and kappa alone,
    12 data points: a posterior map is fed one unit vector per noise value, each of them a Krylov
    solve, and a 2-D embedding of two outputs with couplings has 1 754 of them (250 s on the
    emulator build).  That model is '2d2' (the kernel kinds of lmc_2d, two outputs, rank-one
    couplings plus kappa, 13 data points), which the GPU run checks; the 2-D sampler's own mixing
    of outputs is also held in check_grid_2d."""
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    rng = np.random.RandomState(60 + len(kind))
    if kind == '1d':
        D, lens = 2, (32, 30)
        Xs = [np.sort(rng.rand(n, 1), axis=0) for n in lens]
        kerns, m, ranks = [RBF(1.0), RBF(10.0)], [124], [1, 1]
    elif kind == '2d2':
        D, lens = 2, (7, 6)
        Xs = [rng.rand(n, 2) for n in lens]
        kerns, m, ranks = [RBF(60.0), Matern32(10.0)], [2, 2], [1, 1]
    elif kind == '2d':
        D, lens = 1, (12,)
        Xs = [rng.rand(n, 2) for n in lens]
        kerns, m, ranks = [Matern32(10.0)], [2, 2], [1]
    else:
        D, lens = 2, (7, 6)
        Xs = [rng.rand(n, 2) for n in lens]
        kerns, m, ranks = [RBF(20.0, active_dims=[0]), Matern32(6.0, active_dims=[1])], [4, 3], [1, 1]
    fk = FunctionalKernel(D=D, lmc_kernels=kerns, lmc_ranks=ranks)
    fk.coreg_vecs = [rng.randn(r, D) if D > 1 else np.zeros((r, D)) for r in ranks]
    fk.coreg_diags = [np.abs(rng.randn(D)) + 0.1 for _ in kerns]
    fk.noise = np.array([0.1, 0.15][:D])
    Ys = [np.sin(3 * X.sum(axis=1)) + 0.3 * rng.randn(len(X)) + 2.0 * d for d, X in enumerate(Xs)]
    np.random.seed(5)
    model = InterpolatedLLGP(Xs, Ys, normalize=normalize, m=m, functional_kernel=fk,
                             trace_iterations=2, tolerance=SOLVE_TOL)
    model._ensure()
    return model


class _tight_krylov:
    """Krylov solves that reach 1e-9 on these small systems: MINRES ended by the residual rule
    alone (SciPy's own exits stop near 1e-7 here), the rule checked every 10 iterations, up to
    400 of them (the reference's cap of n iterations is too few in floating point)."""

    def __enter__(self):
        from runlmc_amd.approx.iterative import Iterative
        self.saved = (Iterative.SCIPY_EXITS, Iterative.CHECK_EVERY)
        Iterative.SCIPY_EXITS, Iterative.CHECK_EVERY = False, 10

    def __exit__(self, *exc):
        from runlmc_amd.approx.iterative import Iterative
        Iterative.SCIPY_EXITS, Iterative.CHECK_EVERY = self.saved


def _test_points(model, npts=(5, 3)):
    rng = np.random.RandomState(9)
    return [rng.rand(n, model.input_dim) * 0.9 + 0.05 for n in ((8,) if model.output_dim == 1 else npts)]


@functools.lru_cache(maxsize=None)
def _dense_model(kind, normalize=False):
    """Dense pieces of the SKI model from the model's own grids and interpolants: block-diagonal
    K_UU over the terms, W = [W_1 W_2 ...], K~, the posterior on the grids, test interpolants."""
    import scipy.linalg as la
    from runlmc_amd.approx.interpolation import multi_interpolant
    model = _small_model(kind, normalize)
    fk = model._functional_kernel
    blocks, Ws, Wt = [], [], []
    Xt = _test_points(model)
    for ad in model._grid_kernels:
        kidx = fk.active_dims[ad]
        Bs = [fk.coreg_mats()[q] for q in kidx]
        blocks.append(_dense_kuu([fk.kernels[q] for q in kidx], Bs, model.grid_axes[ad]))
        Ws.append(model.interpolants[ad][0].toarray())
        Wt.append(multi_interpolant([X[:, list(ad)] for X in Xt], *model.grid_axes[ad]).toarray())
    Kuu, W, Wt = la.block_diag(*blocks), np.hstack(Ws), np.hstack(Wt)
    eps = np.repeat(fk.noise, [len(Y) for Y in model.Ys])
    Kt = W @ Kuu @ W.T + np.diag(eps)
    KW = Kuu @ W.T
    cov = Kuu - KW @ np.linalg.solve(Kt, KW.T)
    mean = KW @ np.linalg.solve(Kt, model.y)
    return dict(Xt=Xt, Kuu=Kuu, W=W, Wt=Wt, eps=eps, Kt=Kt, KW=KW, cov=cov, mean=mean)


def check_posterior_map(kind):
    """With y = 0 the posterior draw is linear in (z, e): its matrix from unit vectors, and
    W* G G^T W*^T against the dense posterior covariance W*(K_UU - K_UU W^T K~^-1 W K_UU)W*^T
    within 1e-6 max|K_UU| (residual 1e-9 times ||K~^-1|| <= 10 times ||K_UU W^T||, with a margin).
    With zero noise and the data the draw is predict's mean to 1e-8."""
    model = _small_model(kind)
    d = _dense_model(kind)
    K = model._K
    samplers = model._pathwise_samplers(16)
    dev, n = K.device, len(model.y)
    zl = [s.zlen for s in samplers]
    total = sum(zl) + n

    def draw(Zall):
        # columns: the terms' noise one after another, then e (rows 2p + 1 of e feed draw 2p + 1)
        rows = Zall.shape[0]
        Zs, o = [], 0
        for z in zl:
            Zs.append(Zall[:, o:o + z].contiguous())
            o += z
        E = Zall[:, o:].contiguous()
        out = pw.posterior_grid_draws(K, samplers, torch.zeros(n, dtype=torch.float64, device=dev),
                                      Zs, E, tol=SOLVE_TOL, maxiter=400)
        assert out.max_residual < SOLVE_TOL, (out.solver, out.max_residual, out.iterations.max())
        assert out.draws[0].shape[0] == rows
        return torch.cat(out.draws, dim=1)

    # the e of draw 2p is row 2p of E: unit vectors in the e columns of the ODD row feed draw
    # 2p + 1 alone, so the pair maps hold e's columns in G_a's first half and G_b's second half
    with _tight_krylov():
        Ga, Gb = _pair_maps(draw, total, dev, chunk=512)
    sc = np.abs(d['Kuu']).max()
    ref = d['Wt'] @ d['cov'] @ d['Wt'].T
    for name, G in (('a', Ga), ('b', Gb)):
        err = np.abs(d['Wt'] @ G @ G.T @ d['Wt'].T - ref).max()
        print('%s posterior map %s: max covariance error %.3e (bound %.3e)' % (kind, name, err, 1e-6 * sc))
        assert err <= 1e-6 * sc, (kind, name, err)
    # zero noise: the mean -- with the model's own solver settings against predict (the same
    # solve), with the tight ones against the dense mean
    y = torch.from_numpy(model.y).to(dev)
    Zs = [torch.zeros((2, z), dtype=torch.float64, device=dev) for z in zl]
    E0 = torch.zeros((1, n), dtype=torch.float64, device=dev)

    def at_test(out):
        host = {ad: u.cpu().numpy() for ad, u in zip(model._grid_kernels, out.draws)}
        return np.concatenate(pw.PathwiseDraws(model, host, 0)(d['Xt']), axis=1)[0]

    got = at_test(pw.posterior_grid_draws(K, samplers, y, Zs, E0, tol=SOLVE_TOL))
    want = np.concatenate(model.predict(d['Xt'])[0])
    print('%s zero-noise draw against predict: %.3e' % (kind, np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-8)
    with _tight_krylov():
        out = pw.posterior_grid_draws(K, samplers, y, Zs, E0, tol=SOLVE_TOL, maxiter=400)
    assert out.max_residual < SOLVE_TOL, (out.solver, out.max_residual)
    np.testing.assert_allclose(at_test(out), d['Wt'] @ d['mean'], rtol=0, atol=1e-6)


def check_zero_noise_mean_golden(name):
    """The stored cases lmc_2d and lmc_split at their own sizes: the zero-noise draw is predict's
    mean to 1e-8, the model's solve tolerance set to 1e-9 so that both sides are solved that far."""
    import predict_suite as pr
    from cases import Case
    if name == 'lmc_split':
        model = pr._split_model('on-the-fly', None)[0]
        Xt = [np.random.RandomState(9).rand(5 + d, 2) * 0.9 + 0.05 for d in range(model.output_dim)]
    else:
        c = Case(name)
        model = pr._model(c, 'on-the-fly')
        Xt = pr._test_points(c.D, c.P)
    model._deriv_service._tol = SOLVE_TOL
    model._ensure()
    K, dev, n = model._K, model._K.device, len(model.y)
    samplers = model._pathwise_samplers(16)
    Zs = [torch.zeros((2, s.zlen), dtype=torch.float64, device=dev) for s in samplers]
    out = pw.posterior_grid_draws(K, samplers, torch.from_numpy(model.y).to(dev), Zs,
                                  torch.zeros((1, n), dtype=torch.float64, device=dev), tol=SOLVE_TOL)
    host = {ad: u.cpu().numpy() for ad, u in zip(model._grid_kernels, out.draws)}
    got = np.concatenate(pw.PathwiseDraws(model, host, 0)(Xt), axis=1)[0]
    want = np.concatenate(model.predict(Xt)[0])
    print('%s zero-noise draw against predict: %.3e (residual %.3e)'
          % (name, np.abs(got - want).max(), out.max_residual))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-8)


# --- 7. the noise stream ----------------------------------------------------------------------------
def check_noise_moments():
    lib = _lib.get_library()
    N = 2 ** 20
    z = normal_fill(lib, 12345, 0, 4, N // 4, lib.torch_device(0)).cpu().numpy().reshape(-1)
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2
    print('normal_fill, 2^20 values: mean %.3e var - 1 %.3e kurtosis - 3 %.3e' % (mean, var - 1, kurt - 3))
    assert abs(mean) < 5 / np.sqrt(N)
    assert abs(var - 1) < 5 * np.sqrt(2.0 / N)
    assert abs(kurt - 3) < 5 * np.sqrt(24.0 / N)
    # element (s, j) is a function of (seed, s, j): windows of draws and of columns agree
    dev = lib.torch_device(0)
    a = normal_fill(lib, 7, 0, 6, 1001, dev).cpu().numpy()
    b = normal_fill(lib, 7, 2, 3, 77, dev).cpu().numpy()
    assert np.array_equal(a[2:5, :77], b)
    assert not np.array_equal(a, normal_fill(lib, 8, 0, 6, 1001, dev).cpu().numpy())
    assert len(np.unique(a)) == a.size


def check_stream_invariance():
    """Prior draws bit for bit: the same seed twice, size 5 against the first five of size 8,
    batch 3 against batch 16, the seeded path against explicit noise from normal_fill.  Posterior
    draws pass through the solver, which ends on its residual rule: two runs whose tiles differ
    agree to 2 tol ||K_UU W^T||_2 / min eps; the same tiling is again bit for bit."""
    model = _small_model('1d')
    d = _dense_model('1d')
    Xt = d['Xt']
    cat = lambda draws: np.concatenate(draws(Xt), axis=1)
    p8 = model.prior_draws(8, seed=11)
    assert np.array_equal(cat(p8), cat(model.prior_draws(8, seed=11)))
    assert not np.array_equal(cat(p8), cat(model.prior_draws(8, seed=12)))
    assert np.array_equal(cat(p8)[:5], cat(model.prior_draws(5, seed=11)))
    assert np.array_equal(cat(p8), cat(model.prior_draws(8, seed=11, batch=3)))
    (s,) = model._pathwise_samplers(16)
    Z = normal_fill(s.grid.lib, pw.stream_seed(11, pw.STREAM_TERM0), 0, 8, s.zlen, s.grid.device)
    (ad,) = model._grid_kernels
    assert np.array_equal(s.draw(Z).cpu().numpy(), p8.grid_draws[ad])
    # embedding rows (two grids): pairs of draws never straddle a tile
    split = _small_model('split')
    Xs = _dense_model('split')['Xt']
    cats = lambda draws: np.concatenate(draws(Xs), axis=1)
    e8 = cats(split.prior_draws(8, seed=11))
    assert all(st.form == 'embedding' for smp in split._pathwise_samplers(16) for st in smp.stats)
    assert np.array_equal(e8, cats(split.prior_draws(8, seed=11, batch=3)))
    assert np.array_equal(e8[:5], cats(split.prior_draws(5, seed=11, batch=2)))
    assert np.array_equal(e8[:1], cats(split.prior_draws(1, seed=11)))
    assert len(np.unique(e8)) == e8.size
    q8 = model.posterior_draws(8, seed=11)
    assert np.array_equal(cat(q8), cat(model.posterior_draws(8, seed=11)))
    assert all(t.max_residual < SOLVE_TOL for t in q8.info), [t.max_residual for t in q8.info]
    bound = 2 * SOLVE_TOL * np.linalg.norm(d['KW'], 2) / d['eps'].min() * np.abs(d['Wt']).sum(axis=1).max()
    for other in (model.posterior_draws(5, seed=11), model.posterior_draws(8, seed=11, batch=3)):
        assert all(t.max_residual < SOLVE_TOL for t in other.info)
        err = np.abs(cat(q8)[:other.size] - cat(other)).max()
        print('posterior draws, another tiling: %.3e (bound %.3e)' % (err, bound))
        assert err <= bound


# --- 8. the model -----------------------------------------------------------------------------------
def check_model_interface():
    model = _small_model('1d', True)
    d = _dense_model('1d', True)
    Xt = d['Xt']
    for size in (1, 3):
        draws = model.posterior_draws(size, seed=3)
        out = draws(Xt)
        assert [o.shape for o in out] == [(size, len(x)) for x in Xt]
        # de-normalised: the raw interpolation of the grid draws, scaled and shifted per output
        (ad,) = draws.grid_draws
        raw = draws.grid_draws[ad] @ d['Wt'].T
        for o, r, (mu, sd) in zip(out, np.split(raw, [len(Xt[0])], axis=1), model.normalizer):
            np.testing.assert_allclose(o, r * sd + mu, rtol=0, atol=1e-12 * (abs(mu) + sd))
        # observation noise: the test stream's normals times sqrt(noise) sd, the same on every call
        noisy = draws(Xt, noise=True)
        lens = [len(x) for x in Xt]
        e = normal_fill(model._K.device_operator().lib, pw.stream_seed(3, pw.STREAM_TEST), 0, size,
                        sum(lens), model._K.device).cpu().numpy()
        sds = np.repeat([sd for _, sd in model.normalizer], lens)
        want = np.concatenate(out, axis=1) + e * np.sqrt(np.repeat(model._functional_kernel.noise, lens)) * sds
        np.testing.assert_allclose(np.concatenate(noisy, axis=1), want, rtol=0, atol=1e-12)
        assert np.array_equal(np.concatenate(noisy, axis=1), np.concatenate(draws(Xt, noise=True), axis=1))
    # the one-call form, prior draws, empty test arrays
    one = model.posterior_samples(Xt, size=3, seed=3)
    assert np.array_equal(np.concatenate(one, axis=1), np.concatenate(out, axis=1))
    assert [o.shape for o in model.prior_draws(2, seed=1)(Xt)] == [(2, len(x)) for x in Xt]
    empty = draws([Xt[0], np.zeros((0, 1))], noise=True)
    assert empty[0].shape == (3, len(Xt[0])) and empty[1].shape == (3, 0)
    assert [o.shape for o in draws([np.zeros((0, 1))] * 2)] == [(3, 0)] * 2
    # one set of draws at two test sets that share points
    both = [np.vstack([Xt[0][:2], [[0.5]]]), Xt[1][::-1].copy()]
    assert model.output_dim == 2
    o2 = draws(both)
    np.testing.assert_allclose(o2[0][:, :2], out[0][:, :2], rtol=0, atol=1e-12)
    np.testing.assert_allclose(o2[1][:, ::-1], out[1], rtol=0, atol=1e-12)
    # errors
    for bad in (0, -1, 1.5, True):
        try:
            model.posterior_draws(bad)
        except ValueError:
            pass
        else:
            raise AssertionError('size %r accepted' % (bad,))
    for call in (lambda: draws(Xt[:1]), lambda: model.posterior_samples(Xt + Xt)):
        try:
            call()
        except ValueError:
            pass
        else:
            raise AssertionError('a wrong number of outputs was accepted')


def check_model_statistics():
    """2048 seeded draws at 8 test points against the dense posterior of the SKI model: the
    empirical mean within 5 sigma / sqrt(S), the empirical variance within 5 sqrt(2 / S)
    relative.  The seed is fixed: the check is deterministic."""
    model = _small_model('1d')
    d = _dense_model('1d')
    S = 2048
    f = np.concatenate(model.posterior_draws(S, seed=2024, batch=512)(d['Xt']), axis=1)
    assert f.shape == (S, 8)
    mean = d['Wt'] @ d['mean']
    var = np.diag(d['Wt'] @ d['cov'] @ d['Wt'].T)
    zm = np.abs(f.mean(axis=0) - mean) / np.sqrt(var / S)
    zv = np.abs(f.var(axis=0) / var - 1) / np.sqrt(2.0 / S)
    print('2048 draws: mean z-scores up to %.2f, variance z-scores up to %.2f' % (zm.max(), zv.max()))
    assert np.all(zm < 5) and np.all(zv < 5), (zm, zv)
    # and the prior: zero mean, the SKI model's prior variance
    f0 = np.concatenate(model.prior_draws(S, seed=2024, batch=512)(d['Xt']), axis=1)
    var0 = np.diag(d['Wt'] @ d['Kuu'] @ d['Wt'].T)
    assert np.all(np.abs(f0.mean(axis=0)) / np.sqrt(var0 / S) < 5)
    assert np.all(np.abs(f0.var(axis=0) / var0 - 1) / np.sqrt(2.0 / S) < 5)
