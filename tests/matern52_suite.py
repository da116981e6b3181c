"""Checks of the Matern-5/2 kernel (runlmc_amd.kern.stationary.Matern52) through every layer:
the host class, the detection of degree-3 exponential-polynomial top rows (csrc/rl_gridop.hip:
sf_detect), the four-state recursive filter (csrc/rl_filter.h at NS = 4), the exact dense
likelihood's device formula (csrc/rl_exact.h: EX_MATERN52) and the model.  Shared by the CPU run
on the emulator (tests/test_matern52_emu.py) and the GPU run (tests/test_matern52_gpu.py); every
function uses whichever native library is active.

The oracle has no Matern-5/2 specification, so the kernel is written here in NumPy from its closed
form (Matern52Spec, the duck-typed surface oracle.kernels.KernelSpec consumes):
    k(r) = (1 + s + s^2 / 3) exp(-s),  s = sqrt(5) gamma r,
    dk / dgamma = -(5 gamma r^2 / 3) (1 + sqrt(5) gamma r) exp(-sqrt(5) gamma r).
On a regular grid of step h the kernel row is (1 + a i + a^2 i^2 / 3) rho^i and the derivative
row -(5 gamma h^2 / 3) (i^2 + a i^3) rho^i with a = sqrt(5) gamma h, rho = exp(-a): degree 2
(three filter states) and degree 3 (four)."""
import functools
import os

import numpy as np
import scipy.linalg as la

from oracle import operators as ops
from oracle import likelihood as olik
from oracle.kernels import KernelSpec, RBFSpec, ScaledSpec
from cases import Case

import exact_suite as es
import parity_suite as ps
from parity_suite import _close, _poly_product, _matern32, _d_matern32

from runlmc_amd.kern.stationary import RBF, Matern52, Scaled
from runlmc_amd.lmc.functional_kernel import FunctionalKernel

ROOT5 = np.sqrt(5.0)


def k52(r, gamma):
    s = ROOT5 * gamma * r
    return (1.0 + s + s * s / 3.0) * np.exp(-s)


def dk52(r, gamma):
    return -(5.0 * gamma * r * r / 3.0) * (1.0 + ROOT5 * gamma * r) * np.exp(-ROOT5 * gamma * r)


class Matern52Spec:
    """The oracle-side twin (see oracle/kernels.py for the three kernels the reference has)."""
    n_params = 1

    def __init__(self, inv_lengthscale=1.0, active_dims=None):
        self.inv_lengthscale = float(inv_lengthscale)
        self.active_dims = active_dims

    def from_dist(self, d):
        return k52(np.asarray(d, dtype=float), self.inv_lengthscale)

    def kernel_gradient(self, d):
        return [dk52(np.asarray(d, dtype=float), self.inv_lengthscale)]


# --- 1. the kernel class (host) ---------------------------------------------------------------
def check_kernel_class():
    r = np.array([0.0, 1e-8, 0.3, 5.0])
    for gamma in (1.0, 2.5, 0.3):
        k = Matern52(gamma)
        assert k.name == 'matern52' and k.active_dims is None
        np.testing.assert_array_equal(k.param_array, [gamma])
        got = k.from_dist(r)
        np.testing.assert_allclose(got, k52(r, gamma), rtol=1e-14, atol=0)
        assert got[0] == 1.0
        # the gradient: the closed form entry by entry (nothing cancels at r = 0: the entry at
        # 1e-8 keeps its digits), and a central difference in gamma at 1e-7 of the largest entry
        (g,) = k.kernel_gradient(r)
        assert g[0] == 0.0 and g[1] < 0.0
        np.testing.assert_allclose(g, dk52(r, gamma), rtol=1e-14, atol=0)
        rr = np.concatenate((r, np.linspace(0, 3, 50)))
        h = 1e-5 * gamma
        fd = (Matern52(gamma + h).from_dist(rr) - Matern52(gamma - h).from_dist(rr)) / (2 * h)
        (g,) = k.kernel_gradient(rr)
        assert np.abs(g - fd).max() <= 1e-7 * np.abs(fd).max(), np.abs(g - fd).max()
    k = Matern52(1.0)
    k.set_params([2.0])
    assert k.inv_lengthscale == 2.0
    k.update_gradient([0.5])
    np.testing.assert_array_equal(k.gradient, [0.5])
    assert Matern52(1.0, name='m', active_dims=[1]).active_dims == [1]
    # under Scaled: the inner kernel's parameters, the scale's derivative LAST
    rr = np.linspace(0, 3, 50)
    sk = Scaled(Matern52(1.7), 2.5)
    assert sk.name == 'scaled_matern52'
    np.testing.assert_array_equal(sk.param_array, [1.7])
    np.testing.assert_allclose(sk.from_dist(rr), 2.5 * k52(rr, 1.7), rtol=1e-14)
    grads = sk.kernel_gradient(rr)
    assert len(grads) == 2
    np.testing.assert_allclose(grads[0], 2.5 * dk52(rr, 1.7), rtol=1e-14)
    np.testing.assert_allclose(grads[1], k52(rr, 1.7), rtol=1e-14)
    h = 1e-5
    fd_g = (Scaled(Matern52(1.7 + h), 2.5).from_dist(rr) -
            Scaled(Matern52(1.7 - h), 2.5).from_dist(rr)) / (2 * h)
    fd_c = (Scaled(Matern52(1.7), 2.5 + h).from_dist(rr) -
            Scaled(Matern52(1.7), 2.5 - h).from_dist(rr)) / (2 * h)
    assert np.abs(grads[0] - fd_g).max() <= 1e-7 * np.abs(fd_g).max()
    assert np.abs(grads[1] - fd_c).max() <= 1e-7 * np.abs(fd_c).max()
    sk.set_params([0.9])
    assert sk.k.inv_lengthscale == 0.9 and sk.scale == 2.5
    sk.update_gradient([0.25, 4.0])
    np.testing.assert_array_equal(sk.k.gradient, [0.25])
    assert sk.scale_gradient == 4.0


# --- 2. detection -------------------------------------------------------------------------------
def _form_of(g, row):
    D = g.D if hasattr(g, 'D') else 2
    g.set_lmc(np.asarray(row)[None], [None], [np.ones(D)])
    forms, _ = g.top_forms()
    return forms


def check_detection(m, gamma):
    from runlmc_amd._native import GridOp
    saved = os.environ.pop('RUNLMC_NO_FILTER', None)
    try:
        x = np.linspace(0, 1, m)
        i = np.arange(m, dtype=float)
        rho = np.exp(-ROOT5 * gamma * (x[1] - x[0]))
        rows = dict(k=k52(x, gamma), dk=dk52(x, gamma), cubic=i ** 3 * rho ** i)
        g = GridOp(2, m, 1)
        for name, row in rows.items():
            assert _form_of(g, row) == [2], (name, m, gamma, _form_of(g, row))
        # degree 4 is outside the model; so is the derivative row with a ripple of 1e-10
        # (the acceptance is an l1 bound over the whole row at 2e-14); the handle follows the
        # rows as they are swapped in and out
        assert _form_of(g, i ** 4 * rho ** i) != [2]
        assert _form_of(g, rows['dk']) == [2]
        assert _form_of(g, rows['dk'] + 1e-10 * np.cos(40 * x)) != [2]
        assert _form_of(g, rows['k']) == [2]
        assert _form_of(g, rows['cubic']) == [2]
        os.environ['RUNLMC_NO_FILTER'] = '1'
        g0 = GridOp(2, m, 1)
        for name, row in rows.items():
            assert _form_of(g0, row) != [2], name
    finally:
        os.environ.pop('RUNLMC_NO_FILTER', None)
        if saved is not None:
            os.environ['RUNLMC_NO_FILTER'] = saved


# --- 3. four-state products ---------------------------------------------------------------------
SHAPES = ((2, 1, 601, 1), (3, 2, 2500, 3), (5, 2, 700, 2), (16, 3, 601, 1), (2, 2, 20011, 2))


def _inputs(rng, D, m, k, x):
    """Batches of k vectors: random ones and a coherent one (cos(5 x) + 1 on every output: what
    a wrongly carried state shows up under)."""
    coherent = np.cos(5 * np.tile(x, D)) + 1.0
    X = rng.randn(k, D * m)
    if k > 1:
        X[-1] = coherent
        return [X]
    return [X, coherent[None]]


def _oracle_product(tops, Bs, X):
    toeps = [ops.BTTBOracle(t) for t in tops]
    return np.array([ops.grid_sum_matvec(Bs, toeps, r) for r in X])


def _oracle_top(top, X, D, m):
    T = ops.BTTBOracle(top)
    return np.array([np.concatenate([T.matvec(r) for r in v.reshape(D, m)]) for v in X])


def _check_operator(g, tops, Bs, Xs, want_forms):
    forms, structured = g.top_forms()
    assert forms == want_forms and structured, (forms, structured)
    for X in Xs:
        ref = _oracle_product(tops, Bs, X)
        fft = g.matmat_host(X)                  # below the gate: transform kernels
        _close(fft, ref)
        flt = _poly_product(g, X)
        _close(flt, ref)
        _close(flt, fft, 1e-12)


def check_four_state(D, Q, m, k, scan2=False):
    """(a) an all-Matern-5/2 operator (three states), LMC factors of rank 1 and 2, then dense B;
    (b) an operator [Matern-5/2, its d/dgamma row, Matern-3/2]: every filter top at four states,
    rank-one factors on each (the four-state top among them);
    (c) single-top products of [k52, dk52, k32, dk32, exp] from one handle (the gradient's path);
    (e) at m = 2500 a mixed operator [rbf, dk52, periodic(3)]: a polynomial part accumulating onto
    a four-state filter part.
    Each against the oracle at _close's default and against the transform kernels of the same
    handle (batch below the gate) at 1e-12.  scan2: the chunk chain that reads its chunk states
    twice (k_sf_scan<4>; the issue's check (d))."""
    from runlmc_amd._native import GridOp
    knobs = ('RUNLMC_NO_FILTER', 'RUNLMC_SF_SCAN2')
    saved = {kn: os.environ.pop(kn, None) for kn in knobs}
    rng = np.random.RandomState(52 + D + m)
    try:
        if scan2:
            os.environ['RUNLMC_SF_SCAN2'] = '1'
        x = np.linspace(0, 1, m)
        gam = np.logspace(0, 1, Q) * (1.0 if m > 1200 else 3.0)
        Xs = _inputs(rng, D, m, k, x)
        # (a)
        mat = np.array([k52(x, g_) for g_ in gam])
        A = [rng.randn(1 + q % 2, D) for q in range(Q)]
        kap = [np.abs(rng.randn(D)) + 0.1 for _ in range(Q)]
        Bs = ops.coreg_mats(A, kap)
        g = GridOp(D, m, Q)
        g.set_lmc(mat, A, kap)
        assert g.form()[0] == 0                     # (not the polynomial form)
        _check_operator(g, mat, Bs, Xs, [2] * Q)
        g.set_dense(mat, np.array(Bs))
        for X in Xs:
            _close(_poly_product(g, X), _oracle_product(mat, Bs, X))
        # (b)
        tops = np.array([k52(x, gam[0]), dk52(x, gam[0]), _matern32(x, gam[0])])
        A3 = [rng.randn(1, D) for _ in range(3)]
        k3 = [np.abs(rng.randn(D)) + 0.1 for _ in range(3)]
        g3 = GridOp(D, m, 3)
        g3.set_lmc(tops, A3, k3)
        _check_operator(g3, tops, ops.coreg_mats(A3, k3), Xs, [2, 2, 2])
        # (c)
        gt = np.array([k52(x, gam[0]), dk52(x, gam[0]), _matern32(x, gam[-1]),
                       _d_matern32(x, gam[-1]), np.exp(-3.0 * x)])
        gg = GridOp(D, m, 5)
        gg.set_lmc(gt, [None] * 5, [np.zeros(D)] * 5)
        assert gg.top_forms()[0] == [2] * 5
        for t in range(5):
            for X in Xs:
                want = _oracle_top(gt[t], X, D, m)
                fft = gg.matmat_host(X, top=t)
                got = _poly_product(gg, X, top=t)
                _close(fft, want)
                _close(got, want)
                _close(got, fft, 1e-12)
        # (e)
        if m == 2500:
            mix = np.array([np.exp(-0.5 * x ** 2), dk52(x, 3.0),
                            np.exp(-0.5 * np.sin(np.pi * x / 3.0) ** 2)])
            Am = [rng.randn(1, D) for _ in range(3)]
            km = [np.abs(rng.randn(D)) + 0.1 for _ in range(3)]
            gm = GridOp(D, m, 3)
            gm.set_lmc(mix, Am, km)
            _check_operator(gm, mix, ops.coreg_mats(Am, km), Xs, [1, 2, 1])
    finally:
        for kn in knobs:
            os.environ.pop(kn, None)
            if saved[kn] is not None:
                os.environ[kn] = saved[kn]


# --- 4. the exact likelihood ----------------------------------------------------------------------
def _host_reference(spec, Xs, y, D):
    """log det, alpha and the four gradient families on the host (SciPy's Cholesky, K^-1 by
    cho_solve, dL/dt = 1/2 sum M dK with M = alpha alpha^T - K^-1), and K itself; inputs of any
    dimension, every kernel over all columns."""
    lens = [len(x) for x in Xs]
    X = np.vstack([np.asarray(x, dtype=float).reshape(len(x), -1) for x in Xs])
    n = len(X)
    ends = np.cumsum(lens)
    begins = ends - np.asarray(lens)
    o = np.repeat(np.arange(D), lens)
    dist = np.sqrt(np.square(X[:, None, :] - X[None, :, :]).sum(axis=-1))
    K = np.zeros((n, n))
    for B, k in zip(spec.coreg_mats(), spec._kernels):
        K += B[np.ix_(o, o)] * k.from_dist(dist)
    K[np.diag_indices(n)] += np.repeat(spec.noise, lens)
    cf = la.cho_factor(K, lower=True)
    logdet = 2.0 * np.log(np.diag(cf[0])).sum()
    alpha = la.cho_solve(cf, y)
    M = np.outer(alpha, alpha) - la.cho_solve(cf, np.identity(n))

    def block_sums(Kq):
        P = M * Kq
        return np.array([[P[begins[a]:ends[a], begins[b]:ends[b]].sum() for b in range(D)]
                         for a in range(D)])

    g = dict(coreg_vec=[], coreg_diag=[], kernel=[], noise=None)
    for a_q, B, k in zip(spec.coreg_vecs, spec.coreg_mats(), spec._kernels):
        S = block_sums(k.from_dist(dist))
        g['coreg_vec'].append(0.5 * np.atleast_2d(a_q).dot(S + S.T))
        g['coreg_diag'].append(0.5 * np.diag(S).copy())
        g['kernel'].append([0.5 * np.sum(B * block_sums(dk)) for dk in k.kernel_gradient(dist)])
    g['noise'] = np.array([0.5 * np.trace(M[b:e, b:e]) for b, e in zip(begins, ends)])
    return logdet, alpha, g, K


def _exact_model(n, D, P, seed):
    rng = np.random.RandomState(seed)
    lens = np.full(D, n // D)
    lens[:n - lens.sum()] += 1
    if P == 1:
        Xs = [np.sort(rng.rand(int(l)))[:, None] for l in lens]
    else:
        Xs = [rng.rand(int(l), P) for l in lens]
    A = [rng.randn(1 + q, D) * 0.6 for q in range(2)]
    kappa = [np.abs(rng.randn(D)) * 0.3 + 0.05 for _ in range(2)]
    noise = 0.05 + 0.1 * rng.rand(D)
    y = rng.randn(n)
    kerns = [Matern52(1.5), Scaled(Matern52(3.0), 1.7)]
    okerns = [Matern52Spec(1.5), ScaledSpec(Matern52Spec(3.0), 1.7)]
    fk = es._fk(D, kerns, A, kappa, noise, P=P)
    spec = KernelSpec(D, okerns, A, kappa, noise)
    spec.set_input_dim(P)
    return fk, spec, Xs, y, [int(l) for l in lens]


def check_exact(n, D, P=1):
    from runlmc_amd._native import ExactOp, exact_descriptors
    from runlmc_amd.lmc import ExactLMCLikelihood
    fk, spec, Xs, y, lens = _exact_model(n, D, P, seed=n * 7 + D + P)
    kinds, _, _, nder = exact_descriptors(fk.kernels)
    assert list(kinds) == [3, 3 | 16] and nder == [1, 2]
    logdet, alpha, ref, K = _host_reference(spec, Xs, y, D)
    # K and cross rows: the device formula against from_dist on host distances
    op = ExactOp(n, P)
    op.set(np.vstack(Xs), lens, fk.kernels, fk.coreg_mats(), fk.noise)
    es._close(op.dense(), K, 1e-12, 'dense')
    rng = np.random.RandomState(1)
    Xt = [rng.rand(3 + d, P) for d in range(D)]
    Kx = es._cross_dense(spec, Xt, Xs, D)
    es._close(op.cross(np.vstack(Xt), [len(v) for v in Xt]), Kx, 1e-12, 'cross')
    # the likelihood
    Ys = np.split(y, np.cumsum(lens)[:-1])
    lik = ExactLMCLikelihood(fk, Xs, Ys)
    assert abs(lik.log_det_K() - logdet) <= 1e-9 * abs(logdet), (lik.log_det_K(), logdet)
    es._compare_to_oracle(lik, ref, alpha, K, 2, rtol=1e-9)
    # two calls, two handles: the same bits
    lik2 = ExactLMCLikelihood(fk, Xs, Ys)
    S1, n1 = lik._op.grad_sums(lik._alpha_dev)
    S2, n2 = lik._op.grad_sums(lik._alpha_dev)
    assert np.array_equal(S1, S2) and np.array_equal(n1, n2)
    for u, v in zip(es._grads_flat(lik, 2), es._grads_flat(lik2, 2)):
        for a, b in zip(u, v):
            assert np.array_equal(a, b)
    assert lik.log_det_K() == lik2.log_det_K() and np.array_equal(lik.alpha(), lik2.alpha())


def check_exact_unknown_kind():
    """Kinds past Matern-5/2 are still rejected by rl_exact_set (no default formula)."""
    from runlmc_amd import _native
    fk, _, Xs, _, lens = _exact_model(17, 1, 1, seed=3)
    op = _native.ExactOp(17, 1)
    real = _native.exact_descriptors
    for bad in (4, 15, 4 | 16):
        def patched(kernels, bad=bad):
            kinds, params, cols, nder = real(kernels)
            kinds = kinds.copy()
            kinds[0] = bad
            return kinds, params, cols, nder
        _native.exact_descriptors = patched
        try:
            try:
                op.set(np.vstack(Xs), lens, fk.kernels, fk.coreg_mats(), fk.noise)
            except ValueError as e:
                assert 'unknown kernel kind' in str(e), str(e)
            else:
                raise AssertionError('kind %d accepted' % bad)
        finally:
            _native.exact_descriptors = real
    op.set(np.vstack(Xs), lens, fk.kernels, fk.coreg_mats(), fk.noise)
    op.factor()


# --- 5. the model ---------------------------------------------------------------------------------
GRID = 640


@functools.lru_cache(maxsize=None)
def _model_case():
    c = Case('lmc_small')
    A, kap = list(c.coreg_vecs[:2]), list(c.coreg_diags[:2])
    spec = KernelSpec(c.D, [Matern52Spec(1.5), RBFSpec(2.0)], A, kap, c.noise)
    spec.set_input_dim(1)
    Xtr = [np.asarray(v).reshape(len(v), 1) for v in c.Xs]
    rng = np.random.RandomState(9)
    Xt = [np.sort(rng.rand(4 + d, 1), axis=0) * 0.9 + 0.05 for d in range(c.D)]
    return c, A, kap, spec, Xtr, Xt


def _model(prediction='on-the-fly', metrics=False, variance_batch=None):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    c, A, kap, _, Xtr, _ = _model_case()
    fk = FunctionalKernel(D=c.D, lmc_kernels=[Matern52(1.5), RBF(2.0)],
                          lmc_ranks=[len(a) for a in A])
    fk.coreg_vecs = A
    fk.coreg_diags = kap
    fk.noise = c.noise
    np.random.seed(5)
    return InterpolatedLLGP(Xtr, c.Ys, normalize=False, m=[GRID], functional_kernel=fk,
                            prediction=prediction, metrics=metrics, trace_iterations=len(c.rs),
                            tolerance=1e-4, variance_batch=variance_batch)


def check_model_metrics():
    model = _model(metrics=True)
    model.parameters_changed()
    got = model.metrics.grad_error
    assert len(got) == 1 and np.isfinite(got[0]), got
    assert np.all(np.isfinite(model.gradient))
    (W, _), = model.interpolants.values()
    assert W.shape[1] >= 600 * model.output_dim


def check_model_exact_prediction():
    c, _, _, spec, Xtr, Xt = _model_case()
    model = _model(prediction='exact')
    _, var = model.predict(Xt)
    Kx = es._cross_dense(spec, Xt, Xtr, c.D)
    Kd = es._cross_dense(spec, Xtr, Xtr, c.D) + np.diag(np.repeat(c.noise, c.lens))
    native = _native_variance()
    ref = np.clip(native - np.einsum('ij,ji->i', Kx, la.solve(Kd, Kx.T)), 0, None)
    np.testing.assert_allclose(np.concatenate(var), ref, rtol=0, atol=1e-8 * native.max())
    es._close(model.K(), Kd, 1e-12, 'K()')


def _native_variance():
    c, A, kap, spec, _, Xt = _model_case()
    coreg = np.column_stack([np.square(a).sum(axis=0) for a in A]) + np.column_stack(kap)
    k0 = np.array([float(k.from_dist(0.0)) for k in spec._kernels])
    return np.repeat(coreg @ k0 + c.noise, [len(v) for v in Xt])


def check_model_tiled_variances():
    """variance_batch=16 (rows filled on the device by k_ex_cross_rows) against the host-assembled
    right-hand sides, at predict_suite's tolerance."""
    _, _, _, _, _, Xt = _model_case()
    mu0, var0 = _model().predict(Xt)
    mu1, var1 = _model(variance_batch=16).predict(Xt)
    native = _native_variance()
    atol = 1e-5 * max(native.max(), 1.0)
    err = np.abs(np.concatenate(var1) - np.concatenate(var0)).max()
    print('tiled against host-assembled variances: max difference %.3e (atol %.3e)' % (err, atol))
    np.testing.assert_allclose(np.concatenate(var1), np.concatenate(var0), rtol=0, atol=atol)
    np.testing.assert_array_equal(np.concatenate(mu1), np.concatenate(mu0))


def check_model_solve():
    """Iterative.solve on the model's operator, on whichever path K.preconditioner picks: the
    reference's residual rule on the explicit residual, and alpha against the host's dense solve
    of the oracle's K~ at that path's bar (check_direct_solve: 1e-9 where the factorisation is
    K~^-1; check_precond_hi: 1e-8 where it is a preconditioner; the Krylov solve alone: the
    explicit residual over the smallest eigenvalue's bound, the smallest noise)."""
    from runlmc_amd.approx.iterative import Iterative
    c, _, _, spec, _, _ = _model_case()
    model = _model()
    model._ensure()
    K = model._K
    (ad, (W, WT)), = model.interpolants.items()
    assert W.shape[1] >= 600 * c.D
    op = olik.LMCOperatorOracle(spec, model.dists[ad], W, WT, c.lens)
    Kd = ps._dense_spd(op, c.n)
    xref = la.solve(Kd, c.y, assume_a='pos')
    x, _, res = Iterative.solve(K, c.y, verbose=True)
    assert res < 1e-4 and np.linalg.norm(c.y - Kd @ x) < 1e-4, (res, np.linalg.norm(c.y - Kd @ x))
    M = K.preconditioner
    if M is None:
        bound = np.linalg.norm(c.y - Kd @ x) / c.noise.min()
        assert np.abs(x - xref).max() <= bound
        return 'krylov'
    bar = 1e-9 if M.exact else 1e-8
    x, _, res = Iterative.solve(K, c.y, verbose=True, tol=bar)
    assert res < bar, res
    _close(x, xref, rel=bar)
    return 'exact' if M.exact else 'preconditioner'
