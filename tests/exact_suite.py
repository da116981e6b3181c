"""Checks of the exact dense likelihood (runlmc_amd.lmc.ExactLMCLikelihood, include/runlmc_hip.h
rl_exact_*) shared by the CPU run on the emulator (tests/test_exact_emu.py) and the GPU run
(tests/test_exact_gpu.py).  Every function uses whichever native library is active.

Yardsticks: the reference's own ExactLMCLikelihood output (golden exact_small.npz), the oracle's
dense twin (oracle.likelihood.exact_kernel_dense / exact_gradients, 1-D inputs), dense K and dK
built here in NumPy over each kernel's active columns (2-D and split inputs, through
oracle.likelihood.exact_gradients_from_dense), and SciPy's Cholesky for factor and solves."""
import os

import numpy as np
import scipy.linalg as la
import torch

from oracle import likelihood as olik
from oracle.kernels import KernelSpec, RBFSpec, Matern32Spec, StdPeriodicSpec, ScaledSpec
from cases import Case, GOLDEN

from runlmc_amd._native import ExactOp
from runlmc_amd.kern.stationary import RBF, Matern32, StdPeriodic, Scaled
from runlmc_amd.lmc import ExactLMCLikelihood
from runlmc_amd.lmc.functional_kernel import FunctionalKernel


def _pkg_kernel(desc):
    parts = str(desc).split(';')
    kind, vals = parts[0], [float(v) for v in parts[1:]]
    if kind == 'scaled_rbf':
        return Scaled(RBF(vals[0]), vals[1])
    return {'rbf': RBF, 'matern': Matern32, 'periodic': StdPeriodic}[kind](*vals)


def _fk(D, kerns, A, kappa, noise, P=1, num_lmc=None, num_slfm=0):
    """FunctionalKernel with given parameters: LMC kernels, then SLFM (reference order)."""
    a = len(kerns) - num_slfm if num_lmc is None else num_lmc
    fk = FunctionalKernel(D=D, lmc_kernels=kerns[:a], lmc_ranks=[len(v) for v in A[:a]],
                          slfm_kernels=kerns[a:a + num_slfm], indep_gp=kerns[a + num_slfm:])
    fk.coreg_vecs = A
    fk.coreg_diags = kappa
    fk.noise = noise
    fk.set_input_dim(P)
    return fk


def _grads_flat(lik, Q):
    return ([np.asarray(g) for g in lik.coreg_vec_gradients()],
            [np.asarray(g) for g in lik.coreg_diags_gradients()],
            [np.asarray(g, dtype=float) for g in lik.kernel_gradients()],
            np.asarray(lik.noise_gradient()))


def _close(got, ref, rtol, what=''):
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    scale = max(np.abs(ref).max(), 1e-300)
    err = np.abs(got - ref).max() / scale
    assert err <= rtol, '%s: relative error %.3e > %.1e' % (what, err, rtol)


def _compare_to_oracle(lik, ref, alpha, K, Q, rtol, K_rtol=1e-12, with_K=True):
    if with_K:
        _close(lik.K, K, K_rtol, 'K')
    _close(lik.alpha(), alpha, rtol, 'alpha')
    vec, diag, kern, noise = _grads_flat(lik, Q)
    for q in range(Q):
        _close(vec[q], ref['coreg_vec'][q], rtol, 'coreg_vec %d' % q)
        _close(diag[q], ref['coreg_diag'][q], rtol, 'coreg_diag %d' % q)
        _close(kern[q], ref['kernel'][q], rtol, 'kernel %d' % q)
    _close(noise, ref['noise'], rtol, 'noise')


# --- the reference's own output ------------------------------------------------------------
def golden_small():
    g = np.load(os.path.join(GOLDEN, 'exact_small.npz'))
    D, Q = int(g['D']), int(g['Q'])
    kerns = []
    for d in g['kdesc']:
        parts = str(d).split(';')
        kerns.append(_pkg_kernel(parts[0] + ';' + ';'.join(parts[1:])))
    fk = _fk(D, kerns, [g['A%d' % q] for q in range(Q)], [g['kappa%d' % q] for q in range(Q)],
             g['noise'])
    Xs = [g['X%d' % d] for d in range(D)]
    Ys = np.split(g['y'], np.cumsum(g['lens'])[:-1])
    return g, fk, Xs, Ys


def check_golden_small():
    g, fk, Xs, Ys = golden_small()
    lik = ExactLMCLikelihood(fk, Xs, Ys)
    Q = int(g['Q'])
    ref = dict(coreg_vec=[g['grad_A%d' % q] for q in range(Q)],
               coreg_diag=[g['grad_kappa%d' % q] for q in range(Q)],
               kernel=[g['grad_kern%d' % q] for q in range(Q)], noise=g['grad_noise'])
    _compare_to_oracle(lik, ref, g['alpha'], g['K'], Q, rtol=1e-9, K_rtol=1e-13)
    sign, ld = np.linalg.slogdet(g['K'])
    assert sign > 0
    assert abs(lik.log_det_K() - ld) <= 1e-10 * abs(ld), (lik.log_det_K(), ld)
    nq = g['y'].dot(la.solve(g['K'], g['y']))
    ll = -0.5 * (ld + nq + len(g['y']) * np.log(2 * np.pi))
    assert abs(lik.log_likelihood() - ll) <= 1e-9 * abs(ll)
    # the same likelihood feeds the functional kernel's gradient sink
    fk.update_gradient(lik)
    _close(fk.noise_grad, g['grad_noise'], 1e-9)
    for q in range(Q):
        _close(fk.coreg_vec_grads[q], g['grad_A%d' % q], 1e-9)
        _close(fk.kernels[q].gradient, g['grad_kern%d' % q], 1e-9)


def check_deterministic():
    """Two gradient calls (and two handles) give the same bits."""
    g, fk, Xs, Ys = golden_small()
    a = ExactLMCLikelihood(fk, Xs, Ys)
    b = ExactLMCLikelihood(fk, Xs, Ys)
    S1, n1 = a._op.grad_sums(a._alpha_dev)
    S2, n2 = a._op.grad_sums(a._alpha_dev)
    assert np.array_equal(S1, S2) and np.array_equal(n1, n2)
    for x, y in zip(_grads_flat(a, fk.Q), _grads_flat(b, fk.Q)):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)
    assert a.log_det_K() == b.log_det_K()
    assert np.array_equal(a.alpha(), b.alpha())


# --- tile edges against the oracle's dense twin and SciPy ---------------------------------------
_SIZES_KINDS = (['rbf;2.0', 'matern;1.5', 'periodic;1.0;0.7', 'scaled_rbf;3.0;1.7'])


def random_model(n, D, seed, kdesc=_SIZES_KINDS, rank=1):
    rng = np.random.RandomState(seed)
    lens = np.full(D, n // D)
    lens[:n - lens.sum()] += 1
    Xs = [np.sort(rng.rand(int(l))) for l in lens]
    Q = len(kdesc)
    A = [rng.randn(rank, D) * 0.6 for _ in range(Q)]
    kappa = [np.abs(rng.randn(D)) * 0.3 + 0.05 for _ in range(Q)]
    noise = 0.05 + 0.1 * rng.rand(D)
    y = rng.randn(n)
    return Xs, y, kdesc, A, kappa, noise, [int(l) for l in lens]


def _oracle_kernel(desc):
    parts = str(desc).split(';')
    kind, vals = parts[0], [float(v) for v in parts[1:]]
    if kind == 'scaled_rbf':
        return ScaledSpec(RBFSpec(vals[0]), vals[1])
    return {'rbf': RBFSpec, 'matern': Matern32Spec, 'periodic': StdPeriodicSpec}[kind](*vals)


def check_tile_edges(n, D, rtol=1e-9):
    Xs, y, kdesc, A, kappa, noise, lens = random_model(n, D, seed=n * 7 + D)
    Q = len(kdesc)
    fk = _fk(D, [_pkg_kernel(k) for k in kdesc], A, kappa, noise)
    spec = KernelSpec(D, [_oracle_kernel(k) for k in kdesc], A, kappa, noise)
    spec.set_input_dim(1)
    ref, alpha, K = olik.exact_gradients(spec, Xs, y)
    Ys = np.split(y, np.cumsum(lens)[:-1])
    lik = ExactLMCLikelihood(fk, Xs, Ys)
    c = la.cho_factor(K, lower=True)
    _close(lik.log_det_K(), 2 * np.log(np.diag(c[0])).sum(), 1e-11, 'log det')
    # factor and solves of the handle itself against SciPy
    op = ExactOp(n, 1)
    op.set(np.concatenate(Xs)[:, None], lens, fk.kernels, fk.coreg_mats(), noise)
    op.factor()
    rng = np.random.RandomState(1)
    B = rng.randn(3, n)
    _close(op.solve(B).cpu().numpy(), la.cho_solve(c, B.T).T, rtol, 'solve')
    Xt = [np.sort(rng.rand(3 + d)) for d in range(D)]
    Kx = _cross_dense(spec, [x[:, None] for x in Xt], [x[:, None] for x in Xs], D)
    _close(op.cross(np.concatenate(Xt)[:, None], [len(x) for x in Xt]), Kx, 1e-12, 'cross')
    ev = np.einsum('ij,ji->i', Kx, la.cho_solve(c, Kx.T))
    _close(op.explained_variance(np.concatenate(Xt)[:, None], [len(x) for x in Xt]), ev, rtol,
           'explained variance')
    op.invert()
    _compare_to_oracle(lik, ref, alpha, K, Q, rtol)
    # the static cross-covariance
    _close(ExactLMCLikelihood.kernel_from_indices(Xt, Xs, fk), Kx, 1e-12, 'kernel_from_indices')


def _cross_dense(spec, Xa, Xb, D, kernels=None):
    """K(Xa, Xb) of a KernelSpec, each kernel over its own active columns (default: all)."""
    rl, cl = [len(x) for x in Xa], [len(x) for x in Xb]
    a, b = np.vstack(Xa), np.vstack(Xb)
    ro, co = np.repeat(np.arange(D), rl), np.repeat(np.arange(D), cl)
    K = np.zeros((len(a), len(b)))
    ads = kernels or [None] * len(spec._kernels)
    for B, k, ad in zip(spec.coreg_mats(), spec._kernels, ads):
        cols = list(range(a.shape[1])) if ad is None else list(ad)
        dist = np.sqrt(np.square(a[:, None, cols] - b[None, :, cols]).sum(axis=-1))
        K += B[np.ix_(ro, co)] * k.from_dist(dist)
    return K


def _dense_gradients(spec, Xs, y, D, ads):
    """K and every dK of the reference's loops (likelihood.py:48-96) built densely, each kernel
    over its own active columns, through oracle.likelihood.exact_gradients_from_dense."""
    lens = [len(x) for x in Xs]
    X = np.vstack(Xs)
    o = np.repeat(np.arange(D), lens)
    K = _cross_dense(spec, Xs, Xs, D, ads) + np.diag(np.repeat(spec.noise, lens))
    dKs, where = [], []
    for q, (a_q, B, k, ad) in enumerate(zip(spec.coreg_vecs, spec.coreg_mats(), spec._kernels, ads)):
        cols = list(ad)
        dist = np.sqrt(np.square(X[:, None, cols] - X[None, :, cols]).sum(axis=-1))
        Kq = k.from_dist(dist)
        for i, ai in enumerate(np.atleast_2d(a_q)):
            for j in range(D):
                dB = np.zeros((D, D))
                dB[j] += ai
                dB.T[j] += ai
                dKs.append(dB[np.ix_(o, o)] * Kq)
                where.append(('vec', q, (i, j)))
        for i in range(D):
            dB = np.zeros((D, D))
            dB[i, i] = 1
            dKs.append(dB[np.ix_(o, o)] * Kq)
            where.append(('diag', q, i))
        for p, dk in enumerate(k.kernel_gradient(dist)):
            dKs.append(B[np.ix_(o, o)] * dk)
            where.append(('kern', q, p))
    for d in range(D):
        dKs.append(np.diag((o == d).astype(float)))
        where.append(('noise', None, d))
    vals = olik.exact_gradients_from_dense(K, y, dKs)
    ref = dict(coreg_vec=[np.zeros(np.shape(a)) for a in spec.coreg_vecs],
               coreg_diag=[np.zeros(D) for _ in spec.coreg_vecs],
               kernel=[np.zeros(len(k.kernel_gradient(np.zeros(1)))) for k in spec._kernels],
               noise=np.zeros(D))
    for v, (kind, q, idx) in zip(vals, where):
        if kind == 'vec':
            ref['coreg_vec'][q][idx] = v
        elif kind == 'diag':
            ref['coreg_diag'][q][idx] = v
        elif kind == 'kern':
            ref['kernel'][q][idx] = v
        else:
            ref['noise'][idx] = v
    return ref, la.solve(K, y), K


def check_2d():
    c = Case('lmc_2d')
    spec = c.spec()
    fk = _fk(c.D, [_pkg_kernel(k) for k in c.kdesc], c.coreg_vecs, c.coreg_diags, c.noise, P=2)
    Xs = [np.asarray(x).reshape(len(x), 2) for x in c.Xs]
    ref, alpha, K = _dense_gradients(spec, Xs, c.y, c.D, [(0, 1)] * c.Q)
    lik = ExactLMCLikelihood(fk, Xs, c.Ys)
    _compare_to_oracle(lik, ref, alpha, K, c.Q, rtol=1e-9)


def split_model():
    g = np.load(os.path.join(GOLDEN, 'lmc_split.npz'))
    D, Q = int(g['D']), int(g['Q'])
    kerns, okerns, ads = [], [], []
    for desc, ad in zip(g['kdesc'], g['kad']):
        k = _pkg_kernel(desc)
        k.active_dims = [int(ad)]
        kerns.append(k)
        okerns.append(_oracle_kernel(desc))
        ads.append((int(ad),))
    A = [g['A%d' % q] for q in range(Q)]
    kappa = [g['kappa%d' % q] for q in range(Q)]
    fk = _fk(D, kerns, A, kappa, g['noise'], P=2)
    spec = KernelSpec(D, okerns, A, kappa, g['noise'])
    Xs = [g['X0'], g['X1']]
    return g, fk, spec, Xs, ads


def check_split():
    g, fk, spec, Xs, ads = split_model()
    D, Q = int(g['D']), int(g['Q'])
    ref, alpha, K = _dense_gradients(spec, Xs, g['y'], D, ads)
    Ys = np.split(g['y'], np.cumsum(g['lens'])[:-1])
    lik = ExactLMCLikelihood(fk, Xs, Ys)
    _compare_to_oracle(lik, ref, alpha, K, Q, rtol=1e-9)


def check_not_positive_definite():
    """Duplicate points (a singular kernel matrix) with a slightly negative noise, so that the
    pivot of the duplicate's column is clearly negative whatever the rounding: LinAlgError
    naming the column; the same handle then factors a valid input."""
    X = np.array([0.1, 0.4, 0.4, 0.7, 0.9])
    fk = _fk(1, [RBF(2.0)], [np.array([[1.0]])], [np.array([0.0])], np.array([0.0]))
    op = ExactOp(5, 1)
    op.set(X[:, None], [5], fk.kernels, fk.coreg_mats(), np.array([-0.01]))
    try:
        op.factor()
    except np.linalg.LinAlgError as e:
        assert 'column 2' in str(e), str(e)
    else:
        raise AssertionError('no LinAlgError')
    fk.noise = np.array([-0.01])
    try:
        ExactLMCLikelihood(fk, [X], [np.ones(5)])
    except np.linalg.LinAlgError as e:
        assert 'column' in str(e)
    else:
        raise AssertionError('no LinAlgError')
    op.set(X[:, None], [5], fk.kernels, fk.coreg_mats(), np.array([0.1]))
    ld = op.factor()
    K = fk.coreg_mats()[0][0, 0] * np.exp(-0.5 * 2.0 * (X[:, None] - X[None, :]) ** 2) + 0.1 * np.eye(5)
    assert abs(ld - np.linalg.slogdet(K)[1]) < 1e-12 * abs(np.linalg.slogdet(K)[1]) + 1e-13
    _close(op.solve(np.arange(5.0)).cpu().numpy(), la.solve(K, np.arange(5.0)), 1e-10)


def check_errors():
    class Odd(RBF):
        pass

    fk = _fk(1, [Odd(1.0)], [np.array([[1.0]])], [np.array([1.0])], np.array([0.1]))
    try:
        ExactLMCLikelihood(fk, [np.linspace(0, 1, 4)], [np.ones(4)])
    except NotImplementedError as e:
        assert 'Odd' in str(e)
    else:
        raise AssertionError('no NotImplementedError')
    fk = _fk(2, [RBF(1.0)], [np.ones((1, 2))], [np.ones(2)], np.array([0.1, 0.1]))
    op = ExactOp(6, 1)
    bad = [
        lambda: op.set(np.zeros((5, 1)), [3, 3], fk.kernels, fk.coreg_mats(), [0.1, 0.1]),
        lambda: op.set(np.zeros((6, 2)), [3, 3], fk.kernels, fk.coreg_mats(), [0.1, 0.1]),
        lambda: op.set(np.zeros((6, 1)), [3, 3], fk.kernels, fk.coreg_mats(), [0.1]),
        lambda: op.set(np.zeros((6, 1)), [3, 3], fk.kernels, [np.eye(3)], [0.1, 0.1]),
        lambda: op.set(np.zeros((6, 1)), [4, 3], fk.kernels, fk.coreg_mats(), [0.1, 0.1]),
        lambda: ExactOp(0, 1),
    ]
    for f in bad:
        try:
            f()
        except ValueError:
            pass
        else:
            raise AssertionError('no ValueError')
    op.set(np.linspace(0, 1, 6)[:, None], [3, 3], fk.kernels, fk.coreg_mats(), [0.1, 0.1])
    try:
        op.solve(np.ones(6))        # not factored yet
    except ValueError:
        pass
    else:
        raise AssertionError('solve before factor')
    try:
        op.solve(np.ones(5))
    except ValueError:
        pass
    else:
        raise AssertionError('bad right-hand side')
    # beyond the documented limits: NotImplementedError (RL_ELIMIT)
    many = [RBF(1.0 + q) for q in range(33)]
    fk2 = _fk(1, many, [np.ones((1, 1))] * 33, [np.ones(1)] * 33, np.array([0.1]))
    op2 = ExactOp(4, 1)
    try:
        op2.set(np.zeros((4, 1)), [4], fk2.kernels, fk2.coreg_mats(), [0.1])
    except NotImplementedError:
        pass
    else:
        raise AssertionError('no limit error')


# --- the model ------------------------------------------------------------------------------
def _model(c, prediction='on-the-fly', metrics=False):
    import parity_suite as ps
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    fk = ps.functional_kernel_for(c)
    Xs = [np.asarray(x).reshape(len(x), c.P) for x in c.Xs]
    m = [len(a) - 4 for a in c.grid_axes]
    return InterpolatedLLGP(Xs, c.Ys, normalize=False, m=m, functional_kernel=fk,
                            prediction=prediction, metrics=metrics, trace_iterations=len(c.rs),
                            tolerance=1e-4)


def check_model_exact_prediction(name):
    c = Case(name)
    spec = c.spec()
    rng = np.random.RandomState(9)
    Xt = [np.sort(rng.rand(4 + d, c.P), axis=0) * 0.9 + 0.05 for d in range(c.D)]
    np.random.seed(5)
    fly = _model(c)
    mu_f, _ = fly.predict(Xt)
    np.random.seed(5)
    ex = _model(c, prediction='exact')
    mu_e, var_e = ex.predict(Xt)
    np.testing.assert_array_equal(np.concatenate(mu_e), np.concatenate(mu_f))
    Xtr = [np.asarray(x).reshape(len(x), c.P) for x in c.Xs]
    Kx = _cross_dense(spec, Xt, Xtr, c.D)
    Kd = _cross_dense(spec, Xtr, Xtr, c.D) + np.diag(np.repeat(c.noise, c.lens))
    coreg = np.column_stack([np.square(a).sum(axis=0) for a in c.coreg_vecs]) + \
        np.column_stack(c.coreg_diags)
    k0 = np.array([float(k.from_dist(0.0)) for k in spec._kernels])
    native = np.repeat(coreg @ k0 + c.noise, [len(x) for x in Xt])
    ref = np.clip(native - np.einsum('ij,ji->i', Kx, la.solve(Kd, Kx.T)), 0, None)
    np.testing.assert_allclose(np.concatenate(var_e), ref, rtol=0, atol=1e-8 * native.max())
    # K() is the exact dense kernel
    _close(ex.K(), Kd, 1e-12, 'K()')


def check_model_metrics(name='lmc_small'):
    c = Case(name)
    np.random.seed(3)
    model = _model(c, metrics=True)
    fk = model._functional_kernel
    errs = []
    for step in range(2):
        if step:
            fk.noise = fk.noise * 1.1
        model.parameters_changed()
        spec = KernelSpec(c.D, c.spec()._kernels, fk.coreg_vecs, fk.coreg_diags, fk.noise)
        spec.set_input_dim(1)
        ref = olik.exact_gradients(spec, c.Xs, c.y)[0]
        ge = np.concatenate((np.concatenate(ref['coreg_vec']).reshape(-1),
                             np.concatenate(ref['coreg_diag']),
                             np.concatenate([np.asarray(k, float) for k in ref['kernel']]),
                             ref['noise']))
        lk = model.kernel
        ga = np.concatenate((np.concatenate(lk.coreg_vec_gradients()).reshape(-1),
                             np.concatenate(lk.coreg_diags_gradients()),
                             np.concatenate(lk.kernel_gradients()), lk.noise_gradient()))
        errs.append(np.abs(ga - ge).max() / np.abs(ge).max())
    got = model.metrics.grad_error
    assert len(got) == 2 and np.all(np.isfinite(got)), got
    np.testing.assert_allclose(got, errs, rtol=1e-7)


def check_model_metrics_declined():
    """metrics=True keeps working when the exact path declines (here: a kernel class it has no
    device formula for): NaN entries and one warning, no exception."""
    c = Case('lmc_small')
    np.random.seed(3)
    model = _model(c, metrics=True)
    k0 = model._functional_kernel._kernels[0]
    k0.__class__ = type('Unlisted', (type(k0),), {})
    model.parameters_changed()
    model.parameters_changed()
    assert len(model.metrics.grad_error) == 2 and np.all(np.isnan(model.metrics.grad_error))
    assert np.all(np.isfinite(model.gradient))
