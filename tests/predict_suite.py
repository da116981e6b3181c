"""Checks of the tiled predictive variances (InterpolatedLLGP(variance_batch=...),
runlmc_amd.approx.quadforms, include/runlmc_hip.h rl_exact_cross_dev / rl_row_dots) shared by
the CPU run on the emulator (tests/test_predict_emu.py) and the GPU run
(tests/test_predict_gpu.py).  Every function uses whichever native library is active.

Yardsticks: the existing ExactOp.cross (rl_exact_cross_host, pinned to the oracle by
exact_suite) for the cross-covariance rows, NumPy for the reduction, and for the model the dense
oracle formulas of parity_suite.check_model_prediction at its tolerance."""
import ctypes
import functools

import numpy as np
import torch

import exact_suite as es
import parity_suite as ps
from cases import Case

from runlmc_amd import _lib
from runlmc_amd._native import ExactOp, row_dots

CROSS_N = (1, 17, 64, 65, 129, 1000)
CROSS_NT = (1, 63, 64, 65, 130)
BATCHES = (1, 7, 10 ** 6)


def cross_atol(coreg_mats):
    """Rounding of a Q-term sum whose terms come from the same formulas in both kernels and may
    differ by contraction only: 8 Q 2^-53 sum_q max|B_q|."""
    B = np.asarray(coreg_mats, dtype=float)
    return 8 * len(B) * 2.0 ** -53 * sum(np.abs(b).max() for b in B)


def _windows(nt):
    """(row0, nrows): everything, windows that start and end inside a row group (groups hold at
    most 64 rows), the last row alone, nothing."""
    w = [(0, nt), (nt - 1, 1), (0, 0), (nt, 0)]
    if nt >= 3:
        w.append((nt // 3, nt - nt // 3 - nt // 4))
    if nt > 70:
        w.append((5, 66))
    return w


def _check_windows(op, Xt, tl, atol, what):
    ref = op.cross(Xt, tl)
    nt = ref.shape[0]
    worst = 0.0
    buf = torch.empty((max(nt, 1) * op.n + 3,), dtype=torch.float64, device=op.device)
    for row0, nrows in _windows(nt):
        for out in (None, buf):
            got = op.cross_device(Xt, tl, row0, nrows, out=out)
            assert isinstance(got, torch.Tensor) and got.device == op.device
            assert tuple(got.shape) == (nrows, op.n)
            got = got.cpu().numpy()
            if nrows:
                worst = max(worst, np.abs(got - ref[row0:row0 + nrows]).max())
            np.testing.assert_allclose(got, ref[row0:row0 + nrows], rtol=0, atol=atol,
                                       err_msg='%s rows %d + %d' % (what, row0, nrows))
    print('%s: max |cross_device - cross| = %.3e (atol %.3e)' % (what, worst, atol))


def check_cross_rows(n, nt, D):
    """All three kernel kinds and Scaled (exact_suite.random_model), 1-D inputs, D outputs; with
    D = 3 the middle output has no test rows (and at n < D some have no training rows)."""
    Xs, _, kdesc, A, kappa, noise, lens = es.random_model(n, D, seed=n * 11 + nt + D)
    fk = es._fk(D, [es._pkg_kernel(k) for k in kdesc], A, kappa, noise)
    op = ExactOp(n, 1)
    op.set(np.concatenate(Xs)[:, None], lens, fk.kernels, fk.coreg_mats(), noise)
    rng = np.random.RandomState(nt)
    tl = [nt] if D == 1 else [nt - nt // 2] + [0] * (D - 2) + [nt // 2]
    Xt = rng.rand(nt, 1) * 1.2 - 0.1
    _check_windows(op, Xt, tl, cross_atol(fk.coreg_mats()), 'n %d nt %d D %d' % (n, nt, D))


def check_cross_2d():
    """lmc_2d's kernels on two input columns."""
    c = Case('lmc_2d')
    fk = ps.functional_kernel_for(c)
    X = np.vstack([np.asarray(x).reshape(len(x), 2) for x in c.Xs])
    op = ExactOp(X.shape[0], 2)
    op.set(X, c.lens, fk.kernels, fk.coreg_mats(), c.noise)
    rng = np.random.RandomState(4)
    tl = [70 + d for d in range(c.D)]
    _check_windows(op, rng.rand(sum(tl), 2), tl, cross_atol(fk.coreg_mats()), 'lmc_2d')


def check_cross_split():
    """lmc_split: kernels on different active columns of 2-D inputs."""
    g, fk, _, Xs, _ = es.split_model()
    X = np.vstack(Xs)
    op = ExactOp(X.shape[0], 2)
    op.set(X, [len(x) for x in Xs], fk.kernels, fk.coreg_mats(), g['noise'])
    rng = np.random.RandomState(5)
    tl = [66, 3]
    _check_windows(op, rng.rand(sum(tl), 2), tl, cross_atol(fk.coreg_mats()), 'lmc_split')


def check_row_dots():
    """The fused reduction against NumPy at 1e-14 sum |b_j x_j| (and 1e-14 sum x_j^2 for the
    squared norm), bit-identical on a second call."""
    lib = _lib.get_library()
    dev = lib.torch_device(0)
    rng = np.random.RandomState(8)
    for k, n in ((1, 1), (5, 63), (3, 64), (7, 1000), (70, 129), (2, 70001)):
        B, X = rng.randn(k, n), rng.randn(k, n)
        Bd, Xd = torch.from_numpy(B).to(dev), torch.from_numpy(X).to(dev)
        d1, s1 = [t.cpu().numpy() for t in row_dots(lib, Bd, Xd)]
        d2, s2 = [t.cpu().numpy() for t in row_dots(lib, Bd, Xd)]
        assert np.array_equal(d1, d2) and np.array_equal(s1, s2), (k, n)
        err_d = np.abs(d1 - (B * X).sum(axis=1))
        err_s = np.abs(s1 - (X * X).sum(axis=1))
        print('row_dots k %d n %d: dot error / sum|bx| %.2e, norm error / sum x^2 %.2e'
              % (k, n, (err_d / np.abs(B * X).sum(axis=1)).max(), (err_s / (X * X).sum(axis=1)).max()))
        assert np.all(err_d <= 1e-14 * np.abs(B * X).sum(axis=1)), (k, n)
        assert np.all(err_s <= 1e-14 * (X * X).sum(axis=1)), (k, n)


# --- the model ------------------------------------------------------------------------------
def _test_points(c_D, P):
    rng = np.random.RandomState(9)
    return [np.sort(rng.rand(4 + d, P), axis=0) * 0.9 + 0.05 for d in range(c_D)]


def _model(c, prediction, variance_batch=None):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    fk = ps.functional_kernel_for(c)
    Xs = [np.asarray(x).reshape(len(x), c.P) for x in c.Xs]
    m = [len(a) - 4 for a in c.grid_axes]
    np.random.seed(5)
    return InterpolatedLLGP(Xs, c.Ys, normalize=False, m=m, functional_kernel=fk,
                            prediction=prediction, trace_iterations=len(c.rs), tolerance=1e-4,
                            variance_batch=variance_batch)


@functools.lru_cache(maxsize=None)
def _references(name):
    """(test points, native variance, on-the-fly and precompute references): the dense-oracle
    formulas of parity_suite.check_model_prediction."""
    from runlmc_amd.approx.interpolation import multi_interpolant
    c = Case(name)
    spec, _, Kd, Kuu = ps._dense_pieces(c)
    Xt = _test_points(c.D, c.P)
    Wt = multi_interpolant(Xt, *c.grid_axes).toarray()
    coreg = np.column_stack([np.square(a).sum(axis=0) for a in c.coreg_vecs]) + \
        np.column_stack(c.coreg_diags)
    k0 = np.array([float(k.from_dist(0.0)) for k in spec._kernels])
    native = np.repeat(coreg @ k0 + c.noise, [len(x) for x in Xt])
    Kx = ps._exact_cross(spec, Xt, c.Xs, c.D)
    fly = np.clip(native - np.einsum('ij,ji->i', Kx, np.linalg.solve(Kd, Kx.T)), 0, None)
    nu = np.diag(Kuu @ (c.WT @ np.linalg.solve(Kd, c.W @ Kuu)))
    pre = np.clip(native - Wt @ nu, 0, None)
    return Xt, native, {'on-the-fly': fly, 'precompute': pre}


@functools.lru_cache(maxsize=None)
def _parent_means(name, mode):
    Xt = _references(name)[0]
    return np.concatenate(_model(Case(name), mode).predict(Xt)[0])


def check_model(name, mode, batch):
    c = Case(name)
    Xt, native, refs = _references(name)
    model = _model(c, mode, variance_batch=batch)
    mu, var = model.predict(Xt)
    assert [len(v) for v in var] == [len(x) for x in Xt]
    err = np.abs(np.concatenate(var) - refs[mode]).max()
    atol = 1e-5 * max(native.max(), 1.0)
    print('%s %s batch %d: max variance error %.3e (atol %.3e)' % (name, mode, batch, err, atol))
    np.testing.assert_allclose(np.concatenate(var), refs[mode], rtol=0, atol=atol)
    np.testing.assert_array_equal(np.concatenate(mu), _parent_means(name, mode))
    st = model.variance_stats
    rows = len(native) if mode == 'on-the-fly' else c.D * c.m
    assert all(len(a) == rows for a in st), [len(a) for a in st]
    assert np.all(st.residuals < model.variance_tolerance), st.residuals.max()
    # an empty request for one output, quantiles (as check_model_prediction)
    Xe = [Xt[0]] + [np.zeros((0, c.P))] * (c.D - 1)
    mu, var = model.predict(Xe)
    assert len(var[1]) == 0 and len(var[0]) == len(Xt[0])
    np.testing.assert_allclose(var[0], refs[mode][:len(Xt[0])], rtol=0, atol=atol)
    lo, hi = model.predict_quantiles(Xe)[0]
    assert np.all(lo <= mu[0]) and np.all(mu[0] <= hi)


def _split_model(prediction, variance_batch):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    g, fk, spec, Xs, ads = es.split_model()
    Ys = np.split(g['y'], np.cumsum(g['lens'])[:-1])
    np.random.seed(5)
    model = InterpolatedLLGP(Xs, Ys, normalize=False, m=[12, 14], functional_kernel=fk,
                             prediction=prediction, trace_iterations=4,
                             variance_batch=variance_batch)
    return model, g, spec, Xs, ads


def check_model_split(batch):
    """Split active dimensions: 'on-the-fly' against the dense K~ of the model's own grids and
    interpolants built from the oracle's kernels; 'precompute' raises as without the keyword."""
    model, g, spec, Xs, ads = _split_model('on-the-fly', batch)
    D = int(g['D'])
    lens = [len(x) for x in Xs]
    Kd = np.diag(np.repeat(np.asarray(g['noise'], dtype=float), lens))
    for ad in model.interpolants:
        W = model.interpolants[ad][0].toarray()
        (axis,) = model.grid_axes[ad]
        dist = np.abs(axis[:, None] - axis[None, :])
        Kuu = sum(np.kron(B, k.from_dist(dist))
                  for B, k, a in zip(spec.coreg_mats(), spec._kernels, ads) if a == ad)
        Kd += W @ Kuu @ W.T
    rng = np.random.RandomState(9)
    Xt = [rng.rand(5 + d, 2) * 0.9 + 0.05 for d in range(D)]
    Kx = es._cross_dense(spec, Xt, Xs, D, ads)
    coreg = np.column_stack([np.square(a).sum(axis=0) for a in spec.coreg_vecs]) + \
        np.column_stack(spec.coreg_diags)
    k0 = np.array([float(k.from_dist(0.0)) for k in spec._kernels])
    native = np.repeat(coreg @ k0 + g['noise'], [len(x) for x in Xt])
    ref = np.clip(native - np.einsum('ij,ji->i', Kx, np.linalg.solve(Kd, Kx.T)), 0, None)
    mu, var = model.predict(Xt)
    atol = 1e-5 * max(native.max(), 1.0)
    print('lmc_split batch %d: max variance error %.3e (atol %.3e)'
          % (batch, np.abs(np.concatenate(var) - ref).max(), atol))
    np.testing.assert_allclose(np.concatenate(var), ref, rtol=0, atol=atol)
    parent = _split_model('on-the-fly', None)[0]
    np.testing.assert_array_equal(np.concatenate(mu), np.concatenate(parent.predict(Xt)[0]))
    messages = []
    for vb in (None, batch):
        pre = _split_model('precompute', vb)[0]
        try:
            pre.predict(Xt)
        except ValueError as e:
            messages.append(str(e))
        else:
            raise AssertionError('precompute with split kernels did not raise')
    assert messages[0] == messages[1], messages


def check_host_path_not_taken(monkeypatch, name='lmc_small'):
    """With variance_batch set, neither the host cross-covariance, nor cdist, nor the host
    product with a Dm x Dm identity runs."""
    from runlmc_amd.models import interpolated_llgp as mod
    from runlmc_amd.lmc import grid_kernel

    def refuse(*a, **k):
        raise AssertionError('the host path ran')

    monkeypatch.setattr(mod.InterpolatedLLGP, '_exact_cross_kernel', refuse)
    monkeypatch.setattr(mod.sdist, 'cdist', refuse)
    monkeypatch.setattr(grid_kernel._GridKUU, 'matmat', refuse)
    c = Case(name)
    Xt, native, refs = _references(name)
    for mode in ('on-the-fly', 'precompute'):
        var = _model(c, mode, variance_batch=5).predict(Xt)[1]
        np.testing.assert_allclose(np.concatenate(var), refs[mode], rtol=0,
                                   atol=1e-5 * max(native.max(), 1.0))
    # (the guards do stop the host path)
    for mode in ('on-the-fly', 'precompute'):
        try:
            _model(c, mode).predict(Xt)
        except AssertionError:
            pass
        else:
            raise AssertionError('the guards did not catch the host path of %s' % mode)


def _raises(exc, f):
    try:
        f()
    except exc:
        return
    raise AssertionError('no %s' % exc.__name__)


def check_errors():
    c = Case('lmc_small')
    for bad in (0, -3, 2.5, True, '7'):
        _raises(ValueError, lambda: _model(c, 'on-the-fly', variance_batch=bad))
    assert _model(c, 'exact', variance_batch=3).variance_batch == 3
    # a kernel without a device formula: exact_descriptors' NotImplementedError, no host fallback
    model = _model(c, 'on-the-fly', variance_batch=4)
    k0 = model._functional_kernel._kernels[0]
    k0.__class__ = type('Unlisted', (type(k0),), {})
    _raises(NotImplementedError, lambda: model.predict(_test_points(c.D, c.P)))
    # the C entry points
    lib = _lib.get_library()
    fk = es._fk(2, [es._pkg_kernel('rbf;2.0')], [np.ones((1, 2))], [np.ones(2)], np.array([0.1, 0.1]))
    op = ExactOp(6, 1)
    Xt = np.linspace(0, 1, 5)[:, None]
    _raises(ValueError, lambda: op.cross_device(Xt, [2, 3], 0, 5))         # no rl_exact_set
    op.set(np.linspace(0, 1, 6)[:, None], [3, 3], fk.kernels, fk.coreg_mats(), [0.1, 0.1])
    assert tuple(op.cross_device(Xt, [2, 3], 0, 5).shape) == (5, 6)
    for row0, nrows in ((0, 6), (3, 3), (5, 1), (-1, 2), (0, -1)):
        _raises(ValueError, lambda: op.cross_device(Xt, [2, 3], row0, nrows))
    _raises(ValueError, lambda: op.cross_device(Xt, [2, 3], 0, 5,
                                                out=torch.empty(29, dtype=torch.float64,
                                                                device=op.device)))
    out = torch.empty((5, 6), dtype=torch.float64, device=op.device)
    tl = np.array([2, 3], dtype=np.int32)
    f = lib.cdll.rl_exact_cross_dev
    good = [op._h, _lib.host_ptr(Xt), _lib.host_ptr(tl), 0, 5, _lib.dev_ptr(out), None]
    assert f(*good) == _lib.RL_OK
    for i in (0, 1, 2, 5):
        args = list(good)
        args[i] = None
        assert f(*args) == _lib.RL_EINVAL, i
        assert b'rl_exact_cross_dev' in lib.cdll.rl_last_error()
    B = torch.zeros((2, 6), dtype=torch.float64, device=op.device)
    ws = torch.zeros((2, 128), dtype=torch.float64, device=op.device)
    o = torch.zeros((2, 2), dtype=torch.float64, device=op.device)
    good = [_lib.dev_ptr(B), _lib.dev_ptr(B), 2, 6, _lib.dev_ptr(o[0]), _lib.dev_ptr(o[1]),
            _lib.dev_ptr(ws), None]
    f = lib.cdll.rl_row_dots
    assert f(*good) == _lib.RL_OK
    for i in (0, 1, 4, 5, 6):
        args = list(good)
        args[i] = None
        assert f(*args) == _lib.RL_EINVAL, i
    for i, v in ((2, -1), (3, 0)):
        args = list(good)
        args[i] = v
        assert f(*args) == _lib.RL_EINVAL, (i, v)
    args = list(good)
    args[2] = 70000
    assert f(*args) == _lib.RL_ELIMIT
    _raises(ValueError, lambda: row_dots(lib, B, B[:, :3]))


def check_engine_subset(name='lmc_small'):
    """The grid-column row source with an explicit index list returns those entries of nu, in
    the order asked; a miss of the residual rule is logged once, naming the solver that ran."""
    import logging
    from runlmc_amd.approx import quadforms as qf
    c = Case(name)
    model = _model(c, 'precompute', variance_batch=3)
    model.parameters_changed()
    (gk,) = model._grid_kernels.values()
    _, _, Kd, Kuu = ps._dense_pieces(c)
    nu = np.diag(Kuu @ (c.WT @ np.linalg.solve(Kd, c.W @ Kuu)))
    idx = np.random.RandomState(3).permutation(c.D * c.m)[:11]
    out = qf.quad_forms(model._K, qf.GridColumnRows(gk, idx), len(idx), 4, 1e-4)
    np.testing.assert_allclose(out.v, nu[idx], rtol=0, atol=1e-5 * max(np.abs(nu).max(), 1.0))
    assert np.all(out.residuals < 1e-4) and np.all(out.xnorm > 0)
    _raises(ValueError, lambda: qf.GridColumnRows(gk, [c.D * c.m]))
    _raises(ValueError, lambda: qf.quad_forms(model._K, qf.GridColumnRows(gk, idx), len(idx), 0, 1e-4))

    records = []

    class Keep(logging.Handler):
        def emit(self, record):
            records.append(record)

    handler = Keep(level=logging.CRITICAL)
    qf._LOG.addHandler(handler)
    try:
        qf.quad_forms(model._K, qf.GridColumnRows(gk, idx), len(idx), 4, 1e-300)
    finally:
        qf._LOG.removeHandler(handler)
    assert len(records) == 1, len(records)
    text = records[0].getMessage()
    assert qf._solver_name(model._K) in text and '%d of %d' % (len(idx), len(idx)) in text, text
