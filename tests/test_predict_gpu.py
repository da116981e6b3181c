"""GPU run of the tiled predictive variances (tests/predict_suite.py on librunlmc_hip.so) and its
checks at the sizes the other layers are tuned for: C2 (n = 20 000) against the dense oracle's
Cholesky, C5 (n = 10^6) against the residual rule, the host path on a few rows, and a bound on
the host memory a prediction may take."""
import tracemalloc

import numpy as np
import pytest
import scipy.linalg as la
import torch

import predict_suite as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    return lib


@pytest.mark.parametrize('n,nt,D', [(n, nt, D) for n in pr.CROSS_N for nt in pr.CROSS_NT
                                    for D in (1, 3)])
def test_cross_rows(n, nt, D):
    pr.check_cross_rows(n, nt, D)


def test_cross_rows_2d_inputs():
    pr.check_cross_2d()


def test_cross_rows_split_active_dims():
    pr.check_cross_split()


def test_row_dots():
    pr.check_row_dots()


@pytest.mark.parametrize('batch', pr.BATCHES)
@pytest.mark.parametrize('mode', ['on-the-fly', 'precompute'])
@pytest.mark.parametrize('name', ['lmc_small', 'lmc_2d'])
def test_model(name, mode, batch):
    pr.check_model(name, mode, batch)


@pytest.mark.parametrize('batch', pr.BATCHES)
def test_model_split_active_dims(batch):
    pr.check_model_split(batch)


def test_host_path_not_taken(monkeypatch):
    pr.check_host_path_not_taken(monkeypatch)


def test_errors():
    pr.check_errors()


def test_engine_index_list_and_log():
    pr.check_engine_subset()


def _synth_model(p, prediction, variance_batch):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    from runlmc_amd.util import synth
    np.random.seed(5)
    model = InterpolatedLLGP(p.Xs, p.Ys, normalize=False, functional_kernel=synth.functional_kernel(p),
                             prediction=prediction, variance_batch=variance_batch)
    model.parameters_changed()
    return model


def _seeded_points(p, per_output, seed):
    rng = np.random.RandomState(seed)
    return [rng.rand(per_output, 1) * 0.98 + 0.01 for _ in range(p.D)]


def test_c2_against_dense_oracle():
    """C2 (n = 20 000, Dm = 20 016): 300 on-the-fly variances (variance_batch = 128) and nu at
    64 grid indices against the oracle's dense K~ and LAPACK's Cholesky, built as
    test_gpu_full_size.py: test_c2_direct_solve_vs_dense_oracle builds them.  Every row's
    residual is below tol, and every value within tol ||x_ref||_2 (1 + 1e-6) of the dense one:
    |b^T K~^-1 (b - K~ x)| <= ||K~^-1 b|| ||r||, x_ref from the dense solve.  Then the whole
    'precompute' vector once, tiled: it agrees with the 64 entries within that bound taken twice
    (two solves that both meet the rule) and gives the model's variances through W_*."""
    from threadpoolctl import threadpool_limits
    import test_gpu_full_size as fs
    from oracle import likelihood as olik
    from runlmc_amd.approx import quadforms as qf
    from runlmc_amd.approx.interpolation import multi_interpolant
    from runlmc_amd.util import synth
    D, Q, R, m0, _ = synth.CONFIGS['c2']
    p = synth.make_problem(D, Q, R, m0)
    assert p.n == 20000 and p.m == m0 + 4          # (the grid: 5 000 points and two cells of margin a side)
    spec = fs._spec(p)
    oop = olik.LMCOperatorOracle(spec, p.grid_dists, p.W, p.WT, p.lens)
    Kd = fs._dense_from_oracle(oop, p.n)
    Xt = _seeded_points(p, 75, seed=77)
    Kx = pr.es._cross_dense(spec, Xt, p.Xs, p.D)                        # (300, n)
    idx = np.sort(np.random.RandomState(78).permutation(p.D * p.m)[:64])
    Bnu = np.empty((64, p.n))
    e = np.zeros(p.D * p.m)
    for r, i in enumerate(idx):
        e[i] = 1.0
        Bnu[r] = p.W @ oop.grid_matvec(e)
        e[i] = 0.0
    with threadpool_limits(limits=16):
        cf = la.cho_factor(Kd, overwrite_a=True)
        Xfly = la.cho_solve(cf, Kx.T).T
        Xnu = la.cho_solve(cf, Bnu.T).T
    del Kd, cf
    v_fly, n_fly = np.einsum('ij,ij->i', Kx, Xfly), np.linalg.norm(Xfly, axis=1)
    v_nu, n_nu = np.einsum('ij,ij->i', Bnu, Xnu), np.linalg.norm(Xnu, axis=1)

    model = _synth_model(p, 'on-the-fly', 128)
    tol = model.variance_tolerance
    mu, var = model.predict(Xt)
    st = model.variance_stats
    assert len(st.v) == 300 and np.all(st.residuals < tol), st.residuals.max()
    err = np.abs(st.v - v_fly)
    print('C2 on-the-fly: max error %.3e, smallest bound %.3e, iterations <= %d'
          % (err.max(), (tol * n_fly).min(), st.iterations.max()))
    assert np.all(err <= tol * n_fly * (1 + 1e-6)), (err / (tol * n_fly)).max()
    native = np.repeat(model._native_variance(), [len(x) for x in Xt])
    np.testing.assert_array_equal(np.concatenate(var), np.clip(native - st.v, 0, None))

    pre = _synth_model(p, 'precompute', 128)
    (gk,) = pre._grid_kernels.values()
    sub = qf.quad_forms(pre._K, qf.GridColumnRows(gk, idx), 64, 128, tol)
    assert np.all(sub.residuals < tol), sub.residuals.max()
    err = np.abs(sub.v - v_nu)
    print('C2 nu at 64 indices: max error %.3e, smallest bound %.3e' % (err.max(), (tol * n_nu).min()))
    assert np.all(err <= tol * n_nu * (1 + 1e-6)), (err / (tol * n_nu)).max()
    mu, var = pre.predict(Xt)
    full = pre.variance_stats
    assert len(full.v) == p.D * p.m and np.all(full.residuals < tol), full.residuals.max()
    assert np.all(np.abs(full.v[idx] - sub.v) <= 2 * tol * np.maximum(full.xnorm[idx], sub.xnorm))
    Wt = multi_interpolant(Xt, p.grid)
    np.testing.assert_array_equal(np.concatenate(var), np.clip(native - Wt.dot(full.v), 0, None))


def test_c5_training_size():
    """C5, rbf family (the direct path), n = 10^6: 512 on-the-fly variances, 128 rows per tile.
    Every row meets the residual rule; the first 8 agree with a variance_batch=None model (whose
    8 x 10^6 host array is 64 MB) within 2 tol max ||x||_2 -- both solves meet the same rule, so
    this is the bound |b^T K~^-1 r| <= ||K~^-1 b|| ||r|| applied twice; and the tracemalloc peak of
    the tiled call stays below one eighth of the 8 n_test n bytes ONE host array of right-hand
    sides would take (the tiled path's host arrays are O(n_test P + batch) plus O(n) vectors)."""
    from runlmc_amd.util import synth
    D, Q, R, m0, _ = synth.CONFIGS['c5']
    p = synth.make_problem(D, Q, R, m0)
    assert p.n == 10 ** 6
    rng = np.random.RandomState(79)
    counts = np.bincount(rng.randint(0, p.D, 512 - 8), minlength=p.D)
    counts[0] += 8                                   # (the first 8 rows: output 0)
    Xt = [rng.rand(int(c), 1) * 0.98 + 0.01 for c in counts]
    model = _synth_model(p, 'on-the-fly', 128)
    assert model._K.preconditioner is not None and model._K.preconditioner.exact
    tol = model.variance_tolerance
    tracemalloc.start()
    try:
        mu, var = model.predict(Xt)
        peak = tracemalloc.get_traced_memory()[1]
    finally:
        tracemalloc.stop()
    st = model.variance_stats
    assert len(st.v) == 512 and np.all(st.residuals < tol), st.residuals.max()
    print('C5: tracemalloc peak %.1f MB (limit %.1f MB), iterations <= %d, max ||x|| %.3e'
          % (peak / 2 ** 20, 8 * 512 * p.n / 8 / 2 ** 20, st.iterations.max(), st.xnorm.max()))
    assert peak < 8 * 512 * p.n / 8, peak
    parent = _synth_model(p, 'on-the-fly', None)
    X8 = [Xt[0][:8]] + [np.zeros((0, 1))] * (p.D - 1)
    mu8, var8 = parent.predict(X8)
    diff = np.abs(var8[0] - var[0][:8])
    print('C5: tiled against host path on 8 rows: max difference %.3e (bound %.3e)'
          % (diff.max(), 2 * tol * st.xnorm.max()))
    assert np.all(diff <= 2 * tol * st.xnorm.max()), diff.max()
