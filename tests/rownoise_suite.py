"""Checks of per-observation noise variances (rl_ski_set_noise_rows, rl_exact_set_row_noise,
LMCOperator(extra=), ExactLMCLikelihood / InterpolatedLLGP(fixed_noise=)) shared by the CPU run on
the emulator (tests/test_rownoise_emu.py) and the GPU run (tests/test_rownoise_gpu.py).  Every
function uses whichever native library is active.

Yardsticks: the oracle's operators applied column by column plus diag(e), e_i = eps_d(i) + v_i,
and SciPy's Cholesky of that matrix; for the exact likelihood a dense NumPy log-likelihood built
here and its central differences.

Shapes: synth.make_problem(2, 2, 1, 300) with the second output cut to 211 rows -- unequal
outputs, n = 511 (no multiple of 256), the output border inside the wave of rows 256 .. 319.
v is log-uniform over a factor of 30 around each row's eps (fixed seed)."""
import functools

import numpy as np
import scipy.linalg as la
import torch

from oracle import operators as ops

from runlmc_amd._native import ExactOp, GridOp, SkiOp, solve_direct, solve_pcg
from runlmc_amd.util import synth

LENS = (300, 211)
DIAG_REL = 1e-9             # of max(1 / e): loo_suite's bound for the exact inverse diagonal


def _host(t):
    return t.cpu().numpy()


def _close(got, ref, rel, what=''):
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
    print('%s: relative error %.3e (bound %.1e)' % (what, err, rel))
    assert err <= rel, '%s: relative error %.3e > %.1e' % (what, err, rel)
    return err


class Problem:
    """The synthetic problem with unequal outputs, its interpolants (contiguous rows, or the
    caller's rows permuted so that the outputs interleave), the noise-free dense operator from
    the oracle and the per-observation variances."""


@functools.lru_cache(maxsize=None)
def problem(kern, permuted=False):
    p = synth.make_problem(2, 2, 1, 300, kern=kern)
    keep = np.concatenate([np.arange(LENS[0]), 300 + np.arange(LENS[1])])
    q = Problem()
    q.base, q.kern = p, kern
    q.D, q.Q, q.m = p.D, p.Q, p.m
    q.lens = list(LENS)
    q.n = int(sum(LENS))
    assert q.n % 256 != 0 and LENS[0] % 64 != 0
    q.rows = keep
    rng = np.random.RandomState(5)
    q.perm = rng.permutation(q.n) if permuted else np.arange(q.n)
    W = p.W.tocsr()[keep][q.perm]
    q.W = W
    q.WT = W.transpose().tocsr()
    q.WT.sort_indices()
    q.tops = synth.tops(p)
    q.Bs = ops.coreg_mats(list(p.coreg_vecs), list(p.coreg_diags))
    toeps = [ops.BTTBOracle(t) for t in q.tops]
    # the oracle's operators, column by column (parity_suite.check_direct_row_orders)
    Kd = np.array([W @ ops.grid_sum_matvec(q.Bs, toeps, q.WT @ e) for e in np.eye(q.n)]).T
    q.Knf = 0.5 * (Kd + Kd.T)
    q.Knf.setflags(write=False)
    q.eps = np.array(p.noise, dtype=float)
    # (rows of repeat(eps, lens) are the CALLER's rows: with interleaved outputs the caller still
    # hands lens per output, and row i carries the level of position i in that repeat)
    q.eps_rows = np.repeat(q.eps, q.lens)
    q.v = q.eps_rows * 30.0 ** (np.random.RandomState(77).rand(q.n) - 0.5)
    q.e = q.eps_rows + q.v
    q.eps_rows.setflags(write=False)
    q.v.setflags(write=False)
    q.e.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def dense_factor(kern, permuted=False):
    q = problem(kern, permuted)
    Kd = q.Knf + np.diag(q.e)
    cf = la.cho_factor(Kd)
    return Kd, cf, 2 * np.log(np.diag(cf[0])).sum()


def handle(q):
    g = GridOp(q.D, q.m, q.Q)
    g.set_lmc(q.tops, list(q.base.coreg_vecs), list(q.base.coreg_diags))
    return SkiOp(g, q.W, q.WT)


def _dev(s, B):
    return torch.from_numpy(np.ascontiguousarray(B, dtype=np.float64)).to(s.device)


# --- 1. the product ----------------------------------------------------------------------------
def check_product(permuted):
    """mvm against the oracle's operator + e (.) x, contiguous and interleaved rows, 1 and 17
    vectors (the tolerance of the existing SKI product checks)."""
    q = problem('rbf', permuted)
    s = handle(q)
    s.set_noise_rows(q.eps, q.lens, q.v)
    rng = np.random.RandomState(11)
    for nvec in (1, 17):
        X = rng.randn(nvec, q.n)
        _close(s.matmat_host(X), X @ q.Knf + q.e * X, 1e-11, 'mvm nvec=%d permuted=%s' % (nvec, permuted))


# --- 2. the factorisation where every row is polynomial ---------------------------------------
def check_factor_exact(kern, rank):
    """factor() reports 1; log det and direct solves against dense Cholesky at the constant-noise
    check's tolerances (parity_suite.check_direct_row_orders: 1e-11, 1e-9) for 1, 17 and 40
    right-hand sides (both projection kernels)."""
    q = problem(kern)
    s = handle(q)
    s.set_noise_rows(q.eps, q.lens, q.v)
    ok, ld, _ = s.factor()
    assert ok and s.factor_mode == 1, (s.factor_mode, s.factor_reason)
    assert s.grid.form()[0] == rank, s.grid.form()
    Kd, cf, ref = dense_factor(kern)
    print('log det %s: relative error %.3e' % (kern, abs(ld - ref) / abs(ref)))
    assert abs(ld - ref) <= 1e-11 * abs(ref), (ld, ref)
    rng = np.random.RandomState(3)
    for nvec in (1, 17, 40):
        B = rng.randn(nvec, q.n)
        X, it, rs, st = solve_direct(s, _dev(s, B), tol=1e-9)
        _close(_host(X), la.cho_solve(cf, B.T).T, 1e-9, 'solve_direct %s nvec=%d' % (kern, nvec))
        assert np.all(st == 10), st
        assert np.all(np.asarray(rs) < 1e-9), rs


# --- 3. interleaved rows -----------------------------------------------------------------------
def check_interleaved():
    """A caller whose rows interleave the outputs: per-output noise through set_noise still
    declines (existing behaviour); set_noise_rows factors and solves in the caller's order."""
    q = problem('rbf', True)
    s = handle(q)
    s.set_noise(q.eps, q.lens)
    ok = s.factor()[0]
    assert not ok and 'noise' in s.factor_reason, s.factor_reason
    s.set_noise_rows(q.eps, q.lens, q.v)
    ok, ld, _ = s.factor()
    assert ok and s.factor_mode == 1, (s.factor_mode, s.factor_reason)
    Kd, cf, ref = dense_factor('rbf', True)
    assert abs(ld - ref) <= 1e-11 * abs(ref), (ld, ref)
    B = np.random.RandomState(4).randn(3, q.n)
    X, it, rs, st = solve_direct(s, _dev(s, B), tol=1e-9)
    _close(_host(X), la.cho_solve(cf, B.T).T, 1e-9, 'solve_direct, interleaved rows')
    d, exact = s.inverse_diag()
    assert exact
    err = np.abs(_host(d) - np.diag(la.inv(Kd))).max()
    assert err <= DIAG_REL * np.max(1.0 / q.e), err


# --- 4. the fold identity ------------------------------------------------------------------------
def check_fold_handle():
    """v_i = c_d constant per output: set_noise_rows(eps, lens, c) and set_noise(eps + c, lens)
    agree on log det, direct solves and the inverse diagonal to 1e-10 relative."""
    q = problem('rbf')
    c = np.array([0.03, 0.2])
    a, b = handle(q), handle(q)
    a.set_noise_rows(q.eps, q.lens, np.repeat(c, q.lens))
    b.set_noise(q.eps + c, q.lens)
    (oka, lda, _), (okb, ldb, _) = a.factor(), b.factor()
    assert oka and okb and a.factor_mode == 1 and b.factor_mode == 1
    assert abs(lda - ldb) <= 1e-10 * abs(ldb), (lda, ldb)
    B = np.random.RandomState(8).randn(5, q.n)
    Xa = solve_direct(a, _dev(a, B), tol=1e-12)[0]
    Xb = solve_direct(b, _dev(b, B), tol=1e-12)[0]
    _close(_host(Xa), _host(Xb), 1e-10, 'fold: direct solves')
    _close(_host(a.inverse_diag()[0]), _host(b.inverse_diag()[0]), 1e-10, 'fold: inverse diagonal')


def _synth_model(q, fixed=None, noise=None, normalize=False, seed=1, **kw):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    p = q.base
    fk = synth.functional_kernel(p)
    # (copies: an optimiser writes into the model's parameter arrays, the problem is shared)
    fk.coreg_vecs = [np.array(a, dtype=float) for a in p.coreg_vecs]
    fk.coreg_diags = [np.array(k, dtype=float) for k in p.coreg_diags]
    fk.noise = np.array(q.eps if noise is None else noise, dtype=float)
    Xs = [p.Xs[0][:LENS[0]], p.Xs[1][:LENS[1]]]
    Ys = [p.Ys[0][:LENS[0]], p.Ys[1][:LENS[1]]]
    return InterpolatedLLGP(Xs, Ys, normalize=normalize, functional_kernel=fk, device_probes=seed,
                            fixed_noise=fixed, **kw)


def check_fold_model():
    """InterpolatedLLGP(fixed_noise = c sd^2) at noise eps and a plain model at noise eps + c (the
    same device_probes seed) agree to 1e-8 on the log likelihood, every gradient block, loo_predict
    and posterior draws of one seed: any layer that still used eps alone would show."""
    q = problem('rbf')
    c = np.array([0.03, 0.2])
    p = q.base
    sd = np.array([p.Ys[0][:LENS[0]].std(), p.Ys[1][:LENS[1]].std()])
    fixed = [np.full(n, cd * s ** 2) for n, cd, s in zip(q.lens, c, sd)]
    a = _synth_model(q, fixed=fixed, normalize=True)
    b = _synth_model(q, noise=q.eps + c, normalize=True)
    _close(a.log_likelihood(), b.log_likelihood(), 1e-8, 'fold: log likelihood')
    for (name, _, _, ga), (_, _, _, gb) in zip(a._param_blocks(), b._param_blocks()):
        _close(np.ravel(ga()), np.ravel(gb()), 1e-8, 'fold: gradient block %s' % name)
    (ma, va), (mb, vb) = a.loo_predict(), b.loo_predict()
    _close(np.concatenate(ma), np.concatenate(mb), 1e-8, 'fold: loo means')
    _close(np.concatenate(va), np.concatenate(vb), 1e-8, 'fold: loo variances')
    Xt = [np.linspace(0.05, 0.95, 7).reshape(-1, 1)] * 2
    da = a.posterior_draws(4, seed=9, tolerance=1e-10)(Xt)
    db = b.posterior_draws(4, seed=9, tolerance=1e-10)(Xt)
    _close(np.concatenate(da, axis=1), np.concatenate(db, axis=1), 1e-8, 'fold: posterior draws')


# --- 5. the preconditioner of rows outside the polynomial form -------------------------------
def check_precond():
    """Matern rows: factor() reports 2 (the 96 functions decline for per-observation noise),
    rl_solve_pcg meets its tolerance and matches the dense solve at 1e-8; the preconditioned
    log det is within its own reported error of the dense value, or refused with the reason."""
    from runlmc_amd.lmc.grid_kernel import FactoredInverse
    q = problem('matern')
    s = handle(q)
    s.set_noise_rows(q.eps, q.lens, q.v)
    ok = s.factor()[0]
    assert ok and s.factor_mode == 2, (s.factor_mode, s.factor_reason)
    Kd, cf, ref = dense_factor('matern')
    B = np.random.RandomState(6).randn(3, q.n)
    X, it, rs, st = solve_pcg(s, _dev(s, B), tol=1e-10)
    assert np.all(np.asarray(rs) < 1e-10), rs
    _close(_host(X), la.cho_solve(cf, B.T).T, 1e-8, 'solve_pcg')
    print('solve_pcg iterations', it)
    # P^-1 = precond_apply(I) is symmetric and its diagonal is inverse_diag's
    Pinv = _host(s.precond_apply(torch.eye(q.n, dtype=torch.float64, device=s.device)))
    assert np.abs(Pinv - Pinv.T).max() <= 1e-12 * np.abs(Pinv).max()
    d, exact = s.inverse_diag()
    assert exact is False
    _close(_host(d), np.diag(Pinv), 1e-10, 'preconditioner diagonal')
    try:
        est, sem, _ = FactoredInverse(s, exact=False).logdet_estimate(tol=1e-8)
    except (NotImplementedError, ValueError, RuntimeError) as e:
        assert 'per-observation noise' in str(e), str(e)
        return None
    # (16 probes of a fixed seed: the estimator's own bar, parity_suite's 4 sem + 1e-9 |ld|)
    print('preconditioned log det %.6f +- %.2e, dense %.6f' % (est, sem, ref))
    assert abs(est - ref) <= 4 * sem + 1e-9 * abs(ref), (est, sem, ref)
    return est


# --- 6. the inverse diagonal ---------------------------------------------------------------------
def check_inverse_diag(kern):
    q = problem(kern)
    s = handle(q)
    s.set_noise_rows(q.eps, q.lens, q.v)
    assert s.factor()[0] and s.factor_mode == 1
    Kd, cf, _ = dense_factor(kern)
    d, exact = s.inverse_diag()
    assert exact
    err = np.abs(_host(d) - np.diag(la.inv(Kd))).max()
    bound = DIAG_REL * np.max(1.0 / q.e)
    print('inverse_diag %s: max error %.3e, bound %.3e' % (kern, err, bound))
    assert err <= bound, (err, bound)


# --- 7. the exact likelihood ---------------------------------------------------------------------
def _exact_dense(kerns, A, kappa, X, lens):
    """The noise-free exact LMC kernel in NumPy: sum_q (A_q^T A_q + diag kappa_q)[o, o] k_q(r)."""
    o = np.repeat(np.arange(len(lens)), lens)
    r = np.abs(X[:, None] - X[None, :])
    K = np.zeros((len(X), len(X)))
    for k, a, kap in zip(kerns, A, kappa):
        a = np.atleast_2d(a)
        B = a.T @ a + np.diag(kap)
        K += B[np.ix_(o, o)] * k(r)
    return K


def _exact_params(q):
    p = q.base
    return dict(A=[np.array(a, dtype=float) for a in p.coreg_vecs],
                kappa=[np.array(k, dtype=float) for k in p.coreg_diags],
                theta=[np.array([g]) for g in p.inv_lengthscales], noise=np.array(q.eps))


def _exact_loglik(prm, X, y, lens, v):
    kerns = [lambda r, g=float(t[0]): np.exp(-0.5 * g * r * r) for t in prm['theta']]
    K = _exact_dense(kerns, prm['A'], prm['kappa'], X, lens) + np.diag(np.repeat(prm['noise'], lens) + v)
    c = la.cho_factor(K, lower=True)
    ld = 2 * np.log(np.diag(c[0])).sum()
    return -0.5 * (ld + y @ la.cho_solve(c, y) + len(y) * np.log(2 * np.pi)), K, ld


# eighth-order central differences: f'(x) = sum_k c_k (f(x + k h) - f(x - k h)) / h + O(h^8)
_STENCIL = ((1, 4.0 / 5), (2, -1.0 / 5), (3, 4.0 / 105), (4, -1.0 / 280))


def _central(f, arr, idx, h):
    x0 = arr[idx]
    acc = 0.0
    for k, ck in _STENCIL:
        arr[idx] = x0 + k * h
        up = f()
        arr[idx] = x0 - k * h
        acc += ck * (up - f())
    arr[idx] = x0
    return acc / h


def check_exact():
    """dense_host with row noise is the same handle's matrix without it plus diag(v) (equal off
    the diagonal, one ulp on it); log det, alpha and the four gradient families against a dense
    NumPy log-likelihood and its central differences, at exact_suite's tolerances (1e-11 for the
    log det, 1e-9 for the rest)."""
    from runlmc_amd.kern.stationary import RBF
    from runlmc_amd.lmc import ExactLMCLikelihood
    from runlmc_amd.lmc.functional_kernel import FunctionalKernel
    q = problem('rbf')
    p = q.base
    Xs = [p.Xs[0][:LENS[0]], p.Xs[1][:LENS[1]]]
    Ys = [p.Ys[0][:LENS[0]], p.Ys[1][:LENS[1]]]
    X, y = np.vstack(Xs)[:, 0], np.concatenate(Ys)
    prm = _exact_params(q)
    fk = FunctionalKernel(D=q.D, lmc_kernels=[RBF(float(t[0])) for t in prm['theta']], lmc_ranks=[1] * q.Q)
    fk.coreg_vecs = [a.copy() for a in prm['A']]
    fk.coreg_diags = [k.copy() for k in prm['kappa']]
    fk.noise = prm['noise'].copy()
    fk.set_input_dim(1)
    op = ExactOp(q.n, 1)
    op.set(X[:, None], q.lens, fk.kernels, fk.coreg_mats(), fk.noise)
    K0 = op.dense()
    op.set_row_noise(q.v)
    K1 = op.dense()
    off = ~np.eye(q.n, dtype=bool)
    assert np.array_equal(K0[off], K1[off])
    want = np.diag(K0) + q.v
    assert np.all(np.abs(np.diag(K1) - want) <= np.spacing(want)), np.abs(np.diag(K1) - want).max()
    # (kept across a set; the noise-free cross-covariance does not see it; NULL clears it)
    op.set(X[:, None], q.lens, fk.kernels, fk.coreg_mats(), fk.noise)
    assert np.array_equal(op.dense(), K1)
    Xt = np.linspace(0.1, 0.9, 5)[:, None]
    cross1 = op.cross(np.vstack([Xt, Xt]), [5, 5])
    op.set_row_noise(None)
    assert np.array_equal(op.dense(), K0)
    assert np.array_equal(op.cross(np.vstack([Xt, Xt]), [5, 5]), cross1)

    lik = ExactLMCLikelihood(fk, Xs, Ys, fixed_noise=q.v)
    ll, K, ld = _exact_loglik(prm, X, y, q.lens, q.v)
    _close(lik.K, K, 1e-12, 'exact K')
    _close(lik.log_det_K(), ld, 1e-11, 'exact log det')
    _close(lik.alpha(), la.solve(K, y, assume_a='pos'), 1e-9, 'exact alpha')
    _close(lik.log_likelihood(), ll, 1e-9, 'exact log likelihood')

    def f():
        return _exact_loglik(prm, X, y, q.lens, q.v)[0]
    h = 2e-3
    vec = [np.array([[_central(f, a, (i, j), h) for j in range(a.shape[1])] for i in range(a.shape[0])])
           for a in prm['A']]
    diag = [np.array([_central(f, k, (i,), h) for i in range(len(k))]) for k in prm['kappa']]
    kern = [np.array([_central(f, t, (0,), h * float(t[0]))]) for t in prm['theta']]
    noise = np.array([_central(f, prm['noise'], (d,), h * float(prm['noise'][d])) for d in range(q.D)])
    for i in range(q.Q):
        _close(lik.coreg_vec_gradients()[i], vec[i], 1e-9, 'exact coreg_vec %d' % i)
        _close(lik.coreg_diags_gradients()[i], diag[i], 1e-9, 'exact coreg_diag %d' % i)
        _close(np.asarray(lik.kernel_gradients()[i], dtype=float), kern[i], 1e-9, 'exact kernel %d' % i)
    _close(lik.noise_gradient(), noise, 1e-9, 'exact noise')


# --- 9. validation and refusals -----------------------------------------------------------------
def check_validation():
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    q = problem('rbf')
    s = handle(q)
    bad = [(q.eps, q.lens, -q.v), (q.eps, q.lens, np.where(np.arange(q.n) == 7, np.nan, q.v)),
           (q.eps, q.lens, np.where(np.arange(q.n) == 7, np.inf, q.v)), (q.eps, [300, 210], q.v)]
    for noise, lens, extra in bad:
        try:
            s.set_noise_rows(noise, lens, extra)
        except ValueError:
            pass
        else:
            raise AssertionError('set_noise_rows accepted a bad argument')
    for extra in (q.v[:-1], None):
        try:
            s.set_noise_rows(q.eps, q.lens, extra)
        except (ValueError, TypeError):
            pass
        else:
            raise AssertionError('set_noise_rows accepted a bad extra')
    rc = s.lib.cdll.rl_ski_set_noise_rows(s.handle, None, None, None)
    assert rc != 0, rc
    op = ExactOp(q.n, 1)
    for extra in (-q.v, np.where(np.arange(q.n) == 3, np.nan, q.v), q.v[:-1]):
        try:
            op.set_row_noise(extra)
        except ValueError:
            pass
        else:
            raise AssertionError('set_row_noise accepted a bad argument')
    # after set_noise_rows a plain set_noise restores the per-output behaviour: the bits of a
    # fresh handle
    s.set_noise_rows(q.eps, q.lens, q.v)
    assert s.factor()[0]
    s.set_noise(q.eps, q.lens)
    fresh = handle(q)
    fresh.set_noise(q.eps, q.lens)
    a, b = s.factor(), fresh.factor()
    assert a == b and s.factor_mode == fresh.factor_mode == 1, (a, b)
    B = np.random.RandomState(2).randn(3, q.n)
    assert np.array_equal(_host(solve_direct(s, _dev(s, B), tol=1e-9)[0]),
                          _host(solve_direct(fresh, _dev(fresh, B), tol=1e-9)[0]))
    assert np.array_equal(_host(s.inverse_diag()[0]), _host(fresh.inverse_diag()[0]))
    # the model's arguments
    p = q.base
    Xs = [p.Xs[0][:LENS[0]], p.Xs[1][:LENS[1]]]
    Ys = [p.Ys[0][:LENS[0]], p.Ys[1][:LENS[1]]]
    good = [q.v[:300], q.v[300:]]
    for fixed in ([good[0]], [good[0], good[1][:-1]], [good[0], -good[1]],
                  [good[0], np.where(np.arange(211) == 2, np.nan, good[1])],
                  [np.where(np.arange(300) == 2, np.inf, good[0]), good[1]]):
        try:
            InterpolatedLLGP(Xs, Ys, functional_kernel=synth.functional_kernel(p), fixed_noise=fixed)
        except ValueError:
            pass
        else:
            raise AssertionError('InterpolatedLLGP accepted a bad fixed_noise')


# --- 8. the model with varying v ----------------------------------------------------------------
def _brute_loo(Kd, y, rows):
    """Leave-one-out by deleting the row and column: the dense conditional Gaussian itself."""
    mean, var = np.zeros(len(rows)), np.zeros(len(rows))
    for k, i in enumerate(rows):
        keep = np.delete(np.arange(len(y)), i)
        sol = la.solve(Kd[np.ix_(keep, keep)], np.column_stack([y[keep], Kd[keep, i]]), assume_a='pos')
        mean[k], var[k] = Kd[i, keep] @ sol[:, 0], Kd[i, i] - Kd[i, keep] @ sol[:, 1]
    return mean, var


def check_model(which):
    """InterpolatedLLGP(fixed_noise = v) with v varying per row against the dense conditional
    Gaussian of K~ = W K_UU W^T + diag(eps + v): normal_quadratic, log_det_K, predict,
    loo_predict on 20 rows (brute force), at the tolerances of the existing model checks.
      '1d'    the synthetic problem, normalize=True (v is handed over in the units of Y^2 and must
              arrive divided by sd^2), the operator's factorisation; then three optimiser steps
              and the operator's diagonal is the new eps + v;
      '2d'    golden lmc_2d with precond_rank=32 (no polynomial factorisation: Krylov);
      'exact' the synthetic problem with prediction='exact' (variances from the dense exact K)."""
    from parity_suite import _dense_pieces, _exact_cross, functional_kernel_for
    from cases import Case
    import loo_suite
    from runlmc_amd.approx.interpolation import multi_interpolant
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    rng = np.random.RandomState(9)
    if which == '2d':
        c = Case('lmc_2d')
        spec, _, Kd0, Kuu = _dense_pieces(c)
        eps, lens, D = np.asarray(c.noise, dtype=float), c.lens, c.D
        eps_rows = np.repeat(eps, lens)
        v = eps_rows * 30.0 ** (np.random.RandomState(77).rand(c.n) - 0.5)
        Knf = Kd0 - np.diag(eps_rows)
        Xs = [np.asarray(x).reshape(len(x), c.P) for x in c.Xs]
        Ys, WT, axes = c.Ys, c.WT, c.grid_axes
        sd, mu = np.ones(D), np.zeros(D)
        kfun = [k.from_dist for k in spec._kernels]
        Bs = spec.coreg_mats()
        Xt = [np.sort(rng.rand(4 + d, c.P), axis=0) * 0.9 + 0.05 for d in range(D)]
        with loo_suite._tight_krylov():
            model = InterpolatedLLGP(Xs, Ys, normalize=False, m=[len(a) - 4 for a in axes],
                                     functional_kernel=functional_kernel_for(c), tolerance=1e-12,
                                     precond_rank=32, device_probes=3,
                                     fixed_noise=np.split(v, np.cumsum(lens)[:-1]))
            model._ensure()
            assert model._K.device_operator().factor_mode == 4
            alpha, nq = model.kernel.alpha(), model.normal_quadratic()
    else:
        q = problem('rbf')
        p = q.base
        eps, lens, D, v = q.eps, q.lens, q.D, q.v
        eps_rows = q.eps_rows
        Xs = [p.Xs[0][:LENS[0]], p.Xs[1][:LENS[1]]]
        Ys = [p.Ys[0][:LENS[0]], p.Ys[1][:LENS[1]]]
        kerns = synth.kernel_objects(p.kern_desc)
        kfun, Bs = [k.from_dist for k in kerns], q.Bs
        Xt = [np.sort(rng.rand(4 + d, 1), axis=0) * 0.9 + 0.05 for d in range(D)]
        norm = which == '1d'
        sd = np.array([Y.std() for Y in Ys]) if norm else np.ones(D)
        mu = np.array([Y.mean() for Y in Ys]) if norm else np.zeros(D)
        # (handed over in the units of Y^2: the model divides by sd^2 and works with v)
        fixed = [vd * s ** 2 for vd, s in zip(np.split(v, np.cumsum(lens)[:-1]), sd)]
        model = _synth_model(q, fixed=fixed, normalize=norm, tolerance=1e-9,
                             prediction='exact' if which == 'exact' else 'on-the-fly')
        model._ensure()
        assert model._K.device_operator().factor_mode == 1
        alpha, nq = model.kernel.alpha(), model.normal_quadratic()
        # (the model lays its own grid over the cut data: the oracle's operator on THAT grid)
        axes = model.grid_axes[(0,)]
        W, WT = model.interpolants[(0,)]
        toeps = [ops.BTTBOracle(k(model.dists[(0,)])) for k in kfun]
        Kuu = ops.dense_from_matvec(lambda x: ops.grid_sum_matvec(Bs, toeps, x), D * len(axes[0]))
        Kuu = 0.5 * (Kuu + Kuu.T)
        Knf = W @ (W @ Kuu).T
    n = int(sum(lens))
    y = np.concatenate([(Y - m_) / s for Y, m_, s in zip(Ys, mu, sd)])
    e = eps_rows + v
    Kd = Knf + np.diag(e)
    Kd = 0.5 * (Kd + Kd.T)
    cf = la.cho_factor(Kd)
    aref = la.cho_solve(cf, y)
    ld_ref = 2 * np.log(np.diag(cf[0])).sum()
    # the operator the model built is that matrix
    _close(np.diag(model._K.Ks[-1].as_numpy()), e, 1e-15, 'model %s: Diag term' % which)
    r = np.linalg.norm(y - Kd @ alpha)
    if which == '2d':
        # (Krylov at tolerance 1e-12: a residual r moves alpha by at most r / min e, pivchol_suite's rule)
        assert r < 1e-8 * np.linalg.norm(y), r
        assert np.abs(alpha - aref).max() <= r / e.min() + 1e-12 * np.abs(aref).max()
        assert abs(nq - y @ aref) <= np.linalg.norm(y) * r / e.min() + 1e-12 * abs(y @ aref)
        model.log_det_K()
        est, sem, _ = model.kernel.deriv.logdet_precond
        print('model 2d log det %.6f +- %.2e, dense %.6f' % (est, sem, ld_ref))
        assert abs(est - ld_ref) <= 4.0 * sem + 1e-9 * abs(ld_ref), (est, ld_ref, sem)
    else:
        _close(alpha, aref, 1e-8, 'model %s: alpha' % which)
        _close(nq, y @ aref, 1e-8, 'model %s: normal_quadratic' % which)
        _close(model.log_det_K(), ld_ref, 1e-9, 'model %s: log_det_K' % which)
    # predict: the mean of the SKI model; variances of a NEW observation (eps_d only on top)
    Wt = multi_interpolant([x[:, list(range(x.shape[1]))] for x in Xt], *axes).toarray()
    tl = [len(x) for x in Xt]
    sdt, mut = np.repeat(sd, tl), np.repeat(mu, tl)
    mean_ref = (Wt @ (Kuu @ (WT @ aref))) * sdt + mut
    k0 = np.array([float(k(0.0)) for k in kfun])
    native = np.repeat(np.array([np.diag(B) for B in Bs]).T @ k0 + eps, tl)
    ro, co = np.repeat(np.arange(D), tl), np.repeat(np.arange(D), lens)

    def exact_kernel(A, B_, oa, ob):
        dist = np.sqrt(np.square(A[:, None, :] - B_[None, :, :]).sum(axis=-1))
        return sum(B[np.ix_(oa, ob)] * k(dist) for B, k in zip(Bs, kfun))
    Xa, Xb = np.vstack(Xt), np.vstack(Xs)
    Kx = exact_kernel(Xa, Xb, ro, co)
    if which == 'exact':
        Kex = exact_kernel(Xb, Xb, co, co) + np.diag(e)
        var_ref = native - np.einsum('ij,ji->i', Kx, la.solve(Kex, Kx.T, assume_a='pos'))
        atol = 1e-8 * native.max()              # exact_suite.check_model_exact_prediction
    else:
        var_ref = native - np.einsum('ij,ji->i', Kx, la.cho_solve(cf, Kx.T))
        atol = 1e-5 * max(native.max(), 1.0)    # parity_suite.check_model_prediction
    var_ref = np.clip(var_ref, 0, None) * sdt ** 2
    if which == '2d':
        with loo_suite._tight_krylov():
            mean, var = model.predict(Xt)
    else:
        mean, var = model.predict(Xt)
    _close(np.concatenate(mean), mean_ref, 1e-5, 'model %s: predictive mean' % which)
    err = np.abs(np.concatenate(var) - var_ref).max()
    print('model %s: predictive variance error %.3e (bound %.1e)' % (which, err, atol * sdt.max() ** 2))
    assert np.all(np.abs(np.concatenate(var) - var_ref) <= atol * sdt ** 2), err
    # leave-one-out on 20 rows against brute force (loo_suite.check_model_loo's bars); the
    # borders of the outputs among them
    ends = np.cumsum(lens)[:-1]
    sel = np.unique(np.concatenate([[0, n - 1], ends - 1, ends,
                                    np.random.RandomState(2).choice(n, 20, replace=False)]))[:20]
    bm, bv = _brute_loo(Kd, y, sel)
    sdr, mur = np.repeat(sd, lens)[sel], np.repeat(mu, lens)[sel]
    y_raw = np.concatenate(Ys)
    d = 1.0 / bv
    mean_tol = 1e-8 * np.abs(y_raw).max()
    var_tol = loo_suite.DIAG_REL * np.max(1.0 / e) / d ** 2 * sdr ** 2
    if which == '2d':
        with loo_suite._tight_krylov():
            lm, lv = model.loo_predict(indices=sel, method='solve', tol=1e-12)
    else:
        lm, lv = model.loo_predict(indices=sel)
        assert model.loo_stats['method'] == 'direct', model.loo_stats
    em, ev = np.abs(lm - (bm * sdr + mur)).max(), (np.abs(lv - bv * sdr ** 2) / var_tol).max()
    print('model %s: loo mean error %.3e (bound %.1e), variance error / bound %.3e' % (which, em, mean_tol, ev))
    assert em <= mean_tol and ev <= 1.0, (em, mean_tol, ev)
    if which != '1d':
        return
    # posterior draws: the data side of Matheron's rule carries sqrt(e_i) per training row -- the
    # draws' mean over many draws is statistical; what is exact is that the rule's residual used
    # the operator's diagonal (checked through the fold identity); here: they run and are finite
    dr = model.posterior_samples(Xt, size=2, seed=1, noise=True)
    assert all(np.all(np.isfinite(x)) for x in dr)
    # three optimiser steps: the operator's diagonal is the NEW eps + v, v as handed over / sd^2
    model.optimize(max_it=3)
    new_eps = np.array(model._functional_kernel.noise, dtype=float)
    assert not np.allclose(new_eps, eps)
    want = np.repeat(new_eps, lens) + v
    _close(model._K.Ks[-1].v, want, 1e-15, 'model 1d: Diag after optimize')
    X = np.random.RandomState(1).randn(2, n)
    ski = model._K.device_operator()
    nf = ski.apply_w(ski.grid.mvm(ski.apply_wt(_dev(ski, X))))
    _close(ski.matmat_host(X) - _host(nf), want * X, 1e-11, 'model 1d: operator diagonal after optimize')
