"""Checks of leave-one-out cross-validation (runlmc_amd.approx.loo, InterpolatedLLGP.loo_predict /
loo_log_likelihood, include/runlmc_hip.h: rl_ski_inverse_diag, rl_ski_precond_apply,
rl_diag_accumulate, rl_loo_reduce) shared by the CPU run on the emulator (tests/test_loo_emu.py)
and the GPU run (tests/test_loo_gpu.py).  Every function uses whichever native library is active.

The reference has no leave-one-out; the yardstick everywhere is the ORACLE's dense K~ inverted by
NumPy / SciPy.  Where an estimator is defined through the library's own preconditioner P (the
control variate of the probe estimate) the dense P^-1 enters the restatement as P, the estimator's
parameter; K~^-1 is always the oracle's."""
import ctypes
import logging

import numpy as np
import scipy.linalg as la
import torch

from oracle import operators as ops
from oracle import likelihood as olik
from cases import Case
from parity_suite import (_synth_problem_and_oracle, _dense_spd, _env_set, functional_kernel_for_synth,
                          functional_kernel_for, build_operator, _dense_pieces)

from runlmc_amd import _lib
from runlmc_amd._native import GridOp, SkiOp, diag_accumulate, loo_reduce, solve_pcg
from runlmc_amd.approx import loo
from runlmc_amd.approx.iterative import Iterative
from runlmc_amd.approx.quadforms import UnitRows, quad_forms

DIAG_REL = 1e-9            # of max(1 / eps): what check_direct_solve holds the direct solve to
SOLVE_TOL = 1e-10


def _host(t):
    return t.cpu().numpy()


class _tight_krylov:
    """Krylov solves that reach 1e-10 on these small systems: MINRES ended by the residual rule
    alone, checked every 10 iterations (pathwise_suite's switch)."""

    def __enter__(self):
        self.saved = (Iterative.SCIPY_EXITS, Iterative.CHECK_EVERY)
        Iterative.SCIPY_EXITS, Iterative.CHECK_EVERY = False, 10

    def __exit__(self, *exc):
        Iterative.SCIPY_EXITS, Iterative.CHECK_EVERY = self.saved


# --- 1. the diagonal from the factorisation -----------------------------------------------------------
MIN_GRID = 96              # the polynomial form takes grids of at least 2 x 48 points (rl_gridop.hip)
DECLINED = {('periodic', 16, 70): 92}     # no factorisation at the first size: check_inverse_diag


def _synth_on_grid(D, Q, m_data, kern):
    """parity_suite's synthetic problem with its operator and oracle.  The recipe's grid has
    m_data + 4 points; below MIN_GRID the handle has no polynomial form and nothing to factorise,
    so a problem of fewer points per output is put on a grid of MIN_GRID points instead (same
    data, same kernels, same couplings)."""
    if m_data + 4 >= MIN_GRID:
        return _synth_problem_and_oracle(D, Q, m_data, kern)
    from runlmc_amd.util import synth
    from runlmc_amd.approx.interpolation import autogrid, multi_interpolant
    from runlmc_amd.lmc.grid_kernel import gen_grid_kernel
    from oracle.kernels import KernelSpec, RBFSpec, Matern32Spec, StdPeriodicSpec
    p = synth.make_problem(D, Q, 1, m_data, kern=kern)
    p.grid = autogrid(p.Xs, None, None, [MIN_GRID - 4])[0]
    p.grid_dists = p.grid - p.grid[0]
    p.m = len(p.grid)
    p.W = multi_interpolant(p.Xs, p.grid)
    p.WT = p.W.transpose().tocsr()
    p.WT.sort_indices()
    p.WT.indices = p.WT.indices.astype(np.int32)
    p.WT.indptr = p.WT.indptr.astype(np.int32)
    fk = synth.functional_kernel(p)
    ad = (0,)
    K, gks = gen_grid_kernel(fk, {ad: p.grid_dists}, {ad: (p.W, p.WT)}, p.lens)
    spec = KernelSpec(p.D, synth.kernel_objects(p.kern_desc, rbf=RBFSpec, periodic=StdPeriodicSpec,
                                                matern=Matern32Spec),
                      list(p.coreg_vecs), list(p.coreg_diags), p.noise)
    spec.set_input_dim(1)
    op = olik.LMCOperatorOracle(spec, p.grid_dists, p.W, p.WT, p.lens)
    return p, fk, K, gks[ad], spec, op


def check_inverse_diag(kern, D, m_data):
    """rl_ski_inverse_diag (k_dz_diag) against diag(inv(K~)) of the oracle's dense K~ at
    1e-9 max(1 / eps), again after a coupling update (x 1.7) and after a noise update with a
    different level per output.  (D, m_data) = (16, 70) runs on a 96-point grid: _synth_on_grid.)
    The periodic family at (16, 70) has 36 functions per output and the handle declines to
    factorise 70 rows on them (rl_ski_factor: available = 0, 'too few (or degenerate) rows for the
    basis'; so at 80): there the decline is what is checked -- inverse_diag raises with the handle's
    reason -- and the diagonal is held to the same bound at 92 points per output, the fewest of
    the recipe that factorise."""
    if (kern, D, m_data) in DECLINED:
        p, fk, K, gk, spec, op = _synth_on_grid(D, 2, m_data, kern)
        ski = K.device_operator()
        assert not ski.factor()[0] and ski.factor_mode == 0
        reason = ski.factor_reason
        assert 'too few' in reason, reason
        try:
            ski.inverse_diag()
        except NotImplementedError as e:
            assert 'too few' in str(e) and 'rl_ski_inverse_diag' in str(e), str(e)
        else:
            raise AssertionError('inverse_diag answered without a factorisation')
        try:
            loo.inverse_diagonal(K, method='direct')
        except NotImplementedError as e:
            assert 'too few' in str(e), str(e)
        else:
            raise AssertionError("method='direct' answered without a factorisation")
        m_data = DECLINED[kern, D, m_data]
    p, fk, K, gk, spec, op = _synth_on_grid(D, 2, m_data, kern)
    ski = K.device_operator()
    ok = ski.factor()[0]
    assert ok and ski.factor_mode == 1, (ski.factor_mode, ski.factor_reason)
    out = dict(rank=gk._op.form()[0], n=p.n, err=[])
    print('inverse_diag %s D=%d m=%d: grid of %d points, rank %d' % (kern, D, m_data, p.m, out['rank']))

    def held(Kd, noise):
        d, exact = ski.inverse_diag()
        assert exact is True and d.shape == (p.n,)
        ref = np.diag(la.inv(Kd))
        bound = DIAG_REL * np.max(1.0 / noise)
        err = np.abs(_host(d) - ref).max()
        out['err'].append(err / np.max(1.0 / noise))
        print('inverse_diag %s D=%d m=%d: max error %.3e, bound %.3e' % (kern, D, m_data, err, bound))
        assert err <= bound, (err, bound)

    Kd = _dense_spd(op, p.n)
    held(Kd, p.noise)
    gk.update(functional_kernel_for_synth(p, scale=1.7), p.grid_dists)
    spec.coreg_vecs = [np.sqrt(1.7) * a for a in spec.coreg_vecs]
    spec.coreg_diags = [1.7 * k for k in spec.coreg_diags]
    op2 = olik.LMCOperatorOracle(spec, p.grid_dists, p.W, p.WT, p.lens)
    Kd2 = _dense_spd(op2, p.n)
    held(Kd2, p.noise)
    noise2 = p.noise * np.linspace(0.5, 2.0, D) if D > 1 else p.noise * 0.6
    K.update_noise(noise2, p.lens)
    held(Kd2 + np.diag(np.repeat(noise2 - p.noise, p.lens)), noise2)
    return out


# --- 2. output borders -----------------------------------------------------------------------------
def check_inverse_diag_borders(lens=(37, 64, 129)):
    """A handle built by hand whose outputs end inside a wave, next to a wave's edge and inside a
    workgroup, every output with its own noise and the caller's rows in a random order: row by
    row, in the caller's order, against the dense inverse.  (The handle takes the noise per block
    of the CALLER's rows, so the random order stays inside each output: across outputs the noise
    would no longer be constant per output and the handle would decline to factorise.)"""
    from runlmc_amd.approx.interpolation import autogrid, multi_interpolant
    from runlmc_amd.kern.stationary import RBF
    rng = np.random.RandomState(23)
    D, Q = len(lens), 2
    Xs = [rng.permutation(np.sort(rng.rand(n))).reshape(-1, 1) for n in lens]
    assert all(np.any(np.diff(X[:, 0]) < 0) for X in Xs)            # not in the handle's order
    grid = autogrid(Xs, None, None, [150])[0]
    dists = grid - grid[0]
    W = multi_interpolant(Xs, grid).tocsr()
    WT = W.transpose().tocsr()
    WT.sort_indices()
    tops = np.array([RBF(g).from_dist(dists) for g in (1.0, 10.0)])
    A = [rng.randn(1, D) for _ in range(Q)]
    kap = [np.abs(rng.randn(D)) + 0.1 for _ in range(Q)]
    noise = np.array([0.05, 0.2, 0.11, 0.4, 0.07][:D])
    m = len(grid)
    g = GridOp(D, m, Q)
    g.set_lmc(tops, A, kap)
    s = SkiOp(g, W, WT)
    s.set_noise(noise, lens)
    ok = s.factor()[0]
    assert ok and s.factor_mode == 1, (s.factor_mode, s.factor_reason)
    Bs = ops.coreg_mats(A, kap)
    toeps = [ops.BTTBOracle(t) for t in tops]
    Kuu = ops.dense_from_matvec(lambda v: ops.grid_sum_matvec(Bs, toeps, v), D * m)
    Wd = W.toarray()
    Kd = Wd @ (0.5 * (Kuu + Kuu.T)) @ Wd.T + np.diag(np.repeat(noise, lens))
    ref = np.diag(la.inv(Kd))
    d, exact = s.inverse_diag()
    assert exact
    err = np.abs(_host(d) - ref)
    bound = DIAG_REL * np.max(1.0 / noise)
    print('inverse_diag borders %s: max error %.3e, bound %.3e' % (lens, err.max(), bound))
    assert np.all(err <= bound), (np.flatnonzero(err > bound), err.max(), bound)
    # (the wrong output's noise at a border is an error of |1 / eps_a - 1 / eps_b| >= 2: far above)
    return err.max() / np.max(1.0 / noise)


# --- 3. the preconditioner's diagonal -----------------------------------------------------------------
def check_precond_diag(m_data=300):
    """Matern rows, the factorisation a preconditioner P on the 48 functions (available = 2):
    P^-1 = precond_apply(I) is symmetric, and inverse_diag is its diagonal -- the new kernel
    against the project / mix / expand path.  On the 96-function basis (available = 3) the
    diagonal is declined with the reason, precond_apply still is PCG's first application."""
    with _env_set(RUNLMC_PRECOND_HI_MIN=0, RUNLMC_NO_PRECOND_HI=1):
        p, fk, K, gk, spec, op = _synth_problem_and_oracle(2, 2, m_data, 'matern')
        ski = K.device_operator()
        ok = ski.factor()[0]
    assert ok and ski.factor_mode == 2, (ski.factor_mode, ski.factor_reason)
    d, exact = ski.inverse_diag()
    assert exact is False
    eye = torch.eye(p.n, dtype=torch.float64, device=ski.device)
    Pinv = _host(ski.precond_apply(eye))
    asym = np.abs(Pinv - Pinv.T).max()
    assert asym <= 1e-12 * np.abs(Pinv).max(), (asym, np.abs(Pinv).max())
    rel = np.abs(_host(d) - np.diag(Pinv)) / np.abs(np.diag(Pinv))
    print('precond diag: max relative difference %.3e' % rel.max())
    assert rel.max() <= 1e-10, rel.max()
    # P is a preconditioner, not the inverse: the diagonal differs from K~^-1's
    ref = np.diag(la.inv(_dense_spd(op, p.n)))
    assert np.abs(_host(d) - ref).max() > 1e-6 * ref.max()
    # (the 96 functions want a grid of 768 points: check_precond_hi's size)
    with _env_set(RUNLMC_PRECOND_HI_MIN=0):
        p, fk, K, gk, spec, op = _synth_problem_and_oracle(2, 2, 1000, 'matern')
        ski = K.device_operator()
        ok = ski.factor()[0]
    assert ok and ski.factor_mode == 3, (ski.factor_mode, ski.factor_reason)
    try:
        ski.inverse_diag()
    except NotImplementedError as e:
        assert '96-function basis' in str(e) and 'blocks' in str(e), str(e)
    else:
        raise AssertionError('inverse_diag answered on the 96-function basis')
    rng = np.random.RandomState(3)
    B = torch.from_numpy(rng.randn(3, p.n)).to(ski.device)
    Z = ski.precond_apply(B)
    Qv = ski.mvm(Z)
    b, z, q = _host(B), _host(Z), _host(Qv)
    a = np.einsum('ij,ij->i', b, z) / np.einsum('ij,ij->i', z, q)
    X1, it, res, st = solve_pcg(ski, B, tol=1e-300, maxiter=1)
    assert np.all(it == 1), it
    x1 = a[:, None] * z
    assert np.abs(_host(X1) - x1).max() <= 1e-12 * np.abs(x1).max()
    r1 = np.linalg.norm(b - a[:, None] * q, axis=1)
    assert np.abs(res - r1).max() <= 1e-10 * r1.max(), (res, r1)
    return rel.max()


# --- 4. the accumulation kernel --------------------------------------------------------------------
def check_diag_accumulate():
    """rl_diag_accumulate against NumPy at 1e-13 relative, with and without C, and the same bits
    whatever tiles the rows come in (1, 7, all)."""
    lib = _lib.get_library()
    dev = lib.torch_device()
    rng = np.random.RandomState(41)
    for nvec, n in ((1, 1), (7, 255), (33, 1025)):
        Z = rng.randint(0, 2, (nvec, n)) * 2.0 - 1.0
        X, C = rng.randn(nvec, n), rng.randn(nvec, n)
        s0, q0 = rng.randn(n), np.abs(rng.randn(n))
        tZ, tX, tC = (torch.from_numpy(a).to(dev) for a in (Z, X, C))
        for withC in (True, False):
            t = Z * (X - C) if withC else Z * X
            got = {}
            for tile in (1, 7, nvec):
                s, q = torch.from_numpy(s0.copy()).to(dev), torch.from_numpy(q0.copy()).to(dev)
                for v0 in range(0, nvec, tile):
                    sl = slice(v0, min(v0 + tile, nvec))
                    diag_accumulate(lib, tZ[sl].contiguous(), tX[sl].contiguous(),
                                    tC[sl].contiguous() if withC else None, s, q)
                got[tile] = (_host(s), _host(q))
            s, q = got[nvec]
            rs, rq = s0 + t.sum(axis=0), q0 + (t * t).sum(axis=0)
            scale_s = np.abs(s0) + np.abs(t).sum(axis=0)
            assert np.all(np.abs(s - rs) <= 1e-13 * scale_s), np.abs(s - rs).max()
            assert np.all(np.abs(q - rq) <= 1e-13 * rq), np.abs(q - rq).max()
            for tile in (1, 7):
                assert np.array_equal(got[tile][0], s) and np.array_equal(got[tile][1], q), (tile, nvec, n)


# --- 5. the probe estimator ------------------------------------------------------------------------
def _probe_case(which):
    """(K, ski, dense K~ of the oracle, smallest noise) of the three operators of checks 5 and 6."""
    if which == 'direct':
        p, fk, K, gk, spec, op = _synth_problem_and_oracle(3, 2, 120, 'rbf')
        return K, _dense_spd(op, p.n), p.noise.min(), (p, gk)
    if which == 'precond':
        with _env_set(RUNLMC_PRECOND_HI_MIN=0, RUNLMC_NO_PRECOND_HI=1):
            p, fk, K, gk, spec, op = _synth_problem_and_oracle(2, 2, 150, 'matern')
            K.device_operator().factor()
        return K, _dense_spd(op, p.n), p.noise.min(), (p, gk)
    c = Case('lmc_2d')
    fk, K, gk = build_operator(c)
    return K, _dense_pieces(c)[2], c.noise.min(), (c, gk)


def check_probes_estimator(which):
    """method='probes' with 16 host-supplied +-1 rows and solves at 1e-10 against the dense
    restatement on the SAME probes: |delta d_i| <= tol / eps_min (a residual r moves x by at most
    ||K~^-1||_2 ||r|| <= tol / eps_min, and every term is one such entry times +-1); the standard
    error moves by at most ||delta t||_2 / sqrt(k (k - 1)) <= that.  No statistical assertion."""
    K, Kd, eps_min, keep = _probe_case(which)
    ski = K.device_operator()
    n, k = ski.n, 16
    ski.factor()
    assert ski.factor_mode == dict(direct=1, precond=2, grid2d=0)[which], (ski.factor_mode, ski.factor_reason)
    rng = np.random.RandomState(77)
    Z = rng.randint(0, 2, (k, n)) * 2.0 - 1.0
    with _tight_krylov():
        res = loo.inverse_diagonal(K, method='probes', probes=Z, batch=5, tol=SOLVE_TOL)
    assert res.method == 'probes' and res.stats.n_probes == k
    assert res.stats.control_variate == (which != 'grid2d')
    assert np.all(res.stats.residuals < SOLVE_TOL), res.stats.residuals.max()
    Kinv = la.inv(Kd)
    X = Z @ Kinv
    if which == 'grid2d':
        d0, T = np.zeros(n), Z * X
    else:
        Pinv = _host(ski.precond_apply(torch.eye(n, dtype=torch.float64, device=ski.device)))
        Pinv = 0.5 * (Pinv + Pinv.T)
        d0, T = np.diag(Pinv), Z * (X - Z @ Pinv)
    d_ref = d0 + T.mean(axis=0)
    sem_ref = T.std(axis=0, ddof=1) / np.sqrt(k)
    bound = SOLVE_TOL / eps_min
    ed, es = np.abs(_host(res.d) - d_ref).max(), np.abs(_host(res.sem) - sem_ref).max()
    print('probes %s: |delta d| %.3e, |delta sem| %.3e, bound %.3e' % (which, ed, es, bound))
    assert ed <= bound and es <= bound, (ed, es, bound)
    if which == 'direct':
        # the control variate IS the answer: the estimate equals the dense diagonal for any probes
        assert np.abs(_host(res.d) - np.diag(Kinv)).max() <= bound
    # device-drawn probes: +-1, a function of (seed, v) only -- tiles of 3 and of 16 give the same bits
    with _tight_krylov():
        a = loo.inverse_diagonal(K, method='probes', n_probes=6, seed=9, batch=3, tol=SOLVE_TOL)
        b = loo.inverse_diagonal(K, method='probes', n_probes=6, seed=9, batch=16, tol=SOLVE_TOL)
    P6 = _host(loo.device_probes(ski.lib, 9, 0, 6, n, ski.device))
    assert np.all(np.abs(P6) == 1.0) and abs(P6.mean()) < 0.2
    assert np.array_equal(_host(loo.device_probes(ski.lib, 9, 2, 3, n, ski.device)), P6[2:5])
    assert np.abs(_host(a.d) - _host(b.d)).max() <= 2 * bound
    return ed, es


# --- 6. a subset by solves -------------------------------------------------------------------------
def check_solve_subset(which):
    """method='solve' (UnitRows through quad_forms) on rows 0, n - 1, both sides of every output
    border and five random ones, in tiles of 1, 7 and everything: <= tol / eps_min from the dense
    inverse; bad indices raise ValueError."""
    K, Kd, eps_min, (c, gk) = _probe_case(which)
    ski = K.device_operator()
    n = ski.n
    ends = np.cumsum(c.lens)[:-1]
    rng = np.random.RandomState(5)
    idx = np.concatenate([[0, n - 1], ends - 1, ends, rng.randint(0, n, 5)])
    ref = np.diag(la.inv(Kd))[idx]
    bound = SOLVE_TOL / eps_min
    for batch in (1, 7, 10 ** 6):
        with _tight_krylov():
            res = loo.inverse_diagonal(K, method='solve', indices=idx, batch=batch, tol=SOLVE_TOL)
        assert res.method == 'solve' and res.sem == 0.0 and len(res.stats.v) == len(idx)
        assert np.all(res.stats.residuals < SOLVE_TOL), res.stats.residuals.max()
        err = np.abs(_host(res.d) - ref).max()
        print('solve subset %s batch %d: %.3e, bound %.3e' % (which, batch, err, bound))
        assert err <= bound, (err, bound)
    # the row source on its own, all rows
    rows = UnitRows(n, None, ski.device)
    E = _host(rows.fill(3, 4))
    assert E.shape == (4, n) and np.array_equal(E, np.eye(n)[3:7])
    for bad in ([n], [-1], [0.5], [True], np.array([1.0])):
        for call in (lambda: loo.inverse_diagonal(K, method='solve', indices=bad),
                     lambda: UnitRows(n, bad, ski.device)):
            try:
                call()
            except ValueError:
                pass
            else:
                raise AssertionError('indices %r accepted' % (bad,))
    with _tight_krylov():
        auto = loo.inverse_diagonal(K, indices=idx[:3], tol=SOLVE_TOL)
    assert auto.method == 'solve'


# --- 7. the model ------------------------------------------------------------------------------------
def _loo_model(c, normalize=False):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    fk = functional_kernel_for(c)
    Xs = [np.asarray(x).reshape(len(x), c.P) for x in c.Xs]
    m = [len(a) - 4 for a in c.grid_axes]
    np.random.seed(5)
    model = InterpolatedLLGP(Xs, c.Ys, normalize=normalize, m=m, functional_kernel=fk,
                             trace_iterations=2, tolerance=1e-12)
    np.testing.assert_allclose(model.dists[c.ad], c.grid_dists, rtol=0, atol=1e-12)
    with _tight_krylov():
        model._ensure()
    return model


def check_model_loo(name, normalize=False):
    """loo_predict / loo_log_likelihood of a model against the dense formulas on the oracle's K~
    and, for five rows, against the prediction from the dense K~ with the row and column deleted.
    Means at 1e-8 max|y|, variances at delta_d / d^2 with check 1's delta_d = 1e-9 max(1 / eps);
    the log likelihood at the first-order sum of both (delta_alpha = 1e-9 max|alpha|, the bound
    check_direct_solve holds alpha to)."""
    c = Case(name)
    model = _loo_model(c, normalize)
    Kd = _dense_pieces(c)[2]
    lens = c.lens
    y_raw = np.hstack(c.Ys)
    if normalize:
        sd = np.repeat([np.std(Y) for Y in c.Ys], lens)
        mu = np.repeat([np.mean(Y) for Y in c.Ys], lens)
    else:
        sd, mu = np.ones(c.n), np.zeros(c.n)
    y = (y_raw - mu) / sd
    Kinv = la.inv(Kd)
    alpha, d = Kinv @ y, np.diag(Kinv)
    mean_ref, var_ref = (y - alpha / d) * sd + mu, sd ** 2 / d
    logp_ref = np.sum(-0.5 * np.log(2 * np.pi / d) - 0.5 * alpha ** 2 / d - np.log(sd))
    dd = DIAG_REL * np.max(1.0 / c.noise)
    da = 1e-9 * np.abs(alpha).max()
    mean_tol = 1e-8 * np.abs(y_raw).max()
    var_tol = dd / d ** 2 * sd ** 2
    logp_tol = np.sum(0.5 * dd / d + np.abs(alpha) * da / d + 0.5 * alpha ** 2 * dd / d ** 2)
    # the dense formulas themselves: five rows by deleting the row and column
    rng = np.random.RandomState(2)
    five = rng.choice(c.n, 5, replace=False)
    for i in five:
        keep = np.delete(np.arange(c.n), i)
        sol = la.solve(Kd[np.ix_(keep, keep)], np.column_stack([y[keep], Kd[keep, i]]), assume_a='pos')
        bm, bv = Kd[i, keep] @ sol[:, 0], Kd[i, i] - Kd[i, keep] @ sol[:, 1]
        assert abs(bm * sd[i] + mu[i] - mean_ref[i]) <= mean_tol and abs(bv * sd[i] ** 2 - var_ref[i]) <= var_tol[i]
    direct = name == 'lmc_smooth'
    if direct:
        calls = []
        saved = Iterative.solve_device

        def counting(*a, **kw):
            calls.append(1)
            return saved(*a, **kw)
        Iterative.solve_device = staticmethod(counting)
        try:
            means, vars_ = model.loo_predict(method='direct')
            ll = model.loo_log_likelihood(method='direct')
        finally:
            Iterative.solve_device = staticmethod(saved)
        assert not calls, 'method=direct made %d solves' % len(calls)
        assert model.loo_stats['method'] == 'direct' and model.loo_stats['nonpositive'] == 0
        assert model.loo_stats['sem'] == 0.0
        assert [len(v) for v in means] == lens and [len(v) for v in vars_] == lens
        means, vars_ = np.concatenate(means), np.concatenate(vars_)
        a_means, a_vars = model.loo_predict()
        assert model.loo_stats['method'] == 'direct'
        assert np.array_equal(np.concatenate(a_means), means) and np.array_equal(np.concatenate(a_vars), vars_)
        sel = slice(None)
        ll_ref, ll_tol = logp_ref, logp_tol
    else:
        ends = np.cumsum(lens)[:-1]
        sel = np.concatenate([[0, c.n - 1], ends - 1, ends, five])
        with _tight_krylov():
            means, vars_ = model.loo_predict(indices=sel, tol=1e-12)
            used = model.loo_stats['method']
            ll = model.loo_log_likelihood(indices=sel, tol=1e-12)
        assert used == 'solve' and model.loo_stats['method'] == 'solve', used
        assert np.all(model.loo_stats['stats'].residuals < 1e-12)
        assert means.shape == (len(sel),) and vars_.shape == (len(sel),)
        terms = -0.5 * np.log(2 * np.pi / d) - 0.5 * alpha ** 2 / d - np.log(sd)
        ll_ref = terms[sel].sum()
        ll_tol = np.sum((0.5 * dd / d + np.abs(alpha) * da / d + 0.5 * alpha ** 2 * dd / d ** 2)[sel])
        try:
            model.loo_predict(method='direct')
        except NotImplementedError as e:
            assert 'polynomial form' in str(e), str(e)
        else:
            raise AssertionError("method='direct' answered on a model with a Matern row")
    em, ev = np.abs(means - mean_ref[sel]).max(), np.abs(vars_ - var_ref[sel]) / var_tol[sel]
    print('model loo %s normalize=%s: mean error %.3e (tol %.3e), variance error / tol %.3e, '
          'log likelihood error %.3e (tol %.3e)' % (name, normalize, em, mean_tol, ev.max(),
                                                    abs(ll - ll_ref), ll_tol))
    assert em <= mean_tol, (em, mean_tol)
    assert ev.max() <= 1.0, ev.max()
    assert abs(ll - ll_ref) <= ll_tol, (ll, ll_ref, ll_tol)
    # observations, not the latent function: the noise is inside the variance
    noise_rows = np.repeat(c.noise, lens) * sd ** 2
    assert np.all(vars_ > noise_rows[sel])
    return em, ev.max()


# --- 8. the reduction --------------------------------------------------------------------------------
def check_loo_reduce():
    """rl_loo_reduce: the per-row formulas, the same bits from call to call, rows with d = 0 and
    d < 0 counted and reported (NaN, out of the sum) with every other row untouched; the model logs
    such rows once at CRITICAL."""
    lib = _lib.get_library()
    dev = lib.torch_device()
    rng = np.random.RandomState(8)
    for n in (1, 300, 2500):
        y, alpha, ls = rng.randn(n), rng.randn(n), 0.3 * rng.randn(n)
        d = np.abs(rng.randn(n)) + 0.05
        ty, ta, td, tl = (torch.from_numpy(a).to(dev) for a in (y, alpha, d, ls))
        mean, var, logp, bad = loo_reduce(lib, ty, ta, td, tl)
        assert bad == 0
        mr, vr = y - alpha / d, 1.0 / d
        lp = -0.5 * np.log(2 * np.pi * vr) - (y - mr) ** 2 / (2 * vr) - ls
        assert np.all(np.abs(_host(mean) - mr) <= 1e-13 * (np.abs(y) + np.abs(alpha / d)))
        assert np.all(np.abs(_host(var) - vr) <= 1e-13 * vr)
        assert abs(logp - lp.sum()) <= 1e-13 * np.abs(lp).sum()
        again = loo_reduce(lib, ty, ta, td, tl)
        assert again[2] == logp and np.array_equal(_host(again[0]), _host(mean))
        assert abs(loo_reduce(lib, ty, ta, td, None)[2] - (lp + ls).sum()) <= 1e-13 * np.abs(lp + ls).sum()
        if n < 3:
            continue
        d2 = d.copy()
        i0, i1 = n // 3, n - 2
        d2[i0], d2[i1] = 0.0, -0.4
        m2, v2, logp2, bad2 = loo_reduce(lib, ty, ta, torch.from_numpy(d2).to(dev), tl)
        assert bad2 == 2
        m2, v2 = _host(m2), _host(v2)
        assert np.all(np.isnan(m2[[i0, i1]])) and np.all(np.isnan(v2[[i0, i1]]))
        rest = np.delete(np.arange(n), [i0, i1])
        assert np.array_equal(m2[rest], _host(mean)[rest]) and np.array_equal(v2[rest], _host(var)[rest])
        assert abs(logp2 - lp[rest].sum()) <= 1e-13 * np.abs(lp).sum()
        for extra in (np.inf, np.nan):
            d3 = d.copy()
            d3[0] = extra
            assert loo_reduce(lib, ty, ta, torch.from_numpy(d3).to(dev), tl)[3] == 1
    # the model: one CRITICAL record, the count in loo_stats, NaN where d is not positive
    c = Case('lmc_smooth')
    model = _loo_model(c)
    records = []

    class Grab(logging.Handler):
        def emit(self, record):
            records.append(record)
    log = logging.getLogger('runlmc_amd.models.interpolated_llgp')
    grab = Grab(level=logging.CRITICAL)
    log.addHandler(grab)
    real = loo.inverse_diagonal

    def spoiled(*a, **kw):
        r = real(*a, **kw)
        dbad = r.d.clone()
        dbad[4], dbad[200] = 0.0, -1.0
        return r._replace(d=dbad)
    loo.inverse_diagonal = spoiled
    try:
        means, vars_ = model.loo_predict(method='direct')
    finally:
        loo.inverse_diagonal = real
        log.removeHandler(grab)
    assert len(records) == 1 and records[0].levelno == logging.CRITICAL, records
    assert model.loo_stats['nonpositive'] == 2
    flat = np.concatenate(means)
    assert np.isnan(flat[4]) and np.isnan(flat[200]) and np.isfinite(np.delete(flat, [4, 200])).all()


# --- 9. argument errors --------------------------------------------------------------------------
def check_abi_errors():
    """NULL pointers, negative counts and forbidden aliasing are RL_EINVAL -> ValueError."""
    lib = _lib.get_library()
    dev = lib.torch_device()
    assert lib.cdll.rl_abi_version() == _lib.ABI_VERSION == 8
    c = Case('lmc_smooth')
    fk, K, gk = build_operator(c)
    ski = K.device_operator()
    n = ski.n
    buf = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(6)]
    ptr = [ctypes.c_void_p(b.data_ptr()) for b in buf]
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(0)
    ex, nb = ctypes.c_int(), ctypes.c_int()
    bad = [
        ('rl_ski_inverse_diag', (null, ptr[0], ctypes.byref(ex), st)),
        ('rl_ski_inverse_diag', (ski.handle, null, ctypes.byref(ex), st)),
        ('rl_ski_inverse_diag', (ski.handle, ptr[0], None, st)),
        ('rl_ski_precond_apply', (null, ptr[0], ptr[1], 1, st)),
        ('rl_ski_precond_apply', (ski.handle, null, ptr[1], 1, st)),
        ('rl_ski_precond_apply', (ski.handle, ptr[0], null, 1, st)),
        ('rl_ski_precond_apply', (ski.handle, ptr[0], ptr[1], -1, st)),
        ('rl_ski_precond_apply', (ski.handle, ptr[0], ptr[0], 1, st)),
        ('rl_diag_accumulate', (null, ptr[1], null, 1, n, ptr[2], ptr[3], st)),
        ('rl_diag_accumulate', (ptr[0], null, null, 1, n, ptr[2], ptr[3], st)),
        ('rl_diag_accumulate', (ptr[0], ptr[1], null, 1, n, null, ptr[3], st)),
        ('rl_diag_accumulate', (ptr[0], ptr[1], null, 1, n, ptr[2], null, st)),
        ('rl_diag_accumulate', (ptr[0], ptr[1], null, -1, n, ptr[2], ptr[3], st)),
        ('rl_diag_accumulate', (ptr[0], ptr[1], null, 1, 0, ptr[2], ptr[3], st)),
        ('rl_diag_accumulate', (ptr[0], ptr[1], null, 1, n, ptr[2], ptr[2], st)),
        ('rl_loo_reduce', (null, ptr[1], ptr[2], null, n, ptr[3], ptr[4], ptr[5], ctypes.byref(nb), st)),
        ('rl_loo_reduce', (ptr[0], null, ptr[2], null, n, ptr[3], ptr[4], ptr[5], ctypes.byref(nb), st)),
        ('rl_loo_reduce', (ptr[0], ptr[1], null, null, n, ptr[3], ptr[4], ptr[5], ctypes.byref(nb), st)),
        ('rl_loo_reduce', (ptr[0], ptr[1], ptr[2], null, n, null, ptr[4], ptr[5], ctypes.byref(nb), st)),
        ('rl_loo_reduce', (ptr[0], ptr[1], ptr[2], null, n, ptr[3], null, ptr[5], ctypes.byref(nb), st)),
        ('rl_loo_reduce', (ptr[0], ptr[1], ptr[2], null, n, ptr[3], ptr[4], null, ctypes.byref(nb), st)),
        ('rl_loo_reduce', (ptr[0], ptr[1], ptr[2], null, n, ptr[3], ptr[4], ptr[5], None, st)),
        ('rl_loo_reduce', (ptr[0], ptr[1], ptr[2], null, 0, ptr[3], ptr[4], ptr[5], ctypes.byref(nb), st)),
        ('rl_loo_reduce', (ptr[0], ptr[1], ptr[2], null, -5, ptr[3], ptr[4], ptr[5], ctypes.byref(nb), st)),
        ('rl_loo_reduce', (ptr[0], ptr[1], ptr[2], null, n, ptr[3], ptr[3], ptr[5], ctypes.byref(nb), st)),
        ('rl_loo_reduce', (ptr[0], ptr[1], ptr[2], null, n, ptr[2], ptr[4], ptr[5], ctypes.byref(nb), st)),
    ]
    for name, args in bad:
        try:
            lib.call(name, *args)
        except ValueError as e:
            assert name in str(e), (name, str(e))
        else:
            raise AssertionError('%s%r accepted' % (name, args))
    # zero vectors: nothing to do, no error
    lib.call('rl_ski_precond_apply', ski.handle, ptr[0], ptr[1], 0, st)
    lib.call('rl_diag_accumulate', ptr[0], ptr[1], null, 0, n, ptr[2], ptr[3], st)
    # the Python front ends
    for call in (lambda: loo.inverse_diagonal(K, method='exact'),
                 lambda: loo.inverse_diagonal(K, batch=0),
                 lambda: loo.inverse_diagonal(K, method='probes', probes=np.ones((2, n + 1))),
                 lambda: loo.inverse_diagonal(K, method='probes', probes=np.full((2, n), 0.5)),
                 lambda: loo.inverse_diagonal(K, method='probes', n_probes=0),
                 lambda: ski.precond_apply(torch.zeros((2, n + 1), dtype=torch.float64, device=dev)),
                 lambda: diag_accumulate(lib, buf[0][None], buf[1][None], None, buf[2][:-1], buf[3])):
        try:
            call()
        except ValueError:
            pass
        else:
            raise AssertionError('bad argument accepted')
