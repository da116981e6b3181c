"""The pivoted-Cholesky preconditioner P = L L^T + diag(eps) (csrc/rl_pivchol.h;
rl_ski_set_pivchol, InterpolatedLLGP(precond_rank=...)): build, apply, log det, sample map,
solves, the model, updates and refusals.

Shared by the GPU run (tests/test_pivchol_gpu.py, librunlmc_hip.so on an MI355X) and the CPU
run (tests/test_pivchol_emu.py, the same kernel source under the thread-level emulator, small
problems and low ranks).  Every function uses whichever native library is active.

Operators (the dense K~ of each comes from the suite that owns the problem; another noise level
is Kd - diag(eps_old) + diag(eps_new)):
  (a) 'sep2d'   separable_suite._model_case: n = 297, two inputs, 24 x 20 grid, RBF-ARD + Matern
  (b) 'grid3d'  grid3d_suite._case('mix'): the tricubic problem ('full' on the device, 'small'
                under the emulator)
  (c) 'terms'   grid3d_suite.check_two_terms' operator: a 3-D term beside a 1-D term
  (d) 'wide'    a 1-D operator with D = 17 outputs of 19 rows each (n = 323), the route of "more
                than 16 outputs", built here
Inputs are random, so every handle's internal row order is a permutation of the caller's
(`permuted_rows` asserts it on each).

References.  The factor is held to a np.longdouble pivoted Cholesky of Kd - diag(eps) run WITH
THE DEVICE'S PIVOTS (ties cannot flip the comparison); apply, log det and sample map to dense
linear algebra on P = L_dev L_dev^T + E.  Bars: 10 REL d0 for the factor (REL = 1e-11 the
products' own bar, d0 the largest initial diagonal; Cholesky is backward stable), 1e-9 of
max|x| for the apply (parity_suite.check_direct_solve's bar of the Woodbury apply), 1e-10
relative for log det P, 1e-9 max|P| for S S^T.

Iteration counts of the low-noise variant of (a) (eps = 1e-3 on both outputs, right-hand side y,
||r|| < 1e-8, rank 64), NumPy on the dense matrix with the reference factor: CG 738, PCG 80
(rank 32: 185, rank 128: 31; check_iteration_gain asserts the quarter at rank 64); the device's own counts are in
profiles/pivchol/README.md.
"""
import contextlib
import functools
import types

import numpy as np
import scipy.linalg as la
import torch

import grid2d_suite as g2
import grid3d_suite as g3
import loo_suite
import separable_suite as sep
from separable_suite import _raises

from oracle import interp as ointerp
from oracle.kernels import RBFSpec, Matern32Spec

from runlmc_amd.kern import RBF, Matern32
from runlmc_amd.lmc.functional_kernel import FunctionalKernel

REL = g2.REL
RANKS = (1, 5, 16, 37, 64)
NVECS = (1, 3, 17, 33)
LOW_NOISE = 1e-3


def _say(name, **vals):
    print('pivchol %s: %s' % (name, '  '.join('%s %.3g' % kv for kv in vals.items())), flush=True)


class _Op:
    """An operator under test: the model that owns the handle, the handle, the dense kernel
    part Kk = Kd - diag(eps) and the noise per row."""

    def __init__(self, name, model, Kd, eps_rows, lens, noise):
        self.name, self.model = name, model
        self.K = model._K
        self.ski = model._K.device_operator()
        self.n = Kd.shape[0]
        self.Kk = Kd - np.diag(eps_rows)
        self.eps = np.array(eps_rows, dtype=float)
        self.lens, self.noise = list(lens), np.array(noise, dtype=float)

    def set_noise(self, noise):
        self.noise = np.array(noise, dtype=float)
        self.eps = np.repeat(self.noise, self.lens)
        self.K.update_noise(self.noise, self.lens)

    @property
    def Kd(self):
        return self.Kk + np.diag(self.eps)


def _dev(op, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(op.ski.device)


# --- the operators -----------------------------------------------------------------------------
def _sep_model(precond_rank=0, tolerance=1e-4, variance_batch=None):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    c = sep._model_case()
    fk = FunctionalKernel(D=c.D, lmc_kernels=sep._kernels(), lmc_ranks=[1, 1])
    fk.coreg_vecs, fk.coreg_diags, fk.noise = c.A, c.kappa, c.noise
    np.random.seed(5)
    return InterpolatedLLGP(c.Xs, c.Ys, normalize=False, m=[20, 16], functional_kernel=fk,
                            trace_iterations=4, tolerance=tolerance, variance_batch=variance_batch,
                            precond_rank=precond_rank)


def _g3_model(kind='mix', precond_rank=0, tolerance=1e-4, variance_batch=None, kerns=None):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    c = g3._case(kind)
    kerns = g3.KERNEL_SETS[kind][0]() if kerns is None else kerns
    fk = FunctionalKernel(D=c.D, lmc_kernels=kerns, lmc_ranks=[1] * len(kerns))
    fk.coreg_vecs, fk.coreg_diags, fk.noise = c.A, c.kappa, c.noise
    np.random.seed(5)
    return InterpolatedLLGP(c.Xs, c.Ys, normalize=False, m=c.spec['m'], functional_kernel=fk,
                            trace_iterations=4, tolerance=tolerance, variance_batch=variance_batch,
                            precond_rank=precond_rank)


def _two_term_model(precond_rank=0):
    """grid3d_suite.check_two_terms' construction and its dense operator."""
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    c = g3._case('iso')
    rng = np.random.RandomState(21)
    A = c.A + [rng.uniform(-1, 1, size=(1, c.D))]
    kappa = c.kappa + [0.2 + rng.rand(c.D)]
    fk = FunctionalKernel(D=c.D, lmc_kernels=[RBF(g3.RB, active_dims=[0, 1, 2]),
                                              Matern32(g3.M32, active_dims=[0])], lmc_ranks=[1, 1])
    fk.coreg_vecs, fk.coreg_diags, fk.noise = A, kappa, c.noise
    np.random.seed(5)
    model = InterpolatedLLGP(c.Xs, c.Ys, normalize=False, m=c.spec['m'], functional_kernel=fk,
                             trace_iterations=4, precond_rank=precond_rank)
    model._ensure()
    ax = model.grid_axes[(0,)][0]
    m1 = len(ax)
    W1 = np.zeros((c.n, c.D * m1))
    start = 0
    for d, X in enumerate(c.Xs):
        W1[start:start + len(X), d * m1:(d + 1) * m1] = ointerp.cubic_rows(ax, X[:, 0])
        start += len(X)
    B1 = A[1].T @ A[1] + np.diag(kappa[1])
    K1 = W1 @ np.kron(B1, la.toeplitz(Matern32Spec(g3.M32).from_dist(ax - ax[0]))) @ W1.T
    return model, c.Kd + 0.5 * (K1 + K1.T)


class _WideModel:
    """The little of a model that _Op needs, around a hand-built 1-D operator with D = 17."""

    def __init__(self):
        from runlmc_amd.lmc.grid_kernel import gen_grid_kernel
        from runlmc_amd.approx.interpolation import multi_interpolant, autogrid
        rng = np.random.RandomState(17)
        D, per = 17, 19
        self.lens = [per] * D
        Xs = [rng.rand(per, 1) for _ in range(D)]
        kerns = [RBF(30.0), Matern32(8.0)]
        fk = FunctionalKernel(D=D, lmc_kernels=kerns, lmc_ranks=[1, 1])
        self.A = [rng.uniform(-1, 1, size=(1, D)) for _ in range(2)]
        self.kappa = [0.2 + rng.rand(D) for _ in range(2)]
        self.noise = 0.05 + 0.1 * rng.rand(D)
        fk.coreg_vecs, fk.coreg_diags, fk.noise = self.A, self.kappa, self.noise
        fk.set_input_dim(1)
        (ax,) = autogrid(Xs, None, None, np.array([40]))
        dists = ax - ax[0]
        W = multi_interpolant(Xs, ax)
        self.interpolants = {(0,): (W, W.T.tocsr())}
        self._K, _ = gen_grid_kernel(fk, {(0,): dists}, self.interpolants, self.lens)
        m = len(ax)
        Wd = np.zeros((D * per, D * m))
        for d, X in enumerate(Xs):
            Wd[d * per:(d + 1) * per, d * m:(d + 1) * m] = ointerp.cubic_rows(ax, X[:, 0])
        Bs = [a.T @ a + np.diag(k) for a, k in zip(self.A, self.kappa)]
        tops = [la.toeplitz(RBFSpec(30.0).from_dist(dists)), la.toeplitz(Matern32Spec(8.0).from_dist(dists))]
        Kk = Wd @ sum(np.kron(B, T) for B, T in zip(Bs, tops)) @ Wd.T
        self.Kd = 0.5 * (Kk + Kk.T) + np.diag(np.repeat(self.noise, self.lens))
        self.y = rng.randn(D * per)


@functools.lru_cache(maxsize=None)
def operator(name):
    """The operator `name`, built once (its handle is shared by the checks, each of which sets
    the rank -- and restores the noise -- it works with)."""
    if name == 'sep2d':
        c = sep._model_case()
        model = _sep_model()
        model._ensure()
        op = _Op(name, model, c.Kd, np.repeat(c.noise, c.lens), c.lens, c.noise)
        op.y = c.y
    elif name == 'grid3d':
        c = g3._case('mix')
        model = _g3_model()
        model._ensure()
        op = _Op(name, model, c.Kd, np.repeat(c.noise, c.lens), c.lens, c.noise)
        op.y = c.y
    elif name == 'terms':
        c = g3._case('iso')
        model, Kd = _two_term_model()
        op = _Op(name, model, Kd, np.repeat(c.noise, c.lens), c.lens, c.noise)
        op.y = c.y
    elif name == 'wide':
        w = _WideModel()
        op = _Op(name, w, w.Kd, np.repeat(w.noise, w.lens), w.lens, w.noise)
        op.y = w.y
    else:
        raise KeyError(name)
    got = op.K.matmat(np.identity(op.n))
    err = np.abs(got - op.Kd).max() / np.abs(op.Kd).max()
    assert err <= REL, (name, err)
    return op


def permuted_rows(op):
    """The handle's internal row order (rows sorted by their first grid column, rl_ski_create) is
    not the caller's: the first columns of the first term's W, in the caller's order, descend
    somewhere -- so every readout below goes through the un-permutation."""
    W = list(op.model.interpolants.values())[0][0].tocsr()
    first = W.indices[W.indptr[:-1]]
    assert np.any(np.diff(first) < 0), 'rows are sorted: the handle is not permuted'


def mode4(op, rank, rel_tol=1e-10):
    op.ski.set_pivchol(rank, rel_tol)
    ok, ld, cond = op.ski.factor()
    assert ok and op.ski.factor_mode == 4 and ld == 0.0 and cond >= 1.0, (ok, op.ski.factor_mode, ld, cond)
    return cond


# --- references --------------------------------------------------------------------------------
def ref_factor(Kk, pivots):
    """np.longdouble pivoted Cholesky with given pivots: (L [k][n], the residual diagonal BEFORE
    each step [k][n], the one after the last)."""
    A = np.asarray(Kk, dtype=np.longdouble)
    n = len(A)
    d = np.diag(A).copy()
    L = np.zeros((len(pivots), n), dtype=np.longdouble)
    before = []
    for j, p in enumerate(pivots):
        before.append(d.copy())
        if not d[p] > 0:
            break
        l = (A[p] - L[:j, p] @ L[:j]) / np.sqrt(d[p])
        L[j] = l
        d = d - l * l
    return L, before, d


def np_pivchol(Kk, rank, rel_tol):
    """Greedy pivoted Cholesky in float64 with the early stop: (L [used][n], pivots)."""
    A = np.asarray(Kk, dtype=float)
    d = np.diag(A).copy()
    d0 = d.max()
    L = np.zeros((0, len(A)))
    piv = []
    for _ in range(min(rank, len(A))):
        p = int(np.argmax(d))
        if not d[p] > rel_tol * d0:
            break
        l = (A[p] - L[:, p] @ L) / np.sqrt(d[p])
        l[piv] = 0.0
        L = np.vstack([L, l])
        piv.append(p)
        d = np.maximum(d - l * l, 0.0)
        d[piv] = 0.0
    return L, piv


def np_pcg(K, b, Minv, tol, maxiter=20000):
    """Iterations of (preconditioned) conjugate gradients to ||r|| < tol on a dense matrix."""
    x = np.zeros_like(b)
    r = b.copy()
    z = Minv(r)
    p = z.copy()
    rz = r @ z
    for it in range(1, maxiter + 1):
        q = K @ p
        a = rz / (p @ q)
        x += a * p
        r -= a * q
        if np.linalg.norm(r) < tol:
            return it
        z = Minv(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return maxiter


# --- 1, 2: diagonal and factor -----------------------------------------------------------------
def check_diagonal(name):
    op = operator(name)
    permuted_rows(op)
    mode4(op, 1)
    used, piv, val, resid = op.ski.pivchol_info()
    L = op.ski.pivchol_factor().cpu().numpy()
    assert used == 1 and L.shape == (1, op.n)
    d = resid.cpu().numpy() + L[0] ** 2
    want = np.diag(op.Kk)
    d0 = want.max()
    err = np.abs(d - want).max()
    _say('diagonal (%s)' % name, err=err, bar=10 * REL * d0)
    assert err <= 10 * REL * d0, err
    assert piv[0] == int(np.argmax(want)) or abs(want[piv[0]] - d0) <= 10 * REL * d0
    assert abs(val[0] - want[piv[0]]) <= 10 * REL * d0


def check_factor(name, rank):
    op = operator(name)
    mode4(op, rank)
    used, piv, val, resid = op.ski.pivchol_info()
    k = min(rank, op.n)
    assert len(piv) == k and 1 <= used <= k, (used, k)
    L = op.ski.pivchol_factor().cpu().numpy()
    assert L.shape == (used, op.n)
    resid = resid.cpu().numpy()
    d0 = np.diag(op.Kk).max()
    bar = 10 * REL * d0
    pu = piv[:used]
    assert len(set(pu.tolist())) == used, 'a pivot row was chosen twice'
    e_rows = float(np.abs(op.Kk[pu] - (L.T @ L)[pu]).max())
    for j in range(used):
        assert np.all(L[j, pu[:j]] == 0.0), (j, L[j, pu[:j]])
    want_resid = np.diag(op.Kk) - (L ** 2).sum(axis=0)
    e_res = float(np.abs(resid - want_resid).max())
    assert np.all(resid >= 0.0), resid.min()
    Lr, before, after = ref_factor(op.Kk, pu)
    gap = max(float(b.max() - b[p]) for b, p in zip(before, pu))
    e_val = max(abs(float(b[p]) - v) for b, p, v in zip(before, pu, val))
    e_L = float(np.abs(Lr - L).max())
    _say('factor (%s, rank %d, used %d)' % (name, rank, used), pivot_rows=e_rows, resid=e_res, greedy_gap=gap,
         pivot_values=e_val, factor_vs_longdouble=e_L, bar=bar)
    assert e_rows <= bar and e_res <= bar and gap <= bar and e_val <= bar, (e_rows, e_res, gap, e_val, bar)
    return used


def check_rank_clip():
    """A rank above n is clipped to n."""
    from runlmc_amd._native import GridOp, SkiOp
    from runlmc_amd.approx.interpolation import multi_interpolant
    rng = np.random.RandomState(4)
    D, per, m = 2, 5, 12
    ax = np.linspace(-0.2, 1.2, m)
    Xs = [rng.rand(per, 1) for _ in range(D)]
    W = multi_interpolant(Xs, ax)
    g = GridOp(D, m, 1)
    top = np.exp(-0.5 * 40.0 * (ax - ax[0]) ** 2)
    g.set_lmc(top[None, :], [rng.randn(1, D)], [np.ones(D)])
    s = SkiOp(g, W, W.T.tocsr())
    s.set_noise(np.full(D, 0.1), [per] * D)
    s.set_pivchol(64)
    ok = s.factor()[0]
    assert ok and s.factor_mode == 4, s.factor_reason
    used, piv, val, _ = s.pivchol_info()
    assert len(piv) == D * per and 1 <= used <= D * per, (used, len(piv))
    L = s.pivchol_factor().cpu().numpy()
    Kk = s.matmat_host(np.identity(D * per)) - 0.1 * np.identity(D * per)
    err = np.abs(L.T @ L - Kk).max()
    _say('rank clip (n = 10, rank 64)', used=used, full_rank_err=err)
    if used == D * per:
        assert err <= 1e-9 * np.abs(Kk).max(), err


# --- 3: early stop -----------------------------------------------------------------------------
def check_early_stop():
    """An RBF whose length scale spans the domain (the 'iso' kernel set at inv_lengthscale 0.05) on
    the 3-D problem: numerically of low rank, so the dense float64 pivoted Cholesky stops before
    rank 64 at rel_tol 1e-10 (asserted here first), and so does the device."""
    from separable_suite import _Sep
    c = g3._case('iso')
    GAMMA = 0.05
    Kd = g3._ski_dense(c, [_Sep([(RBFSpec(GAMMA), [0, 1, 2])])])
    eps = np.repeat(c.noise, c.lens)
    Kk = Kd - np.diag(eps)
    Lnp, pnp = np_pivchol(Kk, 64, 1e-10)
    assert len(pnp) < 64, 'the dense pivoted Cholesky does not stop early: %d' % len(pnp)
    model = _g3_model('iso', precond_rank=64, kerns=[RBF(GAMMA, active_dims=[0, 1, 2])])
    model._ensure()
    op = _Op('early', model, Kd, eps, c.lens, c.noise)
    op.y = c.y
    assert op.K.preconditioner is not None and op.ski.factor_mode == 4
    used, piv, val, resid = op.ski.pivchol_info()
    assert used < 64, used
    d0 = np.diag(Kk).max()
    assert np.all(val[used:] <= 1e-10 * d0) and np.all(val[:used] > 1e-10 * d0), val
    L = op.ski.pivchol_factor().cpu().numpy()
    assert L.shape[0] == used
    _say('early stop', used=used, numpy_used=len(pnp), last_pivot=val[used - 1] / d0)
    check_solves(op, rank=64)


# --- 4: apply, log det, sample -----------------------------------------------------------------
def check_apply(name, rank, nvecs=NVECS):
    op = operator(name)
    mode4(op, rank)
    used = op.ski.pivchol_info()[0]
    L = op.ski.pivchol_factor().cpu().numpy()
    P = L.T @ L + np.diag(op.eps)
    assert op.eps.min() >= 1e-2
    rng = np.random.RandomState(rank)
    worst = 0.0
    for nv in nvecs:
        B = rng.randn(nv, op.n)
        X = op.ski.precond_apply(_dev(op, B)).cpu().numpy()
        ref = la.solve(P, B.T, assume_a='pos').T
        worst = max(worst, float(np.abs(X - ref).max() / np.abs(ref).max()))
    S, ld = op.ski.precond_sample(_dev(op, np.identity(op.n)))
    S = S.cpu().numpy().T                      # (column v = S e_v)
    ld_ref = np.linalg.slogdet(P)[1]
    e_ld = abs(ld - ld_ref) / abs(ld_ref)
    e_s = float(np.abs(S @ S.T - P).max() / np.abs(P).max())
    _say('apply (%s, rank %d, used %d)' % (name, rank, used), apply=worst, logdet=e_ld, sample=e_s)
    assert worst <= 1e-9 and e_ld <= 1e-10 and e_s <= 1e-9, (worst, e_ld, e_s)


# --- 5: solves ---------------------------------------------------------------------------------
def check_solves(op, rank):
    """Iterative.solve(K, [y, two +-1 rows], tol=1e-8) with the preconditioner under both rules of
    grid2d_suite._solve_rules; returns the iteration counts."""
    from runlmc_amd.approx.iterative import Iterative
    if isinstance(op, str):
        op = operator(op)
    mode4(op, rank)
    assert op.K.preconditioner is not None and not op.K.preconditioner.exact
    rs = np.random.RandomState(8).randint(0, 2, (2, op.n)) * 2 - 1
    Kd = op.Kd
    p = types.SimpleNamespace(B=np.vstack([op.y, rs.astype(float)]), Kd=Kd,
                              oracle=types.SimpleNamespace(matvec=lambda v: Kd @ v),
                              lam_min=float(np.linalg.eigvalsh(Kd)[0]))
    X, it, resid = Iterative.solve(op.K, p.B, verbose=True, tol=1e-8)
    wr, wx = g2._solve_rules(p, np.atleast_2d(X), np.atleast_1d(resid))
    _say('solves (%s, rank %d)' % (op.name, rank), residual_rule=wr, error_rule=wx, iterations=max(it))
    assert np.all(np.asarray(resid) < 1e-8), resid
    return it


def check_iteration_gain(rank=64):
    """The low-noise variant of (a): first dense CG against dense PCG with the reference factor in
    NumPy (PCG at most a quarter of CG's iterations), then the device's PCG against its own
    precondition=False CG (at most half)."""
    from runlmc_amd.approx.iterative import Iterative
    op = operator('sep2d')
    old = op.noise.copy()
    try:
        op.set_noise(np.full(2, LOW_NOISE))
        Kd = op.Kd
        L, _ = np_pivchol(op.Kk, rank, 1e-10)
        P = L.T @ L + np.diag(op.eps)
        cf = la.cho_factor(P)
        it_cg = np_pcg(Kd, op.y.copy(), lambda r: r.copy(), 1e-8)
        it_pcg = np_pcg(Kd, op.y.copy(), lambda r: la.cho_solve(cf, r), 1e-8)
        _say('iteration gain, numpy (rank %d)' % rank, cg=it_cg, pcg=it_pcg)
        assert 4 * it_pcg <= it_cg, (it_pcg, it_cg)
        mode4(op, rank)
        B = op.y[None, :]
        X1, it1, r1 = Iterative.solve(op.K, B, verbose=True, tol=1e-8)
        X0, it0, r0 = Iterative.solve(op.K, B, verbose=True, tol=1e-8, minres=False, precondition=False)
        _say('iteration gain, device (rank %d)' % rank, cg=int(it0[0]), pcg=int(it1[0]), cg_resid=float(r0[0]),
             pcg_resid=float(r1[0]))
        assert r1[0] < 1e-8 and np.linalg.norm(op.y - Kd @ X1[0]) < 2e-8
        assert 2 * int(it1[0]) <= int(it0[0]), (it1, it0)
    finally:
        op.set_noise(old)
        op.ski.set_pivchol(0)


# --- 6: the model ------------------------------------------------------------------------------
@contextlib.contextmanager
def _default_rank(rank):
    """InterpolatedLLGP's default precond_rank for the duration: the other suites' model checks
    then run, unchanged, on models with the preconditioner."""
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    import inspect
    fn = InterpolatedLLGP.__init__
    names = list(inspect.signature(fn).parameters)
    pos = names.index('precond_rank') - (len(names) - len(fn.__defaults__))
    old = fn.__defaults__
    fn.__defaults__ = old[:pos] + (rank,) + old[pos + 1:]
    try:
        yield
    finally:
        fn.__defaults__ = old


def check_model(which, rank=32):
    c, make, suite = ((sep._model_case(), _sep_model, sep) if which == 'sep2d'
                      else (g3._case('mix'), _g3_model, g3))
    plain = make()
    plain._ensure()
    assert plain._K.preconditioner is None
    # alpha at tolerance 1e-12 against the dense solve (check_model_solve's rule)
    xref = la.solve(c.Kd, c.y, assume_a='pos')
    with loo_suite._tight_krylov():
        model = make(precond_rank=rank, tolerance=1e-12)
        model._ensure()
        M = model._K.preconditioner
        assert M is not None and not M.exact and model._K.device_operator().factor_mode == 4
        alpha = model.kernel.alpha()
    r = np.linalg.norm(c.y - c.Kd @ alpha)
    e = np.abs(alpha - xref).max()
    _say('model alpha (%s)' % which, residual=r, error=e)
    assert r < 1e-8 * np.linalg.norm(c.y), r
    assert e <= r / c.noise.min() + 1e-12 * np.abs(xref).max()
    # log det: the estimator's own bar (parity_suite: 4 sem + 1e-9 |ld|) against dense slogdet
    ld_ref = np.linalg.slogdet(c.Kd)[1]
    est, sem, it = M.logdet_estimate(n_probes=16, tol=1e-8)
    _say('model log det (%s)' % which, estimate=est, dense=ld_ref, sem=sem, iterations=int(np.max(it)))
    assert abs(est - ld_ref) <= 4.0 * sem + 1e-9 * abs(ld_ref), (est, ld_ref, sem)
    model = make(precond_rank=rank)
    np.random.seed(5)
    ll = model.log_likelihood()
    assert np.isfinite(ll) and np.all(np.isfinite(model.gradient))
    assert model._K.device_operator().factor_mode == 4
    # a parameter update keeps the option (the handle rebuilds the factor)
    x = model.param_array.copy()
    np.random.seed(5)
    model.param_array = x + 0.05 * np.random.RandomState(3).randn(len(x))
    assert model._K.preconditioner is not None and model._K.device_operator().factor_mode == 4
    # the other suites' checks on models that carry the option
    with _default_rank(rank):
        assert suite._model().precond_rank == rank
        suite.check_model_gradients()
        if which == 'sep2d':
            suite.check_model_tiled_variances()
        else:
            suite.check_model_variances(precompute=False)
    # loo: 'solve' on a subset at check_model_loo's bars, 'direct' refuses and names the preconditioner
    with loo_suite._tight_krylov():
        model = make(precond_rank=rank, tolerance=1e-12)
        model._ensure()
        Kinv = la.inv(c.Kd)
        a2, d = Kinv @ c.y, np.diag(Kinv)
        mean_ref, var_ref = c.y - a2 / d, 1.0 / d
        mean_tol = 1e-8 * np.abs(c.y).max()
        var_tol = loo_suite.DIAG_REL * np.max(1.0 / c.noise) / d ** 2
        ends = np.cumsum(c.lens)[:-1]
        sel = np.concatenate([[0, c.n - 1], ends - 1, ends, [7, 23]])
        means, vars_ = model.loo_predict(indices=sel, method='solve', tol=1e-12)
    em, ev = np.abs(means - mean_ref[sel]).max(), (np.abs(vars_ - var_ref[sel]) / var_tol[sel]).max()
    _say('model loo (%s)' % which, mean=em, mean_tol=mean_tol, variance_over_tol=ev)
    assert em <= mean_tol and ev <= 1.0, (em, mean_tol, ev)
    _raises(NotImplementedError, lambda: model.loo_predict(indices=sel, method='direct'), 'pivoted-Cholesky')
    mu, var = make(precond_rank=rank, variance_batch=8).predict(c.Xt)
    assert all(np.all(np.isfinite(v)) for v in mu + var)


# --- 7: updates --------------------------------------------------------------------------------
def check_updates(rank=16):
    """A handle walked through three parameter updates and one noise update against a fresh one
    built at the last parameters: equal pivots and equal bits of L; two builds of one operator
    equal bits; rank 0 afterwards restores available = 0."""
    def state(model):
        ski = model._K.device_operator()
        assert ski.factor()[0] and ski.factor_mode == 4
        used, piv, val, resid = ski.pivchol_info()
        return used, piv.copy(), val.copy(), ski.pivchol_factor().cpu().numpy(), resid.cpu().numpy()

    walked = _sep_model(precond_rank=rank)
    walked._ensure()
    first = state(walked)
    again = _sep_model(precond_rank=rank)
    again._ensure()
    second = state(again)
    assert first[0] == second[0]
    for a, b in zip(first[1:], second[1:]):
        np.testing.assert_array_equal(a, b)
    x = walked.param_array.copy()
    rng = np.random.RandomState(8)
    for _ in range(3):
        x = x + 0.1 * rng.randn(len(x))
        np.random.seed(5)
        walked.param_array = x
        state(walked)
    src = walked._functional_kernel
    new_noise = np.array(src.noise) * 1.7
    src.noise = new_noise
    np.random.seed(5)
    walked.parameters_changed()
    fresh = _sep_model(precond_rank=rank)
    fk = fresh._functional_kernel
    fk.coreg_vecs, fk.coreg_diags, fk.noise = src.coreg_vecs, src.coreg_diags, src.noise
    for k, s in zip(fk.kernels, src.kernels):
        k.set_params(s.param_array)
    np.random.seed(5)
    fresh._ensure()
    sw, sf = state(walked), state(fresh)
    assert sw[0] == sf[0]
    for a, b in zip(sw[1:], sf[1:]):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(sw[3], first[3])
    V = np.random.RandomState(2).randn(3, walked._K.shape[0])
    ski_w, ski_f = walked._K.device_operator(), fresh._K.device_operator()
    t = torch.from_numpy(V).to(ski_w.device)
    np.testing.assert_array_equal(ski_w.precond_apply(t).cpu().numpy(), ski_f.precond_apply(t).cpu().numpy())
    ski_w.set_pivchol(0)
    assert not ski_w.factor()[0] and ski_w.factor_mode == 0 and ski_w.factor_reason
    assert walked._K.preconditioner is None


# --- 8: refusals -------------------------------------------------------------------------------
def check_refusals():
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    from runlmc_amd.approx.iterative import Iterative
    op = operator('sep2d')
    for bad in (-1, 257, 2.5, '3', None, True):
        _raises(ValueError, lambda: op.ski.set_pivchol(bad))
        c = sep._model_case()
        fk = FunctionalKernel(D=c.D, lmc_kernels=sep._kernels(), lmc_ranks=[1, 1])
        _raises(ValueError, lambda: InterpolatedLLGP(c.Xs, c.Ys, normalize=False, m=[20, 16],
                                                     functional_kernel=fk, precond_rank=bad), 'precond_rank')
    # without a rank: exactly as before, with the parent's reason
    op.ski.set_pivchol(0)
    assert not op.ski.factor()[0] and op.ski.factor_mode == 0
    reason0 = op.ski.factor_reason
    assert reason0 and 'pivoted' not in reason0, reason0
    _raises(NotImplementedError, lambda: op.ski.pivchol_info(), 'pivoted-Cholesky')
    # mode 4 refuses what needs the polynomial form, and says why
    mode4(op, 8)
    B = _dev(op, np.ones((1, op.n)))
    from runlmc_amd._native import solve_direct
    _raises(NotImplementedError, lambda: solve_direct(op.ski, B), 'pivoted-Cholesky')
    _raises(NotImplementedError, lambda: op.ski.project(B), 'pivoted-Cholesky')
    _raises(NotImplementedError, lambda: op.ski.inverse_diag(), 'pivoted-Cholesky')
    # zero noise: no preconditioner, with a reason
    old = op.noise.copy()
    try:
        op.set_noise(np.array([0.0, old[1]]))
        assert not op.ski.factor()[0] and op.ski.factor_mode == 0 and 'noise' in op.ski.factor_reason
        assert op.K.preconditioner is None
    finally:
        op.set_noise(old)
        op.ski.set_pivchol(0)
    # a handle wholly in the polynomial form keeps mode 1 with a rank set
    from runlmc_amd._native import GridOp, SkiOp
    from cases import Case
    cs = Case('lmc_smooth')
    g = GridOp(cs.D, cs.m, cs.Q)
    g.set_lmc(cs.tops, cs.coreg_vecs, cs.coreg_diags)
    s = SkiOp(g, cs.W, cs.WT)
    s.set_noise(cs.noise, cs.lens)
    before = s.factor()
    mode_before = s.factor_mode
    s.set_pivchol(16)
    after = s.factor()
    assert s.factor_mode == mode_before and after == before, (mode_before, s.factor_mode, before, after)
    return mode_before
