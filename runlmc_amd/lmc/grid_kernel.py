"""The LMC covariance operator on the device (mirror of reference
runlmc/lmc/grid_kernel.py:22-136).

The reference builds K_UU in one of three algebraically identical
representations ('sum', 'bt', 'slfm') to trade FFT counts.  On the device a
single formulation serves every (D, Q, R): forward transforms of the D
outputs, a real D x D mix at each frequency from the factors A_q, kappa_q and
the Q real circulant spectra, D inverse transforms -- 2D transforms per
product regardless of Q and R.  ``ktype`` is accepted and recorded for
interface compatibility; it does not change the arithmetic performed.

The reference quirk of adding an identity on the grid for pure-SLFM or
pure-independent models under 'slfm' (grid_kernel.py:87-88,104-105) is NOT
reproduced by default: the operator here is the mathematical sum_q B_q (x) K_q.
``reference_slfm_identity=True`` reproduces it (an extra unit-impulse top row with
B = I per identity the reference adds), for callers that need the reference's
numbers bit for bit in those two degenerate model classes.
"""
import numpy as np
import torch

from ..linalg.matrix import Matrix, check_vector, check_block
from ..linalg.diag import Diag
from ..linalg.sum_matrix import SumMatrix
from .._native import GridOp, SkiOp, solve_direct, solve_pcg
from .._lib import as_f64
from ..kern.stationary import Lags


def _distances(grid_dists):
    return grid_dists if isinstance(grid_dists, Lags) else np.asarray(grid_dists)


def choose_ktype(fk, active_dim):
    """What the reference would pick (grid_kernel.py:52-64); informational."""
    if fk.Q == 1:
        return 'sum'
    no_diag = (not fk.num_lmc[active_dim]) and (not fk.num_indep[active_dim])
    bonus = fk.D if no_diag else 0
    return 'slfm' if fk.total_rank(active_dim) + fk.D < fk.D ** 2 + bonus else 'bt'


def slfm_identity_terms(fk, active_dim):
    """Identity matrices the reference's 'slfm' representation adds on the grid
    (grid_kernel.py:87-88: no coregionalised kernel in the set; :104-105:
    neither LMC nor independent kernels)."""
    kidx = fk.active_dims[active_dim]
    count = 0
    if not fk.filter_non_indep_idxs(kidx):
        count += 1
    if fk.num_lmc[active_dim] == 0 and fk.num_indep[active_dim] == 0:
        count += 1
    return count


class _GridKUU(Matrix):
    """K_UU on grid vectors (what the reference exposes as GridKernel.grid_K;
    prediction reaches into it, models/interpolated_llgp.py:298,373)."""

    def __init__(self, gridop):
        super().__init__(gridop.width, gridop.width)
        self.op = gridop

    def matvec(self, x):
        x = check_vector(x, self.shape[1])
        return self.op.matmat_host(x.astype(np.float64))

    def matmat(self, X):
        X = check_block(X, self.shape[1])
        return self.op.matmat_host(np.ascontiguousarray(X.T, dtype=np.float64)).T

    def matmat_device(self, X):
        return self.op.mvm(X)


class _DeviceSKI(Matrix):
    """W K_UU W^T without noise, device resident (reference SKI object,
    approx/ski.py:8-16)."""

    def __init__(self, ski, W, WT, grid_K):
        super().__init__(ski.n, ski.n)
        self._ski = ski
        self.W, self.WT, self.K = W, WT, grid_K

    def matmat_device(self, X):
        return self._ski.apply_w(self._ski.grid.mvm(self._ski.apply_wt(X)))

    def _host(self, rows):
        t = torch.from_numpy(rows).to(self._ski.device)
        return self.matmat_device(t).cpu().numpy()

    def matvec(self, x):
        x = check_vector(x, self.shape[1])
        return self._host(np.ascontiguousarray(x, dtype=np.float64)[None, :])[0]

    def matmat(self, X):
        X = check_block(X, self.shape[1])
        return self._host(np.ascontiguousarray(X.T, dtype=np.float64)).T

    def as_numpy(self):
        half = self.W.dot(self.K.as_numpy().T)
        return self.W.dot(half.T)


class GridKernel(Matrix):
    """W K_UU W^T for the kernels that share one active-dimension set."""

    def __init__(self, functional_kernel, grid_dists, interpolant,
                 interpolantT, ktype, active_dim, device_index=0,
                 reference_slfm_identity=False):
        n = interpolant.shape[0]
        super().__init__(n, n)
        if ktype not in ('sum', 'bt', 'slfm'):
            raise AssertionError(ktype)
        self.ktype = ktype
        self.active_dim = active_dim
        fk = functional_kernel
        # (a kern.Lags -- the distances with the grid's per-axis lags -- passes as it is)
        grid_dists = _distances(grid_dists)
        if grid_dists.ndim > 3:
            raise NotImplementedError(
                'device GridKernel supports 1-D, 2-D and 3-D grids')
        kidx = fk.active_dims[active_dim]
        tops = as_f64(fk.eval_kernels_fixed_dim(grid_dists, active_dim)
                      ).reshape(len(kidx), -1)
        self._m = tops.shape[1]
        # the reference's identity terms under 'slfm', on request: a unit impulse as
        # an extra top row (T = I) with B = count * I
        self._eye = (slfm_identity_terms(fk, active_dim)
                     if reference_slfm_identity and ktype == 'slfm' else 0)
        self._op = GridOp(fk.D, self._m, len(kidx) + (1 if self._eye else 0),
                          device_index=device_index, sizes=grid_dists.shape)
        self._set(fk, kidx, tops)
        self._skiop = SkiOp(self._op, interpolant, interpolantT)
        # parameter sets this object has taken since it was built (LMCOperator.state_version)
        self.version = 0
        self.grid_K = _GridKUU(self._op)
        self.ski = _DeviceSKI(self._skiop, interpolant, interpolantT, self.grid_K)

    def update(self, functional_kernel, grid_dists):
        """New hyper-parameters, same grid and interpolants: rebuild only the
        spectra and factors (rl_gridop_set_lmc), keep W on the device."""
        fk = functional_kernel
        kidx = fk.active_dims[self.active_dim]
        tops = as_f64(fk.eval_kernels_fixed_dim(_distances(grid_dists),
                                                self.active_dim)).reshape(len(kidx), -1)
        self._set(fk, kidx, tops)
        self.version += 1

    def _set(self, fk, kidx, tops):
        vecs = [fk.coreg_vecs[q] for q in kidx]
        diags = [fk.coreg_diags[q] for q in kidx]
        if self._eye:
            impulse = np.zeros((1, tops.shape[1]))
            impulse[0, 0] = 1.0
            tops = np.vstack([tops, impulse])
            vecs = vecs + [None]
            diags = diags + [float(self._eye) * np.ones(fk.D)]
        self._op.set_lmc(tops, vecs, diags)

    @property
    def device(self):
        return self._op.device

    def matvec(self, x):
        return self.ski.matvec(x)

    def matmat(self, X):
        return self.ski.matmat(X)

    def matmat_device(self, X):
        return self.ski.matmat_device(X)

    def as_numpy(self):
        return self.ski.as_numpy()


class FactoredInverse(Matrix):
    """K~^-1 through the Woodbury factorisation of K~ = F M F^T + diag(eps) that an
    operator wholly in the polynomial form admits (csrc/rl_direct.h): what
    ``LMCOperator.preconditioner`` hands to ``Iterative.solve`` -- the reference reads
    the same attribute (approx/iterative.py:47: ``M = getattr(K, 'preconditioner', None)``)
    and no reference operator sets it.  As a Matrix it applies K~^-1 (one pass, no
    refinement); ``solve`` refines to the reference's residual rule."""

    MAX_REFINE = 4

    def __init__(self, skiop, exact=True, version=None):
        super().__init__(skiop.n, skiop.n)
        self._skiop = skiop
        # exact: every top row is in the polynomial form and the factorisation IS K~^-1.  Not
        # exact (a Matern row next to smooth ones, Matern rows alone): it inverts the
        # operator's projection on the polynomial subspace -- the M of preconditioned conjugate
        # gradients (rl_solve_pcg), no log det
        self._exact = bool(exact)
        # version: () -> LMCOperator.state_version() of the operator this was taken from.  The
        # handle refactors itself after every parameter or noise update, so an object kept
        # across one always works on the CURRENT operator; which of the two kinds its
        # factorisation is may have changed with it, and is read again from the handle then
        self._version = version
        self._stamp = version() if version is not None else None

    @property
    def exact(self):
        """Whether the handle's factorisation is K~^-1 (else a preconditioner) for the operator's
        CURRENT parameters: the flag of construction until a parameter or noise update, read from
        the handle again after one.  RuntimeError when the current parameters have no
        factorisation at all."""
        if self._version is not None:
            now = self._version()
            if now != self._stamp:
                ok = self._skiop.factor()[0]
                if not ok:
                    raise RuntimeError(
                        'this FactoredInverse was taken before a parameter or noise update, and the '
                        'operator has no factorisation for its current parameters (%s): ask '
                        'K.preconditioner again' % self._skiop.factor_reason)
                self._exact = self._skiop.factor_mode == 1
                self._stamp = now
        return self._exact

    def solve(self, B, tol=1e-4, max_refine=None, maxiter=0):
        """B: (k, n) tensor on the device.  (X, applications of the factorisation, residuals,
        istop): refinement when it is K~^-1, preconditioned CG when it is a preconditioner."""
        if not self.exact:
            return solve_pcg(self._skiop, B, tol=tol, maxiter=maxiter)
        return solve_direct(self._skiop, B, tol=tol,
                            max_refine=self.MAX_REFINE if max_refine is None else max_refine)

    def logdet(self):
        """log det K~, exactly (determinant lemma) -- the reference's dense
        ``log_det_K`` (models/interpolated_llgp.py:262-276) without the Cholesky."""
        ok, ld, _ = self._skiop.factor()
        if not ok or self._skiop.factor_mode != 1:
            raise ValueError(self._skiop.factor_reason or
                             'the factorisation is a preconditioner here, not K~^-1: no exact log det')
        return ld

    LOGDET_PROBES = 16
    LOGDET_SEED = 20240607

    def logdet_estimate(self, n_probes=None, tol=1e-4, maxiter=0, seed=None, group=None):
        """log det K~ when the factorisation is a PRECONDITIONER (include/runlmc_hip.h,
        rl_ski_precond_sample):  log det P  exactly  +  Hutchinson / Lanczos-quadrature estimate of
        tr log(P^-1/2 K~ P^-1/2)  from a few extra conjugate-gradient solves whose right-hand sides
        are +-1 rows mapped to covariance P.  Returns (estimate, standard error of the mean,
        iterations of this rank's solves).  Every rank draws the same rows (fixed seed); with a
        process group each solves rows rank, rank + world, ... and ONE all-reduce of (sum, sum of
        squares) gives every rank the same estimate."""
        from .._native import solve_pcg_lanczos, slq_quadratic_forms
        if self.exact:
            return self.logdet(), 0.0, np.zeros(0, dtype=np.int32)
        N = int(n_probes or self.LOGDET_PROBES)
        gen = torch.Generator().manual_seed(self.LOGDET_SEED if seed is None else int(seed))
        W = (torch.randint(0, 2, (N, self._skiop.n), generator=gen, dtype=torch.int8) * 2 - 1)
        from ..util.dist import rank_world, all_reduce_sum_
        rank, world = rank_world(group)
        W = W[rank::world].contiguous().to(self._skiop.device).to(torch.float64)
        R, ld_p = self._skiop.precond_sample(W)
        cap = int(min(max(maxiter or 1024, 1), 4096))
        X, it, res, st, lz, sq = solve_pcg_lanczos(self._skiop, R, tol=tol, maxiter=maxiter, cap=cap)
        quad = slq_quadratic_forms(lz, it, sq, lib=self._skiop.lib)
        sums = torch.tensor([float(np.sum(quad)), float(np.sum(quad * quad))], dtype=torch.float64)
        all_reduce_sum_(sums, group)                      # (no-op in a world of one)
        mean = float(sums[0]) / N
        var = max(float(sums[1]) / N - mean * mean, 0.0) * N / (N - 1) if N > 1 else float('nan')
        sem = float(np.sqrt(var / N)) if N > 1 else float('nan')
        return ld_p + mean, sem, it

    def matmat_device(self, X):
        if not self.exact:
            if self._skiop.factor_mode == 4:
                # (the pivoted-Cholesky preconditioner: one application, rl_ski_precond_apply)
                return self._skiop.precond_apply(X.contiguous())
            raise NotImplementedError('this preconditioner is applied inside rl_solve_pcg only')
        return solve_direct(self._skiop, X.contiguous(), tol=np.finfo(np.float64).max,
                            max_refine=0)[0]

    def matvec(self, x):
        x = check_vector(x, self.shape[1])
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)[None, :])
        return self.matmat_device(t.to(self._skiop.device)).cpu().numpy()[0]

    def matmat(self, X):
        X = check_block(X, self.shape[1])
        t = torch.from_numpy(np.ascontiguousarray(X.T, dtype=np.float64))
        return self.matmat_device(t.to(self._skiop.device)).cpu().numpy().T


class LMCOperator(SumMatrix):
    """K~ = sum over active-dimension sets of GridKernel + Diag(noise): the
    SumMatrix gen_grid_kernel returns (reference grid_kernel.py:66-74), with
    ONE device handle (all terms and the noise) that serves the fused product
    and the batched solver.  ``extra``: known per-observation variances (n values >= 0, the
    rows' order) added to the noise diagonal, never a parameter (SkiOp.set_noise_rows)."""

    def __init__(self, grid_kernels, noise_diag_matrix, noise, lens, extra=None):
        grid_kernels = list(grid_kernels)
        super().__init__(grid_kernels + [noise_diag_matrix])
        self._gks = grid_kernels
        first = grid_kernels[0]
        self._skiop = first._skiop
        self.term_of = {first.active_dim: 0}
        for gk in grid_kernels[1:]:
            W, WT = gk.ski.W, gk.ski.WT
            self.term_of[gk.active_dim] = self._skiop.add_term(gk._op, W, WT)
        self.extra = None if extra is None else np.ascontiguousarray(as_f64(extra).reshape(-1))
        self._set_noise(noise, lens)
        self.lens = list(lens)
        self._noise_version = 0

    def _set_noise(self, noise, lens):
        if self.extra is None:
            self._skiop.set_noise(noise, lens)
            self.Ks[-1].v = np.repeat(noise, lens)
        else:
            self._skiop.set_noise_rows(noise, lens, self.extra)
            self.Ks[-1].v = np.repeat(noise, lens) + self.extra

    def state_version(self):
        """A value that changes with every GridKernel.update() of a term and every
        update_noise(): what an object derived from the operator's parameters keeps to find out
        later whether it still describes them (StochasticDeriv's deferred log det,
        FactoredInverse.exact)."""
        return tuple(gk.version for gk in self._gks), self._noise_version

    def device_operator(self):
        return self._skiop

    @property
    def preconditioner(self):
        """The attribute the reference's Iterative.solve looks for (approx/iterative.py:47).
        A FactoredInverse when every top row of the CURRENT parameters is in the
        polynomial form (the factorisation is rebuilt on the device handle whenever
        parameters or noise changed), else None -- the Krylov path as before."""
        ok = self._skiop.factor()[0]
        return (FactoredInverse(self._skiop, exact=self._skiop.factor_mode == 1,
                                version=self.state_version) if ok else None)

    @property
    def device(self):
        return self._skiop.device

    def _try_fuse(self):
        return None

    def matmat_device(self, X):
        return self._skiop.mvm(X)

    def matvec(self, x):
        x = check_vector(x, self.shape[1])
        return self._skiop.matmat_host(x.astype(np.float64))

    def matmat(self, X):
        X = check_block(X, self.shape[1])
        return self._skiop.matmat_host(
            np.ascontiguousarray(X.T, dtype=np.float64)).T

    def update_noise(self, noise, lens):
        self._set_noise(noise, lens)
        self._noise_version += 1


def gen_grid_kernel(fk, grid_dists, interpolants, lens_per_output,
                    device_index=0, reference_slfm_identity=False, precond_rank=0, fixed_noise=None):
    """(K~, {active_dim: GridKernel}) exactly as the reference returns them
    (grid_kernel.py:49-74): one GridKernel per active-dimension set, summed
    with the noise.  precond_rank > 0 opts in to the pivoted-Cholesky preconditioner of that
    rank for operators without a polynomial factorisation (SkiOp.set_pivchol).  fixed_noise: known
    per-observation variances (n values, the rows' order) on top of fk.noise (LMCOperator)."""
    grid_kerns = {}
    for active_dim in fk.active_dims:
        W, WT = interpolants[active_dim]
        grid_kerns[active_dim] = GridKernel(
            fk, grid_dists[active_dim], W, WT, choose_ktype(fk, active_dim),
            active_dim, device_index=device_index,
            reference_slfm_identity=reference_slfm_identity)
    noise = Diag(np.repeat(fk.noise, lens_per_output))
    K = LMCOperator(list(grid_kerns.values()), noise, fk.noise, lens_per_output, extra=fixed_noise)
    if precond_rank:
        K.device_operator().set_pivchol(precond_rank)
    return K, grid_kerns
