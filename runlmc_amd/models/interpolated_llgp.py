"""The caller of the hot path: an InterpolatedLLGP-compatible model without
paramz (mirror of reference runlmc/models/interpolated_llgp.py:24-443 and
multigp.py:18-200).

Same constructor arguments, ``parameters_changed()`` / ``optimize()`` /
``predict()`` / ``log_likelihood()`` / ``normal_quadratic()`` / ``log_det_K()``.
Every product, solve and gradient inside runs on the device
(runlmc_amd.lmc.*).  Differences, all stated:

* ``log_det_K()`` is the matrix-free stochastic-Lanczos estimate of
  log det K~ (the reference's is a dense Cholesky of the exact kernel and is
  never on its optimiser path, interpolated_llgp.py:262-276); the exact one is
  ``ExactLMCLikelihood.log_det_K()``, the dense likelihood ``K()`` returns.
* inputs of any dimension, each kernel acting on one or two of them (bicubic
  interpolation, BTTB kernels; kernels on different active-dimension sets get
  their own grids);
* prediction modes: 'on-the-fly' and 'precompute' (both batched solves on the
  device) and 'exact' (variances from the device Cholesky factor of the exact
  kernel, runlmc_amd.lmc.ExactLMCLikelihood; any input dimension, split kernels).
* ``metrics=True`` records ``grad_error`` against the exact likelihood's
  gradient, as the reference does; at sizes the dense path cannot hold (device
  memory, kernel limits) the entry is NaN and one warning is logged.
* parameters live in one flat array in the optimiser's space; positive
  parameters go through paramz's Logexp (softplus) transform as in the
  reference (functional_kernel.py:130,185; rbf.py:33).
* `max_procs` is accepted and ignored (no process pool).
* ``fixed_noise``: known per-observation noise variances v_i (stated error bars, sigma^2 / count of
  binned means, down-weighted points) on top of the learned per-output noise:
  K~ = sum_t W_t K_t W_t^T + diag(eps_d(i) + v_i).  They are data, never a parameter.  ``predict``
  and ``posterior_samples(noise=True)`` describe a NEW observation, whose error bar is not known:
  they keep adding the per-output noise eps_d only.
"""
import logging

import numpy as np
import scipy.spatial.distance as sdist
import torch

from ..approx.interpolation import autogrid, multi_interpolant
from ..approx.iterative import Iterative
from ..kern.stationary import Lags, kernel_values
from ..lmc.grid_kernel import gen_grid_kernel
from ..lmc.likelihood import ApproxLMCLikelihood, ExactLMCLikelihood
from ..lmc.metrics import Metrics
from ..lmc.stochastic_deriv import StochasticDerivService
from .optimization import AdaDelta

_LOG = logging.getLogger(__name__)
_LIM = 36.0       # paramz Logexp switches to the identity beyond this


def _softplus(x):
    x = np.asarray(x, dtype=float)
    return np.where(x > _LIM, x, np.log1p(np.exp(np.clip(x, -np.inf, _LIM))))


def _softplus_inv(f):
    f = np.asarray(f, dtype=float)
    return np.where(f > _LIM, f, np.log(np.expm1(np.clip(f, 1e-300, _LIM))))


def _softplus_grad(f):
    """d softplus / dx expressed through the value f (paramz Logexp.gradfactor)."""
    f = np.asarray(f, dtype=float)
    return np.where(f > _LIM, 1.0, -np.expm1(-f))


class InterpolatedLLGP:
    EVAL_NORM = np.inf

    def __init__(self, Xs, Ys, normalize=True, lo=None, hi=None, m=None,
                 name='lmc', metrics=False, prediction='on-the-fly',
                 max_procs=None, trace_iterations=15, tolerance=1e-4,
                 functional_kernel=None, group=None, device_index=0, device_probes=None,
                 variance_batch=None, precond_rank=0, fixed_noise=None):
        self.name = name
        self.input_dim, self.output_dim = self._validate_io(Xs, Ys)
        self.normalizer = None
        Ys = [np.asarray(Y, dtype=float) for Y in Ys]
        # fixed_noise: one array per output, as long as that output's Y, in the units of Y^2
        fixed = self._validate_fixed_noise(fixed_noise, Ys)
        if normalize:
            self.normalizer = [(Y.mean(), Y.std()) for Y in Ys]
            if any(s == 0 for _, s in self.normalizer):
                raise ValueError('an output has no variance')
            Ys = [(Y - mu) / sd for Y, (mu, sd) in zip(Ys, self.normalizer)]
            if fixed is not None:
                fixed = [v / sd ** 2 for v, (_, sd) in zip(fixed, self.normalizer)]
        self.Ys = Ys
        # (the rows' order, the units of the normalised Ys; None: every path as without it)
        self.fixed_noise = None if fixed is None else np.concatenate(fixed)
        self.Xs = [np.asarray(X, dtype=float).reshape(len(X), -1) for X in Xs]
        if not functional_kernel:
            raise ValueError('functional_kernel must be provided')
        if prediction not in ('on-the-fly', 'precompute', 'exact'):
            raise ValueError('Variance prediction method {} unrecognized'
                             .format(prediction))
        self.prediction = prediction
        # variance_batch: None keeps the host-assembled right-hand sides of the reference
        # (interpolated_llgp.py:358-397); an integer >= 1 tiles 'on-the-fly' and 'precompute'
        # on the device with that many rows per solve (approx/quadforms.py); 'exact' ignores it
        if variance_batch is not None:
            if (isinstance(variance_batch, bool) or not isinstance(variance_batch, (int, np.integer))
                    or variance_batch < 1):
                raise ValueError('variance_batch must be None or an integer >= 1, got {!r}'
                                 .format(variance_batch))
            variance_batch = int(variance_batch)
        self.variance_batch = variance_batch
        # precond_rank: 0 (the default) changes nothing; 1 .. 256 opts in to the pivoted-Cholesky
        # preconditioner of that rank for operators without a polynomial factorisation (2-D and 3-D
        # grids, several active-dimension sets, more than 16 outputs: SkiOp.set_pivchol) -- the
        # operator then has a ``preconditioner`` and its solves run preconditioned CG
        if (isinstance(precond_rank, bool) or not isinstance(precond_rank, (int, np.integer))
                or not 0 <= precond_rank <= 256):
            raise ValueError('precond_rank must be an integer in 0 .. 256, got {!r}'
                             .format(precond_rank))
        self.precond_rank = int(precond_rank)
        # (the residual rule of the tiled solves: Iterative.solve's default, which the host
        # path's solves run with)
        self.variance_tolerance = 1e-4
        # what the last tiled variance computation returned per row (approx.quadforms.QuadForms)
        self.variance_stats = None
        # what the last leave-one-out call used: method, sem, solver statistics, count of rows
        # with a non-positive diagonal entry (loo_predict)
        self.loo_stats = None
        self._functional_kernel = functional_kernel
        self._functional_kernel.set_input_dim(self.input_dim)
        if any(len(ad) > 3 for ad in functional_kernel.active_dims):
            raise NotImplementedError(
                'kernels may act on at most three input dimensions each')
        if any(len(ad) == 3 for ad in functional_kernel.active_dims) and m is None:
            # (the default grid has as many points PER AXIS as an output has data: n^3 points)
            raise NotImplementedError(
                'a kernel over three input dimensions needs the grid sizes: the default grid '
                'would hold n points per axis, n^3 in all -- pass m=[m0, m1, m2] (shortest '
                'axis first, at most 60 there), or use ExactLMCLikelihood for small data')
        self.y = np.hstack(self.Ys)
        self.kernel = None
        self.dists, self.interpolants, self.grid_axes = {}, {}, {}
        # lags[ad]: dists[ad] together with the per-axis mesh it is the norm of (kern.Lags): what
        # the layers below are handed, so that a Separable kernel finds its axes
        self.lags = {}
        self._generate_grids(lo, hi, m)
        self.metrics = Metrics() if metrics else None
        self._device_index = device_index
        # (device_probes: a seed -- the Hutchinson probes are drawn on the device instead of by
        # NumPy's global RNG, StochasticDerivService; None keeps the reference's stream)
        self._deriv_service = StochasticDerivService(
            self.metrics, None, trace_iterations, tolerance, group=group,
            device_probes=device_probes)
        self._K = None
        self._grid_kernels = None
        self._caches = {}
        self._exact_declined = False
        _LOG.info('InterpolatedLLGP %s fully initialized', self.name)

    # -- data handling (multigp.py:75-118) ----------------------------------------
    @staticmethod
    def _validate_io(Xs, Ys):
        if len(Xs) != len(Ys):
            raise ValueError('Xs and Ys must have one entry per output')
        if not Xs:
            raise ValueError('need at least one output')
        dims = set()
        for X, Y in zip(Xs, Ys):
            X = np.asarray(X)
            if len(X) != len(Y):
                raise ValueError('an X and its Y differ in length')
            dims.add(1 if X.ndim == 1 else X.shape[1])
        if len(dims) != 1:
            raise ValueError('inputs differ in dimension')
        return dims.pop(), len(Ys)

    @staticmethod
    def _validate_fixed_noise(fixed_noise, Ys):
        if fixed_noise is None:
            return None
        if len(fixed_noise) != len(Ys):
            raise ValueError('fixed_noise must have one array per output (%d), got %d'
                             % (len(Ys), len(fixed_noise)))
        out = []
        for d, (v, Y) in enumerate(zip(fixed_noise, Ys)):
            v = np.asarray(v, dtype=float).reshape(-1)
            if len(v) != len(Y):
                raise ValueError('fixed_noise[%d] has %d values, output %d has %d observations'
                                 % (d, len(v), d, len(Y)))
            if not np.all(np.isfinite(v)):
                raise ValueError('fixed_noise[%d] holds values that are not finite' % d)
            if np.any(v < 0):
                raise ValueError('fixed_noise[%d] holds negative variances' % d)
            out.append(v)
        return out

    @staticmethod
    def _wrap(v, active_dims):
        """Entries of lo / hi / m that belong to one active-dimension set
        (interpolated_llgp.py:406-413): a scalar only for a single active
        dimension, otherwise indexed by the set."""
        if v is None:
            return None
        a = np.asarray(v, dtype=float)
        if not a.shape:
            if len(active_dims) != 1:
                raise ValueError('scalar lo / hi / m needs a single active dimension, got %d'
                                 % len(active_dims))
            return a.reshape(1)
        return a[list(active_dims)]

    def _generate_grids(self, lo, hi, m):
        for ad in self._functional_kernel.active_dims:
            Xs = [X[:, list(ad)] for X in self.Xs]
            wlo, whi, wm = (self._wrap(v, ad) for v in (lo, hi, m))
            self.grid_axes[ad] = autogrid(Xs, wlo, whi, wm)
            axes = self.grid_axes[ad]
            # distance of every grid point to grid point 0, shaped like the
            # grid (interpolated_llgp.py:425-432)
            mesh = np.meshgrid(*[a - a[0] for a in axes], indexing='ij')
            self.dists[ad] = np.sqrt(sum(np.square(g) for g in mesh))
            self.lags[ad] = Lags(mesh, self.dists[ad])
            W = multi_interpolant(Xs, *self.grid_axes[ad])
            WT = W.transpose().tocsr()
            WT.sort_indices()
            WT.indices = WT.indices.astype(np.int32)
            WT.indptr = WT.indptr.astype(np.int32)
            self.interpolants[ad] = (W, WT)

    # -- flat parameter vector in the optimiser's space ------------------------------
    def _param_blocks(self):
        """(array view, is_positive, gradient getter) for every free block, in
        a fixed order: coregionalisation vectors of LMC and SLFM kernels,
        kappa of LMC kernels, kernel parameters, noise."""
        fk = self._functional_kernel
        n_lmc, n_slfm = fk._num_lmc, fk._num_slfm
        blocks = []
        for q in range(n_lmc + n_slfm):
            blocks.append(('a%d' % q, fk.coreg_vecs[q], False,
                           lambda q=q: fk.coreg_vec_grads[q]))
        for q in range(n_lmc):
            blocks.append(('kappa%d' % q, fk.coreg_diags[q], True,
                           lambda q=q: fk.coreg_diag_grads[q]))
        for q, k in enumerate(fk.kernels):
            blocks.append(('kern%d' % q, k, True, lambda k=k: k.gradient))
        blocks.append(('noise', fk.noise, True, lambda: fk.noise_grad))
        return blocks

    @property
    def param_array(self):
        out = []
        for _, holder, positive, _ in self._param_blocks():
            vals = holder.param_array if hasattr(holder, 'set_params') else np.ravel(holder)
            out.append(_softplus_inv(vals) if positive else np.array(vals, dtype=float))
        return np.concatenate(out)

    @param_array.setter
    def param_array(self, x):
        x = np.asarray(x, dtype=float)
        pos = 0
        for _, holder, positive, _ in self._param_blocks():
            size = (len(holder.param_array) if hasattr(holder, 'set_params')
                    else holder.size)
            vals = x[pos:pos + size]
            pos += size
            vals = _softplus(vals) if positive else vals
            if hasattr(holder, 'set_params'):
                holder.set_params(vals)
            else:
                holder[...] = vals.reshape(holder.shape)
        assert pos == len(x)
        self.parameters_changed()

    @property
    def gradient(self):
        """d log-likelihood / d param_array (optimiser space)."""
        out = []
        for _, holder, positive, getter in self._param_blocks():
            g = np.ravel(np.asarray(getter(), dtype=float))
            if positive:
                vals = holder.param_array if hasattr(holder, 'set_params') else np.ravel(holder)
                g = g * _softplus_grad(vals)
            out.append(g)
        return np.concatenate(out)

    # -- the step (interpolated_llgp.py:192-245) -------------------------------------
    def parameters_changed(self):
        self._caches.clear()
        fk = self._functional_kernel
        lens = [len(Y) for Y in self.Ys]
        if self._K is None:
            self._K, self._grid_kernels = gen_grid_kernel(
                fk, self.lags, self.interpolants, lens,
                device_index=self._device_index, precond_rank=self.precond_rank,
                fixed_noise=self.fixed_noise)
        else:
            # same grid and interpolants: only spectra, factors and noise change
            for ad, gk in self._grid_kernels.items():
                gk.update(fk, self.lags[ad])
            self._K.update_noise(fk.noise, lens)
        self.kernel = ApproxLMCLikelihood(
            fk, self._K, self.lags, self.interpolants, self.Ys,
            self._deriv_service)
        self.kernel._grid_kernels = self._grid_kernels
        fk.update_gradient(self.kernel)
        if self.metrics is not None:
            g = self.gradient
            self.metrics.grad_norms.append(float(np.abs(g).max()))
            self.metrics.grad_error.append(self._grad_error())
            self.metrics.log_likely.append(self.log_likelihood())

    @staticmethod
    def _grad_vector(lik):
        """The four gradient families concatenated in the reference's order
        (interpolated_llgp.py:230-238)."""
        return np.concatenate((
            np.concatenate(lik.coreg_vec_gradients()).reshape(-1),
            np.concatenate(lik.coreg_diags_gradients()),
            np.concatenate(lik.kernel_gradients()),
            lik.noise_gradient()))

    def _grad_error(self):
        """|g_approx - g_exact| / |g_exact| in EVAL_NORM (interpolated_llgp.py:228-245); NaN
        when the exact likelihood cannot be formed at this size."""
        try:
            exact = self._dense()
        except (MemoryError, NotImplementedError, np.linalg.LinAlgError) as e:
            if not self._exact_declined:
                _LOG.warning('metrics: no exact gradient for grad_error (%s); recording NaN', e)
                self._exact_declined = True
            return float('nan')
        ga, ge = self._grad_vector(self.kernel), self._grad_vector(exact)
        return float(np.linalg.norm(ga - ge, self.EVAL_NORM) /
                     np.linalg.norm(ge, self.EVAL_NORM))

    def _dense(self):
        """The exact likelihood for the current parameters, built once per
        parameters_changed (reference interpolated_llgp.py:247-250)."""
        if 'dense' not in self._caches:
            self._caches['dense'] = ExactLMCLikelihood(
                self._functional_kernel, self.Xs, self.Ys, device_index=self._device_index,
                fixed_noise=self.fixed_noise)
        return self._caches['dense']

    def K(self):
        """The dense exact kernel matrix (reference interpolated_llgp.py:252-260).

        .. warning:: quadratic in memory and time."""
        self._ensure()
        return self._dense().K

    def optimize(self, optimizer=None, **kwargs):
        """Maximise the likelihood with AdaDelta (reference multigp.py:176-197
        through paramz)."""
        if self.metrics is not None:
            self.metrics = Metrics()
            self._deriv_service.metrics = self.metrics
        opt = optimizer or AdaDelta(**kwargs)
        x = self.param_array.copy()

        def neg_grad(xx):
            self.param_array = xx
            return -self.gradient

        try:
            opt.opt(x, neg_grad)
        except KeyboardInterrupt:
            _LOG.warning('optimization interrupted; keeping current parameters')
            raise
        self.param_array = x
        return opt

    # -- likelihood terms -----------------------------------------------------------
    def _ensure(self):
        if self.kernel is None:
            self.parameters_changed()

    def normal_quadratic(self):
        self._ensure()
        return self.kernel.normal_quadratic()

    def log_det_K(self):
        self._ensure()
        return self.kernel.log_det_K()

    def log_likelihood(self):
        self._ensure()
        return self.kernel.log_likelihood()

    # -- prediction (interpolated_llgp.py:293-397) --------------------------------------
    def _grid_alpha(self):
        if 'grid_alpha' not in self._caches:
            out = {}
            for ad, gk in self._grid_kernels.items():
                _, WT = self.interpolants[ad]
                out[ad] = gk.grid_K.matvec(WT.dot(self.kernel.alpha()))
            self._caches['grid_alpha'] = out
        return self._caches['grid_alpha']

    def _native_variance(self):
        fk = self._functional_kernel
        coregs = np.column_stack([np.square(a).sum(axis=0) for a in fk.coreg_vecs])
        coregs = coregs + np.column_stack(fk.coreg_diags)
        zero = {ad: Lags.zero(len(ad)) for ad in fk.active_dims}
        k0 = np.array(fk.eval_kernels(zero), dtype=float)
        return coregs.dot(k0).reshape(-1) + fk.noise

    def _exact_cross_kernel(self, Xs):
        """Exact (non-SKI) covariance between test and training points
        (reference likelihood.py:176-199)."""
        fk = self._functional_kernel
        rl, cl = [len(X) for X in Xs], [len(X) for X in self.Xs]
        A = np.vstack([X.reshape(len(X), self.input_dim) for X in Xs])
        B = np.vstack(self.Xs)
        dist = {ad: sdist.cdist(A[:, list(ad)], B[:, list(ad)])
                for ad in fk.active_dims}
        for k in fk.kernels:
            ad = k.active_dims
            if k.separable and not isinstance(dist[ad], Lags):
                dist[ad] = Lags.between(A[:, list(ad)], B[:, list(ad)], dist[ad])
        ro, co = np.repeat(np.arange(fk.D), rl), np.repeat(np.arange(fk.D), cl)
        K = np.zeros((sum(rl), sum(cl)))
        for Bq, k in zip(fk.coreg_mats(), fk.kernels):
            K += Bq[np.ix_(ro, co)] * kernel_values(k, dist[k.active_dims])
        return K

    def _light_exact(self):
        """The exact kernel's device handle holding the training points and the current
        parameters: set, never assembled or factored (no n x n buffer).  Kernels without a
        device formula raise exact_descriptors' NotImplementedError."""
        if 'light_exact' not in self._caches:
            from .._native import ExactOp
            fk = self._functional_kernel
            X = np.vstack(self.Xs)
            op = ExactOp(X.shape[0], X.shape[1], device_index=self._device_index)
            if self.fixed_noise is not None:
                op.set_row_noise(self.fixed_noise)
            op.set(X, [len(x) for x in self.Xs], fk.kernels, fk.coreg_mats(), fk.noise)
            self._caches['light_exact'] = op
        return self._caches['light_exact']

    def _var_on_the_fly_tiled(self, Xs):
        from ..approx.quadforms import CrossRows, quad_forms
        lens = [len(X) for X in Xs]
        if sum(lens) == 0:
            return np.zeros(0)
        rows = CrossRows(self._light_exact(), np.vstack(Xs), lens)
        self.variance_stats = quad_forms(self._K, rows, rows.total_rows, self.variance_batch,
                                         self.variance_tolerance)
        return self.variance_stats.v

    def _var_on_the_fly(self, _W, Xs):
        if self.variance_batch is not None:
            return self._var_on_the_fly_tiled(Xs)
        Kx = self._exact_cross_kernel(Xs)
        if Kx.shape[0] == 0:
            return np.zeros(0)
        sol = Iterative.solve(self._K, Kx)           # one batched device solve
        return np.einsum('ij,ij->i', Kx, np.atleast_2d(sol))

    def _var_exact(self, _W, Xs):
        """diag(K_*X K^-1 K_X*) with the exact K's Cholesky factor (reference
        interpolated_llgp.py:350-356)."""
        return self._dense().explained_variance(Xs)

    def _precomputed_nu(self):
        if 'nu' not in self._caches:
            if len(self.interpolants) != 1:
                raise ValueError(
                    'precompute prediction mode unavailable for split kernels')
            (ad,) = self.interpolants
            W, WT = self.interpolants[ad]
            gk = self._grid_kernels[ad]
            if self.variance_batch is not None:
                from ..approx.quadforms import GridColumnRows, quad_forms
                rows = GridColumnRows(gk)
                self.variance_stats = quad_forms(self._K, rows, rows.total_rows,
                                                 self.variance_batch, self.variance_tolerance)
                self._caches['nu'] = self.variance_stats.v
                return self._caches['nu']
            Dm = W.shape[1]
            # K_XU e_i for every grid index: columns of W K_UU
            KXU = W.dot(gk.grid_K.matmat(np.identity(Dm)))          # (n, Dm)
            sol = Iterative.solve(self._K, np.ascontiguousarray(KXU.T))   # (Dm, n)
            back = gk.grid_K.matmat(WT.dot(np.atleast_2d(sol).T))    # K_UX K^-1 K_XU
            self._caches['nu'] = np.diag(back).copy()
        return self._caches['nu']

    def _var_precompute(self, Ws, _Xs):
        nu = self._precomputed_nu()
        (W,) = Ws.values()
        return W.dot(nu)

    def _raw_predict(self, Xs):
        self._ensure()
        Xs = [np.asarray(X, dtype=float).reshape(len(X), self.input_dim) for X in Xs]
        lens = [len(X) for X in Xs]
        mean = np.zeros(sum(lens))
        Ws = {}
        for ad, grid_alpha in self._grid_alpha().items():
            Ws[ad] = multi_interpolant([X[:, list(ad)] for X in Xs], *self.grid_axes[ad])
            mean += Ws[ad].dot(grid_alpha)
        native = np.repeat(self._native_variance(), lens)
        explained = {'on-the-fly': self._var_on_the_fly, 'precompute': self._var_precompute,
                     'exact': self._var_exact}[self.prediction](Ws, Xs)
        var = native - explained
        var[var < 0] = 0
        cuts = np.cumsum(lens)[:-1]
        return np.split(mean, cuts), np.split(var, cuts)

    def predict(self, Xs):
        """(means, variances), one array per output, de-normalised
        (multigp.py:108-150)."""
        if len(Xs) != self.output_dim:
            raise ValueError('need one (possibly empty) input array per output')
        mu, var = self._raw_predict(Xs)
        if self.normalizer:
            mu = [m * sd + mean for m, (mean, sd) in zip(mu, self.normalizer)]
            var = [v * sd ** 2 for v, (_, sd) in zip(var, self.normalizer)]
        return mu, var

    # -- function draws (no reference twin; approx/pathwise.py) -------------------------------
    def _pathwise_samplers(self, max_embed):
        """One GridSampler per term of the operator, in its term order, for the current
        parameters (rebuilt after parameters_changed)."""
        from ..approx.pathwise import GridSampler
        key = ('samplers', int(max_embed))
        if key not in self._caches:
            fk = self._functional_kernel
            out = []
            for ad, gk in self._grid_kernels.items():
                kidx = fk.active_dims[ad]
                out.append(GridSampler(gk, [fk.kernels[q] for q in kidx],
                                       [fk.coreg_vecs[q] for q in kidx],
                                       [fk.coreg_diags[q] for q in kidx],
                                       self.grid_axes[ad], max_embed=max_embed))
            self._caches[key] = out
        return self._caches[key]

    def _draw_tiles(self, size, seed, batch, max_embed, tolerance, posterior):
        from ..approx import pathwise as pw
        self._ensure()
        if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size < 1:
            raise ValueError('size must be an integer >= 1, got {!r}'.format(size))
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise ValueError('batch must be an integer >= 1, got {!r}'.format(batch))
        size = int(size)
        tile = int(batch) + int(batch) % 2         # pairs of draws share a transform
        samplers = self._pathwise_samplers(max_embed)
        ads = list(self._grid_kernels)
        K = self._K
        lib, dev = K.device_operator().lib, K.device
        tol = self._deriv_service._tol if tolerance is None else float(tolerance)
        y = torch.from_numpy(np.ascontiguousarray(self.y, dtype=np.float64)).to(dev) if posterior else None
        host = {ad: np.empty((size, s.grid.width)) for ad, s in zip(ads, samplers)}
        info = []
        for s0 in range(0, size, tile):
            k = min(tile, size - s0)
            Zs = [s.noise(pw.stream_seed(seed, pw.STREAM_TERM0 + t), s0, k)
                  for t, s in enumerate(samplers)]
            if posterior:
                E = pw.normal_fill(lib, pw.stream_seed(seed, pw.STREAM_E), s0, k, len(self.y), dev)
                res = pw.posterior_grid_draws(K, samplers, y, Zs, E, tol=tol)
                U = res.draws
                info.append(res._replace(draws=None))
            else:
                U = pw.prior_grid_draws(samplers, Zs, k)
            for ad, u in zip(ads, U):
                host[ad][s0:s0 + k] = u.cpu().numpy()
        return pw.PathwiseDraws(self, host, seed, info)

    def prior_draws(self, size, seed=0, batch=16, max_embed=16):
        """`size` functions from the SKI model's PRIOR f = sum_t W_t u_t, u_t ~ N(0, K_t), as a
        PathwiseDraws: call it with test inputs.  See posterior_draws for the arguments."""
        return self._draw_tiles(size, seed, batch, max_embed, None, posterior=False)

    def posterior_draws(self, size, seed=0, batch=16, tolerance=None, max_embed=16):
        """`size` functions from the SKI model's POSTERIOR given the training data, by Matheron's
        rule (approx/pathwise.py): prior draws on the grids, one batched solve of the operator
        per tile of `batch` draws (rounded up to an even number: two draws share one complex
        transform) and a back-projection.  Returns a PathwiseDraws: ``draws(Xs, noise=False)``
        gives one (size, len(Xs[d])) array per output, de-normalised, the SAME functions at
        whatever inputs it is asked for; ``.info`` holds solver, iterations, largest residual
        and exit codes per tile; a residual above the tolerance is logged, not raised.

        tolerance=None: the model's solve tolerance.  Draw s is a function of (seed, s) only:
        not of size, of batch, or of the rank that draws it (every rank given the same seed
        holds the same draws; nothing is communicated).  max_embed bounds the circulant
        embedding (approx.pathwise.GridSampler).

        The draws' mean is the mean ``predict`` returns (up to the solve tolerance).  Their
        covariance is the SKI model's, W*(K_UU - K_UU W^T K~^-1 W K_UU)W*^T, which differs
        slightly from ``predict``'s variances: those take the exact k(0) for the native term,
        and 'on-the-fly' the exact cross-kernel."""
        return self._draw_tiles(size, seed, batch, max_embed, tolerance, posterior=True)

    def posterior_samples(self, Xs, size=1, seed=0, noise=False, **kw):
        """posterior_draws(size, seed, **kw)(Xs, noise) in one call."""
        if len(Xs) != self.output_dim:
            raise ValueError('need one (possibly empty) input array per output')
        return self.posterior_draws(size, seed=seed, **kw)(Xs, noise=noise)

    # -- leave-one-out cross-validation (no reference twin; approx/loo.py) -----------------------
    def _loo(self, indices, method, kw):
        """(means, variances, log density sum) of the held-out observations, in the units of the
        original Ys: tensors over all rows, or over `indices`.  Fills loo_stats."""
        from ..approx.loo import inverse_diagonal
        from .._native import loo_reduce
        self._ensure()
        K = self._K
        dev, lib = K.device, K.device_operator().lib
        res = inverse_diagonal(K, method=method, indices=indices, **kw)
        lens = [len(Y) for Y in self.Ys]

        def rows(v):
            return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
        alpha = getattr(getattr(self.kernel, 'deriv', None), 'alpha_dev', None)
        if alpha is None:
            alpha = rows(self.kernel.alpha())
        y = rows(self.y)
        sd = np.repeat([s for _, s in self.normalizer], lens) if self.normalizer else None
        mu = np.repeat([m for m, _ in self.normalizer], lens) if self.normalizer else None
        sel = None
        if indices is not None:
            sel = np.asarray(indices, dtype=np.int64).reshape(-1)
            if sel.size == 0:
                self.loo_stats = dict(method=res.method, sem=res.sem, stats=res.stats, nonpositive=0)
                return np.zeros(0), np.zeros(0), 0.0
            at = torch.from_numpy(sel).to(dev)
            alpha, y = alpha[at].contiguous(), y[at].contiguous()
            if sd is not None:
                sd, mu = sd[sel], mu[sel]
        logscale = rows(np.log(sd)) if sd is not None else None
        mean, var, logp, bad = loo_reduce(lib, y, alpha.contiguous(), res.d.contiguous(), logscale)
        if bad:
            _LOG.critical('leave-one-out (%s): %d of %d rows have a diagonal entry of K~^-1 that is '
                          'not a positive finite number; their predictions are NaN and they are '
                          'left out of the log likelihood', res.method, bad, int(y.shape[0]))
        self.loo_stats = dict(method=res.method, sem=res.sem, stats=res.stats, nonpositive=bad)
        mean, var = mean.cpu().numpy(), var.cpu().numpy()
        if sd is not None:
            mean, var = mean * sd + mu, var * sd ** 2
        return mean, var, logp

    def loo_predict(self, indices=None, method='auto', **kw):
        """(means, variances) of every training OBSERVATION predicted from all the others
        (leave-one-out, Rasmussen & Williams 5.4.2): mean y_i - alpha_i / d_i and variance
        1 / d_i with d = diag(K~^-1), de-normalised as ``predict`` de-normalises.  One array per
        output; with `indices` (rows of the concatenated outputs) two arrays over those rows.

        The held-out quantity is the noisy observation, so the noise is part of the variance:
        ``variances[d] - noise_d * sd_d ** 2`` is the latent function's (sd_d = 1 without
        normalisation); with ``fixed_noise`` the held-out row's own variance is part of it too, and
        ``variances[d] - noise_d * sd_d ** 2 - fixed_noise[d]`` is the latent function's.

        method and **kw (probes, n_probes, seed, batch, tol, control_variate) go to
        ``approx.loo.inverse_diagonal``: 'direct' (no solve at all, operators whose factorisation
        is K~^-1), 'solve' (one solve per row asked for), 'probes' (an estimate; ``loo_stats['sem']``
        is the standard error of d), 'auto'.  alpha is the solve the model has already made.
        ``loo_stats`` holds the method that ran, sem, the solver's statistics and the count of
        rows with a non-positive d (logged at CRITICAL, NaN in the result, never clamped)."""
        mean, var, _ = self._loo(indices, method, kw)
        if indices is not None:
            return mean, var
        cuts = np.cumsum([len(Y) for Y in self.Ys])[:-1]
        return np.split(mean, cuts), np.split(var, cuts)

    def loo_log_likelihood(self, indices=None, method='auto', **kw):
        """The leave-one-out pseudo-likelihood: sum over the rows (or over `indices`) of the log
        density of y_i under its leave-one-out prediction, in the units of the original Ys (a
        normalising model subtracts log sd_d per row).  Arguments as loo_predict."""
        return float(self._loo(indices, method, kw)[2])

    def predict_quantiles(self, Xs, quantiles=(2.5, 97.5)):
        """Gaussian predictive quantiles (multigp.py:152-174)."""
        from scipy.stats import norm
        mu, var = self.predict(Xs)
        return [[m + norm.ppf(q / 100.0) * np.sqrt(v) for q in quantiles]
                for m, v in zip(mu, var)]
