"""Function draws from the SKI model by Matheron's rule (pathwise sampling); the reference has
no sampler (its predictions are means and marginal variances, models/interpolated_llgp.py:293-397).

Model, per grid term t (one per active-dimension set):  u_t ~ N(0, K_t),  K_t = sum_q B_q (x) T_q;
f = sum_t W_t u_t;  y = f + sqrt(eps) * e.  One posterior draw on the grid from the noise (u_t, e):

    r    = y - sum_t W_t u_t - sqrt(eps) * e
    v    = K~^-1 r                      (the operator's own solver, batched over the draws)
    u_t* = u_t + K_t W_t^T v

With zero noise u_t* is the grid vector ``predict`` interpolates its mean from; its covariance is
the SKI model's posterior covariance K_UU - K_UU W^T K~^-1 W K_UU.

:class:`GridSampler` draws the priors u_t on the device (include/runlmc_hip.h: rl_sampler_*):
per top row either the polynomial form (rows the grid operator runs as Phi C Phi^T) or circulant
embedding of the extended row, whose length it doubles until the spectrum is non-negative."""
import collections
import logging

import numpy as np
import torch

from .iterative import Iterative
from .._native import Sampler, normal_fill, pathwise_residual, sampler_length
from .._lib import as_f64
from ..kern.stationary import Lags, kernel_values

_LOG = logging.getLogger(__name__)

CLIP_TOL = 1e-12       # share of the spectrum an embedding may clip before the ladder goes on

RowStats = collections.namedtuple('RowStats', 'form Ls rank clipped')
PathwiseSolve = collections.namedtuple('PathwiseSolve',
                                       'draws solver iterations max_residual istop')


class _Impulse:
    """T = I: the top row of the reference's identity terms (lmc/grid_kernel.py)."""

    @staticmethod
    def from_dist(d):
        return (np.asarray(d) == 0).astype(float)


def channel_matrix(a, kappa, D):
    """F = [A^T, diag sqrt(kappa)] without its zero columns (at least one column is kept):
    F F^T = A^T A + diag(kappa)."""
    a = np.zeros((0, D)) if a is None else np.atleast_2d(as_f64(a)).reshape(-1, D)
    kappa = as_f64(kappa).reshape(D)
    if np.any(kappa < 0):
        raise ValueError('coreg_diags must be non-negative')
    F = np.hstack([a.T, np.diag(np.sqrt(kappa))])
    keep = np.any(F != 0.0, axis=0)
    if not keep.any():
        keep[0] = True
    return np.ascontiguousarray(F[:, keep])


def poly_sqrt(C):
    """(G, clipped): G G^T = C with its negative eigenvalues set to zero, and their share
    sum |w_-| / sum |w|."""
    C = 0.5 * (C + C.T)
    w, V = np.linalg.eigh(C)
    tot = np.abs(w).sum()
    clipped = float(-w[w < 0].sum() / tot) if tot > 0 else 0.0
    return np.ascontiguousarray(V * np.sqrt(np.clip(w, 0.0, None))), clipped


class GridSampler:
    """Prior draws u ~ N(0, sum_q B_q (x) T_q) of one grid term on the device.

    grid_kernel: the term's GridKernel (or its GridOp), holding the CURRENT parameters;
    kernels[q].from_dist (from_lags for a Separable) gives top row q at any distance; coreg_vecs[q] (R_q, D) or None,
    coreg_diags[q] (D,); axes: the grid's axes (one or two regular arrays).
    forms: None -- rows the operator runs in its polynomial form take it, the others embed;
    'embedding' -- every row embeds.  max_embed: the embedding is at most that multiple of the
    grid (doubling from 2) -- past it the last length is kept, a warning logged and the clipped
    share reported in .stats (RowStats per row: form, Ls, rank, clipped)."""

    def __init__(self, grid_kernel, kernels, coreg_vecs, coreg_diags, axes, max_embed=16,
                 forms=None):
        op = getattr(grid_kernel, '_op', grid_kernel)
        self.grid = op
        if op.sizes is not None and len(op.sizes) > 2:
            raise NotImplementedError(
                'no function draws on a 3-D grid: the sampler embeds one- and two-dimensional '
                'grids only')
        kernels, coreg_vecs, coreg_diags = list(kernels), list(coreg_vecs), list(coreg_diags)
        eye = getattr(grid_kernel, '_eye', 0)
        if eye:
            kernels.append(_Impulse)
            coreg_vecs.append(None)
            coreg_diags.append(float(eye) * np.ones(op.D))
        Q = len(kernels)
        if Q != op.Q or len(coreg_vecs) != Q or len(coreg_diags) != Q:
            raise ValueError('need one kernel, coreg_vec block and coreg_diag per top row (%d)' % op.Q)
        if forms not in (None, 'embedding'):
            raise ValueError("forms must be None or 'embedding'")
        if max_embed < 2:
            raise ValueError('max_embed must be >= 2')
        axes = [as_f64(a).reshape(-1) for a in axes]
        sizes = tuple(len(a) for a in axes)
        if int(np.prod(sizes)) != op.m or len(axes) not in (1, 2):
            raise ValueError('axes do not describe the grid of the operator')
        steps = [float(a[1] - a[0]) if len(a) > 1 else 1.0 for a in axes]
        channels = [channel_matrix(a, k, op.D) for a, k in zip(coreg_vecs, coreg_diags)]
        # forms: the polynomial form of a row is the operator's own (verified at its set time)
        row_forms, sq, rank, poly_clip = [0] * Q, [], 0, {}
        if forms is None and len(axes) == 1:
            for q in range(Q):
                try:
                    r, C = op.poly_coeffs(q)
                except NotImplementedError:
                    r = 0
                if r and op.top_forms()[0][q] == 1:
                    G, poly_clip[q] = poly_sqrt(C)
                    row_forms[q], rank = 1, r
                    sq.append(G)
        emb = [q for q in range(Q) if row_forms[q] == 0]
        self._h = Sampler(op)

        def set_at(embed):
            """(lengths, clipped) of the sampler set at `embed` x the grid; NotImplementedError
            past a limit of the device code (total length, length per axis of a 2-D grid)."""
            lengths, ext = None, None
            if emb:
                lengths = tuple(sampler_length(op.lib, embed * n) for n in sizes)
                lags = np.meshgrid(*[h * np.arange(n // 2 + 1) for h, n in zip(steps, lengths)],
                                   indexing='ij')
                dist = np.sqrt(sum(np.square(g) for g in lags))
                # (a Separable row is evaluated at the mesh's per-axis lags, axis order = the grid's)
                at = Lags(lags, dist)
                ext = [as_f64(kernel_values(kernels[q], at)) for q in emb]
            return lengths, self._h.set(channels, row_forms, lengths, ext, rank, sq)

        embed = 2
        lengths, clipped = set_at(embed)
        worst = max([clipped[q] for q in emb], default=0.0)
        limit = None
        while worst > CLIP_TOL and 2 * embed <= max_embed:
            try:
                lengths, clipped = set_at(2 * embed)
            except NotImplementedError as e:
                # no longer embedding exists on the device: back to the last one that does
                limit = str(e)
                lengths, clipped = set_at(embed)
                break
            embed *= 2
            worst = max([clipped[q] for q in emb], default=0.0)
        if emb and worst > CLIP_TOL:
            _LOG.warning('circulant embedding at %d x the grid (lengths %s) still clips %.3e of a '
                         'spectrum (%s): the draws\' covariance differs from K_UU by about that '
                         'share', embed, lengths, worst,
                         'max_embed = %s' % max_embed if limit is None else limit)
        self.embed = embed
        self.channels = [f.shape[1] for f in channels]
        for q, c in poly_clip.items():
            clipped[q] = c
        self.zlen = self._h.zlen
        self.lengths = lengths if emb else None
        self.stats = [RowStats('polynomial' if row_forms[q] else 'embedding',
                               None if row_forms[q] else (lengths[0] if len(lengths) == 1 else lengths),
                               rank if row_forms[q] else 0, float(clipped[q])) for q in range(Q)]

    def noise(self, seed, draw0, nsamp):
        """The seeded noise of draws draw0 .. draw0 + nsamp (draw0 even): 2 ceil(nsamp / 2) rows."""
        if draw0 % 2:
            raise ValueError('a tile of draws starts at an even draw (pairs share a transform)')
        return normal_fill(self.grid.lib, seed, draw0, 2 * ((nsamp + 1) // 2), self.zlen,
                           self.grid.device)

    def spectrum(self, q):
        """The clipped spectrum of embedding row q as the device uses it, shaped like the
        embedding (test hook: rl_sampler_spectrum_host)."""
        return self._h.spectrum(q, int(np.prod(self.lengths))).reshape(self.lengths)

    def draw(self, Z, nsamp=None):
        """(nsamp, D m) draws on the device from Z (2 ceil(nsamp / 2), zlen)."""
        return self._h.draw(Z, nsamp)


def _solver_name(K):
    from .quadforms import _solver_name as name
    return name(K)


def prior_grid_draws(samplers, Zs, nsamp):
    return [s.draw(Z, nsamp) for s, Z in zip(samplers, Zs)]


def posterior_grid_draws(K, samplers, y, Zs, E, tol=1e-4, maxiter=0):
    """Posterior draws on the grids of the operator K (an LMCOperator): samplers and Zs one per
    term in the operator's term order, y (n,) and E (nsamp, n) on the device.  The solve is
    ``Iterative.solve_device`` (the operator's preconditioner honoured as in training); a
    residual above tol is logged at CRITICAL as the reference logs its own
    (approx/iterative.py:55-58), never raised.  maxiter: the solver's cap (0: the reference's, n
    iterations).  Returns PathwiseSolve."""
    from .iterative import _device_operator
    ski = _device_operator(K)
    lib = ski.lib
    nsamp = E.shape[0]
    if len(samplers) != len(ski.grids) or len(Zs) != len(samplers):
        raise ValueError('need one sampler and one noise buffer per term of the operator')
    U = prior_grid_draws(samplers, Zs, nsamp)
    WU = ski.apply_w(U[0], term=0)
    for t in range(1, len(U)):
        WU += ski.apply_w(U[t], term=t)
    sq = torch.from_numpy(np.sqrt(as_f64(K.Ks[-1].v))).to(ski.device)
    R = pathwise_residual(lib, y, WU, E, sq)
    V, iters, resid, istop = Iterative.solve_device(K, R, tol=tol, maxiter=maxiter)[:4]
    for t, grid in enumerate(ski.grids):
        U[t] += grid.mvm(ski.apply_wt(V, term=t))
    resid = np.asarray(resid, dtype=float)
    worst = float(resid.max()) if resid.size else 0.0
    if not worst < tol:
        _LOG.critical('%d of %d pathwise solves (n = %d) by %s ended with a residual >= %e: '
                      'largest %e', int((~(resid < tol)).sum()), nsamp, K.shape[0], _solver_name(K),
                      tol, worst)
    return PathwiseSolve(U, _solver_name(K), np.asarray(iters), worst, np.asarray(istop))


# noise streams of one seed: the data noise e, the observation noise at test points, then one
# stream per grid term
STREAM_E, STREAM_TEST, STREAM_TERM0 = 0, 1, 2


def stream_seed(seed, stream):
    return (int(seed) * 0x9E3779B97F4A7C15 + int(stream) * 0xD1342543DE82EF95 + int(stream)) & (2 ** 64 - 1)


class PathwiseDraws:
    """A set of function draws, held on the grids (host copies, one (size, D m_t) array per
    term); calling it evaluates the SAME functions at any test inputs."""

    def __init__(self, model, grid_draws, seed, info=None):
        self._model = model
        self.grid_draws = grid_draws          # {active_dims: (size, D m)}
        self.size = next(iter(grid_draws.values())).shape[0]
        self.seed = int(seed)
        self.info = info or []                # one PathwiseSolve-like record per tile (posterior)

    def __call__(self, Xs, noise=False):
        """One (size, len(Xs[d])) array per output, de-normalised; noise=True adds
        observation noise (independent per draw and test point): that of a NEW observation,
        the per-output eps_d alone -- a model's fixed_noise belongs to its training rows (the
        data side of Matheron's rule uses sqrt(eps_d + v_i) per training row, the operator's
        diagonal)."""
        from .interpolation import multi_interpolant
        model = self._model
        if len(Xs) != model.output_dim:
            raise ValueError('need one (possibly empty) input array per output')
        Xs = [np.asarray(X, dtype=float).reshape(len(X), model.input_dim) for X in Xs]
        lens = [len(X) for X in Xs]
        total = sum(lens)
        f = np.zeros((self.size, total))
        if total:
            for ad, U in self.grid_draws.items():
                W = multi_interpolant([X[:, list(ad)] for X in Xs], *model.grid_axes[ad])
                f += W.dot(U.T).T
            if noise:
                K = model._K
                lib = K.device_operator().lib
                e = normal_fill(lib, stream_seed(self.seed, STREAM_TEST), 0, self.size, total,
                                K.device).cpu().numpy()
                f += e * np.sqrt(np.repeat(model._functional_kernel.noise, lens))
        out = np.split(f, np.cumsum(lens)[:-1], axis=1)
        if model.normalizer:
            out = [o * sd + mu for o, (mu, sd) in zip(out, model.normalizer)]
        return out
