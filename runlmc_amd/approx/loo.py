"""diag(K~^-1) on the device: what leave-one-out cross-validation needs besides alpha.

With alpha = K~^-1 y and d = diag(K~^-1) the prediction of observation y_i from all the others
has mean y_i - alpha_i / d_i and variance 1 / d_i (Rasmussen & Williams 5.4.2).  Three ways to d:

* 'direct'  the operator's Woodbury factorisation IS K~^-1 (csrc/rl_direct.h): one pass over the
  table of F (rl_ski_inverse_diag), no solve;
* 'solve'   d_i = e_i^T K~^-1 e_i for a subset of rows through the tiled quadratic forms of
  approx/quadforms.py, by whatever solver the operator takes: exact up to the solver's `tol`;
* 'probes'  Hutchinson's estimator  d ~ mean_v z_v (.) K~^-1 z_v  over +-1 rows z_v.  Where the
  factorisation is a preconditioner P, diag(P^-1) is known exactly and only the difference is
  estimated:  d ~ diag(P^-1) + mean_v z_v (.) (K~^-1 z_v - P^-1 z_v)  -- the control variate
  ``FactoredInverse.logdet_estimate`` uses for the log det.

Every rank computes the whole thing for itself: no collective appears here (ADVICE.md on lazy
collectives)."""
import collections

import numpy as np
import torch

from .iterative import Iterative, _device_operator
from .quadforms import UnitRows, quad_forms
from .._native import diag_accumulate, normal_fill
from .pathwise import stream_seed

InverseDiagonal = collections.namedtuple('InverseDiagonal', 'd sem method stats')
ProbeStats = collections.namedtuple('ProbeStats', 'n_probes control_variate iterations residuals istop')

METHODS = ('auto', 'direct', 'solve', 'probes')
_STREAM_LOO = 0x4c4f4f        # the probes' stream of a seed (approx/pathwise.py: stream_seed)


def _indices(indices, n):
    if indices is None:
        return None
    raw = np.asarray(indices)
    if raw.size and (raw.dtype == bool or not np.issubdtype(raw.dtype, np.integer)):
        raise ValueError('row indices must be integers, got dtype %s' % raw.dtype)
    idx = raw.astype(np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError('row indices must lie in [0, %d)' % n)
    return idx


def _why_not_direct(ski):
    if ski.factor_mode == 0:
        return ski.factor_reason
    if ski.factor_mode == 4:
        return ('the factorisation of this operator is the pivoted-Cholesky preconditioner '
                '(rl_ski_factor: available = 4), not K~^-1: it has no inverse diagonal')
    return ('the factorisation of this operator is a preconditioner, not K~^-1 (rl_ski_factor: '
            'available = %d): not every top row is in the polynomial form' % ski.factor_mode)


def device_probes(lib, seed, v0, k, n, device):
    """+-1 rows v0 .. v0 + k of the stream (seed, v): entry (v, i) is the sign of the counter-
    based normal (seed, v, i) of rl_normal_fill -- a function of its address only, not of how
    the probes are tiled."""
    Z = normal_fill(lib, stream_seed(seed, _STREAM_LOO), int(v0), int(k), int(n), device)
    return torch.where(Z < 0, -1.0, 1.0).to(torch.float64)


def _probe_estimate(K, ski, probes, n_probes, seed, batch, tol, control_variate):
    n, dev, lib = ski.n, ski.device, ski.lib
    if probes is not None:
        P = probes if isinstance(probes, torch.Tensor) else torch.from_numpy(np.asarray(probes))
        if P.dim() != 2 or P.shape[1] != n:
            raise ValueError('probes must have shape (k, %d), got %s' % (n, tuple(P.shape)))
        if P.numel() and not bool((P.abs() == 1).all()):
            raise ValueError('probes must be rows of +-1')
        k = int(P.shape[0])
    else:
        if isinstance(n_probes, bool) or not isinstance(n_probes, (int, np.integer)):
            raise ValueError('n_probes must be an integer >= 1, got %r' % (n_probes,))
        k = int(n_probes)
    if k < 1:
        raise ValueError('need at least one probe')
    ski.factor()
    cv = bool(control_variate) and ski.factor_mode in (1, 2)
    d0 = ski.inverse_diag()[0] if cv else torch.zeros(n, dtype=torch.float64, device=dev)
    s1 = torch.zeros(n, dtype=torch.float64, device=dev)
    s2 = torch.zeros(n, dtype=torch.float64, device=dev)
    its, res, stop = [], [], []
    for v0 in range(0, k, batch):
        kk = min(batch, k - v0)
        if probes is not None:
            Z = P[v0:v0 + kk].to(dev).to(torch.float64).contiguous()
        else:
            Z = device_probes(lib, seed, v0, kk, n, dev)
        X, it, r, st = Iterative.solve_device(K, Z, tol=tol)[:4]
        C = ski.precond_apply(Z) if cv else None
        diag_accumulate(lib, Z, X.contiguous(), C, s1, s2)
        its.append(np.asarray(it))
        res.append(np.asarray(r))
        stop.append(np.asarray(st))
    m = s1 / k
    d = d0 + m
    if k > 1:
        sem = torch.sqrt(torch.clamp(s2 / k - m * m, min=0.0) / (k - 1))
    else:
        sem = torch.full_like(d, float('nan'))
    return d, sem, ProbeStats(k, cv, np.concatenate(its), np.concatenate(res), np.concatenate(stop))


def inverse_diagonal(K, method='auto', indices=None, probes=None, n_probes=32, seed=0, batch=128,
                     tol=1e-4, control_variate=True):
    """diag(K~^-1) of the LMC operator K, or its entries `indices` (rows of the caller's order).

    Returns InverseDiagonal(d, sem, method, stats): d a float64 tensor on the operator's device,
    one entry per row (per index when `indices` is given); sem the standard error of the probe
    estimate, entry by entry (a tensor like d), or 0.0 for the methods that do not sample; the
    method that ran; its statistics (None, QuadForms or ProbeStats).

    method: 'direct' (needs the factorisation to be K~^-1, NotImplementedError with the handle's
    reason otherwise; no solve), 'solve' (one tolerance-`tol` solve per row, `batch` a tile),
    'probes' (+-1 rows from `probes`, shape (k, n), or `n_probes` rows drawn on the device from
    (seed, v); `batch` rows a tile, solves at `tol`; control_variate=False leaves P^-1 out) or
    'auto': 'direct' where it is exact, else 'solve' when `indices` is given, else 'probes'."""
    if method not in METHODS:
        raise ValueError('method must be one of %s, got %r' % (METHODS, method))
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError('batch must be an integer >= 1, got %r' % (batch,))
    batch = int(batch)
    ski = _device_operator(K)
    n, dev = ski.n, ski.device
    idx = _indices(indices, n)
    if method == 'auto':
        ski.factor()
        method = 'direct' if ski.factor_mode == 1 else ('solve' if idx is not None else 'probes')
    if method == 'direct':
        ski.factor()
        if ski.factor_mode != 1:
            raise NotImplementedError("inverse_diagonal(method='direct'): " + _why_not_direct(ski))
        d, exact = ski.inverse_diag()
        assert exact
        sem, stats = 0.0, None
    elif method == 'solve':
        rows = UnitRows(n, idx, dev)
        stats = quad_forms(K, rows, rows.total_rows, batch, tol)
        return InverseDiagonal(torch.from_numpy(stats.v).to(dev), 0.0, method, stats)
    else:
        d, sem, stats = _probe_estimate(K, ski, probes, n_probes, seed, batch, float(tol), control_variate)
    if idx is not None:
        sel = torch.from_numpy(idx).to(dev)
        d = d[sel]
        if isinstance(sem, torch.Tensor):
            sem = sem[sel]
    return InverseDiagonal(d, sem, method, stats)
