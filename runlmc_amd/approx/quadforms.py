"""Quadratic forms  v_t = b_t^T K~^-1 b_t  of many rows b_t, a tile at a time on the device: the
explained part of the predictive variances (reference models/interpolated_llgp.py:358-397, which
builds every b_t on the host and solves them one by one in a process pool).

A tile of `batch` rows is written straight into device memory by a row source, solved with
``Iterative.solve_device`` (so that the operator's ``preconditioner`` is honoured exactly as in
training) and reduced on the device (rl_row_dots); only O(batch) scalars per tile reach the
host.  Row sources:

* :class:`CrossRows`   b_t = K_exact(x_t, X)      -- 'on-the-fly' variances (rl_exact_cross_dev);
* :class:`GridColumnRows`   b_i = W K_UU e_i      -- 'precompute': nu_i = (K_UU W^T K~^-1 W K_UU)_ii
  = b_i^T K~^-1 b_i, since K_UU and K~^-1 are symmetric;
* :class:`UnitRows`   b_t = e_i                    -- (K~^-1)_ii, leave-one-out (approx/loo.py).
"""
import collections
import logging

import numpy as np
import torch

from .iterative import Iterative
from .._native import row_dots

_LOG = logging.getLogger(__name__)

QuadForms = collections.namedtuple('QuadForms', 'v xnorm iterations residuals istop')


class CrossRows:
    """b_t = K_exact(x_t, X): rows of the exact cross-covariance from an ExactOp that holds the
    training points and parameters (set; never assembled).  Xt (nt, P): all test rows, the
    outputs concatenated; lens: their count per output."""

    def __init__(self, op, Xt, lens):
        self.op = op
        self.Xt, self.lens = op._rows(Xt, lens, 'CrossRows')
        self.total_rows = self.Xt.shape[0]
        self._buf = None

    def fill(self, row0, nrows):
        if self._buf is None or self._buf.shape[0] < nrows:
            self._buf = torch.empty((nrows, self.op.n), dtype=torch.float64, device=self.op.device)
        return self.op.cross_device(self.Xt, self.lens, row0, nrows, out=self._buf)


class GridColumnRows:
    """b_i = W K_UU e_i for grid indices i: one-hot grid vectors made on the device, the grid
    product, the interpolation.  `indices`: an explicit list (default: every grid index in
    order)."""

    def __init__(self, grid_kernel, indices=None):
        self.grid = grid_kernel._op
        self.ski = grid_kernel._skiop
        width = self.grid.width
        if indices is None:
            self.indices = None
            self.total_rows = width
        else:
            idx = np.asarray(indices, dtype=np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= width):
                raise ValueError('grid indices must lie in [0, %d)' % width)
            self.indices = torch.from_numpy(idx).to(self.grid.device)
            self.total_rows = idx.size

    def fill(self, row0, nrows):
        dev = self.grid.device
        if self.indices is None:
            idx = torch.arange(row0, row0 + nrows, device=dev)
        else:
            idx = self.indices[row0:row0 + nrows]
        E = torch.zeros((nrows, self.grid.width), dtype=torch.float64, device=dev)
        E[torch.arange(nrows, device=dev), idx] = 1.0
        return self.ski.apply_w(self.grid.mvm(E), term=0)


class UnitRows:
    """b_t = e_i(t): one-hot training rows written on the device, so that quad_forms gives
    (K~^-1)_ii for the indices asked for (default: every row in order) -- leave-one-out
    cross-validation on operators without a factorisation (approx/loo.py)."""

    def __init__(self, n, indices=None, device=None):
        self.n = int(n)
        self.device = device
        if indices is None:
            self.indices = None
            self.total_rows = self.n
        else:
            raw = np.asarray(indices)
            if raw.size and (raw.dtype == bool or not np.issubdtype(raw.dtype, np.integer)):
                raise ValueError('row indices must be integers, got dtype %s' % raw.dtype)
            idx = raw.astype(np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= self.n):
                raise ValueError('row indices must lie in [0, %d)' % self.n)
            self.indices = torch.from_numpy(idx).to(device)
            self.total_rows = idx.size

    def fill(self, row0, nrows):
        if self.indices is None:
            idx = torch.arange(row0, row0 + nrows, device=self.device)
        else:
            idx = self.indices[row0:row0 + nrows]
        E = torch.zeros((nrows, self.n), dtype=torch.float64, device=self.device)
        E[torch.arange(nrows, device=self.device), idx] = 1.0
        return E


def _solver_name(K):
    """The solver ``Iterative.solve_device`` takes for this operator."""
    M = getattr(K, 'preconditioner', None) if Iterative.PRECONDITION else None
    if M is None:
        return 'MINRES' if Iterative.SCIPY_EXITS else 'MINRES (residual rule only)'
    if getattr(M, 'exact', False):
        return 'the direct solve (Woodbury factorisation with iterative refinement)'
    return 'preconditioned conjugate gradients'


def quad_forms(K, row_source, total_rows=None, batch=128, tol=1e-4):
    """v_t = b_t^T K~^-1 b_t for rows 0 .. total_rows of `row_source` (``fill(row0, nrows)`` ->
    device tensor (nrows, n)), `batch` rows per tile.  Returns QuadForms of host arrays, one
    entry per row: v, ||x_t||_2 of the solution, iterations, residual ||b_t - K~ x_t||_2 and
    the solver's exit code.  Rows whose residual misses `tol` are logged once per call at
    CRITICAL (the iterate is kept, as the reference keeps its own: approx/iterative.py:55-58)."""
    total = int(row_source.total_rows if total_rows is None else total_rows)
    batch = int(batch)
    if batch < 1:
        raise ValueError('batch must be >= 1, got %r' % (batch,))
    if total < 0 or total > row_source.total_rows:
        raise ValueError('total_rows must lie in [0, %d]' % row_source.total_rows)
    v, xn, res = np.zeros(total), np.zeros(total), np.zeros(total)
    its, istop = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.int64)
    lib = None
    for row0 in range(0, total, batch):
        nrows = min(batch, total - row0)
        B = row_source.fill(row0, nrows)
        X, it, r, st = Iterative.solve_device(K, B, tol=tol)[:4]
        if lib is None:
            from .iterative import _device_operator
            lib = _device_operator(K).lib
        dots, sq = row_dots(lib, B, X)
        both = torch.stack((dots, sq)).cpu().numpy()          # the tile's 2 x nrows scalars
        sl = slice(row0, row0 + nrows)
        v[sl], xn[sl] = both[0], np.sqrt(both[1])
        its[sl], res[sl], istop[sl] = it, r, st
    missed = np.flatnonzero(~(res < tol))
    if len(missed):
        _LOG.critical('%d of %d variance solves (n = %d) by %s ended with a residual >= %e: '
                      'largest %e (row %d, %d iterations, exit code %d)',
                      len(missed), total, K.shape[0], _solver_name(K), tol, res[missed].max(),
                      missed[np.argmax(res[missed])], its[missed[np.argmax(res[missed])]],
                      istop[missed[np.argmax(res[missed])]])
    return QuadForms(v, xn, its, res, istop)
