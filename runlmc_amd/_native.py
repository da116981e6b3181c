"""Thin object wrappers over the C ABI handles (device-resident state).

These are the only places that call into the native library.  torch tensors
are used purely as device-memory handles (allocation + lifetime + streams).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import host_ptr, dev_ptr, as_f64


def _vec_batch(lib, X, width, device):
    """Accept (width,) / (k, width) numpy or torch input, return a contiguous
    float64 tensor of shape (k, width) on `device` plus a flag telling
    whether the input was a single vector."""
    if isinstance(X, torch.Tensor):
        t = X
        if t.dtype != torch.float64:
            raise TypeError('device vectors must be float64')
    else:
        t = torch.from_numpy(as_f64(X))
    single = t.dim() == 1
    if single:
        t = t.unsqueeze(0)
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError('expected vectors of length %d, got shape %s'
                         % (width, tuple(X.shape)))
    return t.to(device).contiguous(), single


class GridOp:
    """Device handle of K_UU = sum_q B_q (x) T_q  (include/runlmc_hip.h)."""

    def __init__(self, D, m, max_tops, device_index=0, lib=None, sizes=None):
        """`m` grid points per output; `sizes=(m1, m2)` (m1*m2 == m) makes the
        kernel matrices BTTB on a two-dimensional grid, `sizes=(m0, m1, m2)` on a
        three-dimensional one (leading axis of at most 64 points)."""
        self.lib = lib or _lib.get_library()
        self.D, self.m, self.max_tops = int(D), int(m), int(max_tops)
        self.device = self.lib.torch_device(device_index)
        self.device_index = device_index
        self._h = ctypes.c_void_p()
        self.sizes = None if sizes is None else tuple(int(v) for v in sizes)
        if self.sizes is None or len(self.sizes) == 1:
            self.lib.call('rl_gridop_create', device_index, self.D, self.m,
                          self.max_tops, ctypes.byref(self._h))
        elif len(self.sizes) == 2:
            if self.sizes[0] * self.sizes[1] != self.m:
                raise ValueError('sizes %s do not multiply to m = %d' % (self.sizes, self.m))
            self.lib.call('rl_gridop_create_2d', device_index, self.D,
                          self.sizes[0], self.sizes[1], self.max_tops,
                          ctypes.byref(self._h))
        elif len(self.sizes) == 3:
            if self.sizes[0] * self.sizes[1] * self.sizes[2] != self.m:
                raise ValueError('sizes %s do not multiply to m = %d' % (self.sizes, self.m))
            self.lib.call('rl_gridop_create_3d', device_index, self.D,
                          self.sizes[0], self.sizes[1], self.sizes[2], self.max_tops,
                          ctypes.byref(self._h))
        else:
            raise NotImplementedError(
                'grids of more than three dimensions have no device path')
        info = [ctypes.c_int() for _ in range(5)]
        self.lib.call('rl_gridop_info', self._h, *[ctypes.byref(i) for i in info])
        self.L, self.N1, self.N2, self.colsA, self.rowsB = [i.value for i in info]
        # three-dimensional grids: leading extent, its embedding length, leading frequencies
        # (the five values above are then those of the inner two-dimensional products)
        lead = [ctypes.c_int() for _ in range(3)]
        self.lib.call('rl_gridop_info_3d', self._h, *[ctypes.byref(i) for i in lead])
        self.m0, self.N0, self.F = [i.value for i in lead]
        self.Q = 0

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self.lib.cdll.rl_gridop_destroy(h)
            self._h = ctypes.c_void_p()

    @property
    def handle(self):
        return self._h

    @property
    def width(self):
        return self.D * self.m

    def form(self):
        """(rank, min_elements): rank r > 0 when the current parameters run
        batches of >= min_elements elements in the polynomial-subspace form
        (csrc/rl_lowrank.h), 0 when on the transform kernels only."""
        r, n = ctypes.c_int(), ctypes.c_longlong()
        self.lib.call('rl_gridop_form', self._h, ctypes.byref(r), ctypes.byref(n))
        return r.value, n.value

    def top_forms(self):
        """(forms, structured): per top row 0 = transform kernels, 1 =
        polynomial-subspace form, 2 = recursive filter (csrc/rl_filter.h);
        structured is True when operator products above the batch gate need
        no transform."""
        forms = (ctypes.c_int * max(self.Q, 1))()
        st = ctypes.c_int()
        self.lib.call('rl_gridop_top_forms', self._h, forms, ctypes.byref(st))
        return [forms[q] for q in range(self.Q)], bool(st.value)

    def form_stats(self, q):
        """What the set-time verification of the polynomial form measured for top row q:
        (trial ratio, tail ratio, estimate of ||T - Phi C Phi^T||_2, estimate of ||T||_2)
        -- include/runlmc_hip.h: rl_gridop_form_stats."""
        out = np.zeros(4)
        self.lib.call('rl_gridop_form_stats', self._h, int(q), host_ptr(out))
        return tuple(float(v) for v in out)

    def poly_coeffs(self, q):
        """(rank, C): C = Phi^T T_q Phi (rank x rank, symmetric) when top row q is in the
        polynomial form for the current parameters, else (0, None) -- include/runlmc_hip.h:
        rl_gridop_poly_coeffs (runs the pending verification)."""
        r = ctypes.c_int()
        buf = np.zeros(48 * 48)
        self.lib.call('rl_gridop_poly_coeffs', self._h, int(q), host_ptr(buf), buf.size,
                      ctypes.byref(r))
        if r.value == 0:
            return 0, None
        return r.value, buf[:r.value * r.value].reshape(r.value, r.value).copy()

    def project(self, G, rank):
        """(k, D, rank) tensor of Phi_rank^T g per output block of the GRID vectors G (k, D*m):
        rl_gridop_project."""
        k = G.shape[0]
        out = torch.empty((k, self.D, int(rank)), dtype=torch.float64, device=self.device)
        self.lib.call('rl_gridop_project', self._h, dev_ptr(G.contiguous()), k, int(rank),
                      dev_ptr(out), self.lib.stream_ptr(self.device))
        return out

    def set_rank_hint(self, rank):
        """First basis size the verification of the polynomial form tries (0: from 24 up)."""
        self.lib.call('rl_gridop_set_rank_hint', self._h, int(rank))

    def set_form_gate(self, min_elements):
        """Smallest batch (nvec*D*m elements) run in the polynomial form;
        0 = every batch, negative = the library default."""
        self.lib.call('rl_gridop_set_form_gate', self._h, int(min_elements))

    def _tops(self, tops):
        tops = as_f64(tops)
        if tops.ndim != 2 or tops.shape[1] != self.m:
            raise ValueError('tops must have shape (Q, %d), got %s'
                             % (self.m, tops.shape))
        return tops

    def set_lmc(self, tops, coreg_vecs, coreg_diags):
        """B_q = A_q^T A_q + diag(kappa_q); coreg_vecs[q] is (R_q, D) (or
        empty), coreg_diags[q] is (D,)."""
        tops = self._tops(tops)
        Q = tops.shape[0]
        if len(coreg_vecs) != Q or len(coreg_diags) != Q:
            raise ValueError('need one coreg_vec block and one coreg_diag per kernel')
        rows, ranks = [], []
        for a in coreg_vecs:
            a = np.zeros((0, self.D)) if a is None else np.atleast_2d(as_f64(a))
            if a.size and a.shape[1] != self.D:
                raise ValueError('coreg_vec block must be (R, %d)' % self.D)
            if a.size:
                # all-zero rows (independent-GP kernels carry one) add nothing
                a = a[np.any(a != 0.0, axis=1)]
            ranks.append(a.shape[0] if a.size else 0)
            if a.size:
                rows.append(a)
        vecs = (np.ascontiguousarray(np.vstack(rows)) if rows
                else np.zeros((0, self.D)))
        diags = np.ascontiguousarray(
            np.vstack([as_f64(k).reshape(1, -1) for k in coreg_diags]))
        if diags.shape != (Q, self.D):
            raise ValueError('coreg_diags must be Q x D')
        ranks = np.ascontiguousarray(np.array(ranks, dtype=np.int32))
        self.lib.call('rl_gridop_set_lmc', self._h, Q, host_ptr(tops),
                      host_ptr(ranks), host_ptr(vecs) if vecs.size else None,
                      host_ptr(diags))
        self.Q = Q

    def set_dense(self, tops, Bs):
        tops = self._tops(tops)
        Q = tops.shape[0]
        Bs = as_f64(Bs)
        if Bs.shape != (Q, self.D, self.D):
            raise ValueError('B must have shape (Q, D, D)')
        self.lib.call('rl_gridop_set_dense', self._h, Q, host_ptr(tops),
                      host_ptr(Bs))
        self.Q = Q

    def mvm(self, X, out=None, top=None):
        """Device-side product; X: (k, D*m) tensor on self.device."""
        k = X.shape[0]
        if out is None:
            out = torch.empty_like(X)
        sp = self.lib.stream_ptr(self.device)
        if top is None:
            self.lib.call('rl_gridop_mvm', self._h, dev_ptr(X), dev_ptr(out), k, sp)
        else:
            self.lib.call('rl_gridop_mvm_top', self._h, int(top), dev_ptr(X),
                          dev_ptr(out), k, sp)
        return out

    def matmat_host(self, X, top=None):
        """numpy in, numpy out; X is (D*m,) or (k, D*m) (vectors as ROWS)."""
        t, single = _vec_batch(self.lib, X, self.width, self.device)
        y = self.mvm(t, top=top).cpu().numpy()
        return y[0] if single else y

    def spectrum(self, q):
        out = np.empty(self.L)
        self.lib.call('rl_gridop_spectrum_host', self._h, int(q), host_ptr(out))
        return out


class SkiOp:
    """Device handle of K~ = W K_UU W^T + diag(eps)."""

    def __init__(self, gridop, W, WT):
        self.lib = gridop.lib
        self.grid = gridop
        self.device = gridop.device
        n, ng = W.shape
        if ng != gridop.width:
            raise ValueError('W has %d columns, grid operator has %d points'
                             % (ng, gridop.width))
        if WT.shape != (ng, n):
            raise ValueError('WT must be the transpose of W')
        W = W.tocsr()
        WT = WT.tocsr()
        self.n = int(n)
        arrs = [np.ascontiguousarray(W.indptr, dtype=np.int32),
                np.ascontiguousarray(W.indices, dtype=np.int32),
                as_f64(W.data),
                np.ascontiguousarray(WT.indptr, dtype=np.int32),
                np.ascontiguousarray(WT.indices, dtype=np.int32),
                as_f64(WT.data)]
        self._h = ctypes.c_void_p()
        self.lib.call('rl_ski_create', gridop.handle, self.n,
                      *[host_ptr(a) for a in arrs], ctypes.byref(self._h))
        self.grids = [gridop]          # grid operator of every term (kept alive)

    @staticmethod
    def _csr_arrays(W, WT):
        W, WT = W.tocsr(), WT.tocsr()
        return [np.ascontiguousarray(W.indptr, dtype=np.int32),
                np.ascontiguousarray(W.indices, dtype=np.int32),
                as_f64(W.data),
                np.ascontiguousarray(WT.indptr, dtype=np.int32),
                np.ascontiguousarray(WT.indices, dtype=np.int32),
                as_f64(WT.data)]

    def add_term(self, gridop, W, WT):
        """Add W_t K_t W_t^T for kernels on another active-dimension set;
        returns the term index."""
        if W.shape != (self.n, gridop.width) or WT.shape != (gridop.width, self.n):
            raise ValueError('interpolant shapes do not match the operator')
        arrs = self._csr_arrays(W, WT)
        self.lib.call('rl_ski_add_term', self._h, gridop.handle,
                      *[host_ptr(a) for a in arrs])
        self.grids.append(gridop)
        return len(self.grids) - 1

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self.lib.cdll.rl_ski_destroy(h)
            self._h = ctypes.c_void_p()

    @property
    def handle(self):
        return self._h

    def set_noise(self, noise, lens):
        noise = as_f64(noise)
        lens = np.ascontiguousarray(np.asarray(lens), dtype=np.int32)
        if noise.shape != (self.grid.D,) or lens.shape != (self.grid.D,):
            raise ValueError('noise and lens must have one entry per output')
        self.lib.call('rl_ski_set_noise', self._h, host_ptr(noise), host_ptr(lens))

    def set_noise_rows(self, noise, lens, extra):
        """K~'s diagonal becomes repeat(noise, lens) + extra: known per-observation variances
        `extra` (n values >= 0, the order of W's rows) on top of the per-output noise
        (rl_ski_set_noise_rows).  A later set_noise returns to the per-output state."""
        noise = as_f64(noise)
        lens = np.ascontiguousarray(np.asarray(lens), dtype=np.int32)
        if noise.shape != (self.grid.D,) or lens.shape != (self.grid.D,):
            raise ValueError('noise and lens must have one entry per output')
        extra = np.ascontiguousarray(as_f64(extra).reshape(-1))
        if extra.shape != (self.n,):
            raise ValueError('extra must have one entry per observation (%d), got %d'
                             % (self.n, extra.size))
        self.lib.call('rl_ski_set_noise_rows', self._h, host_ptr(noise), host_ptr(lens), host_ptr(extra))

    def factor(self):
        """(available, logdet, cond): builds / refreshes the Woodbury factorisation of
        K~ = F M F^T + diag(eps) for the current parameters (include/runlmc_hip.h:
        rl_ski_factor).  available is False when some top row is not in the polynomial
        form (or the operator is otherwise outside it); `reason` then says why."""
        av, ld, cond = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        self.lib.call('rl_ski_factor', self._h, ctypes.byref(av), ctypes.byref(ld),
                      ctypes.byref(cond))
        self.factor_reason = ('' if av.value else
                              self.lib.cdll.rl_last_error().decode())
        # 1: the factorisation is K~^-1 (every top row in the polynomial form); 2: it inverts the
        # operator's projection on the polynomial subspace -- a preconditioner (solve_pcg); 3: the
        # same on the handle's larger basis (up to 192 polynomials per output); 4: the
        # pivoted-Cholesky preconditioner of set_pivchol, where the operator has none of those
        self.factor_mode = int(av.value)
        return bool(av.value), float(ld.value), float(cond.value)

    def set_pivchol(self, rank, rel_tol=1e-10):
        """Opt in to the pivoted-Cholesky preconditioner P = L L^T + diag(eps) of the given rank
        (0 .. 256; 0 switches it off) for operators without a polynomial factorisation
        (rl_ski_set_pivchol).  ValueError for a rank that is not an int in that range."""
        if isinstance(rank, bool) or not isinstance(rank, (int, np.integer)):
            raise ValueError('rank must be an int in 0 .. 256, got %r' % (rank,))
        if not 0 <= int(rank) <= 256:
            raise ValueError('rank must be an int in 0 .. 256, got %r' % (rank,))
        self.lib.call('rl_ski_set_pivchol', self._h, int(rank), float(rel_tol))
        self.pivchol_rank = int(rank)

    def pivchol_info(self):
        """(rank_used, pivots, pivot_values, resid_diag): the state of the pivoted-Cholesky build
        (rl_ski_pivchol_info): pivot rows in the caller's numbering and the residual diagonal at
        each when it was chosen (numpy, one per requested step), the residual diagonal after the
        last step (device tensor (n,), caller's row order)."""
        k = min(int(getattr(self, 'pivchol_rank', 0)), self.n)
        used = ctypes.c_int()
        piv = np.zeros(max(k, 1), dtype=np.int32)
        val = np.zeros(max(k, 1))
        resid = torch.empty((self.n,), dtype=torch.float64, device=self.device)
        self.lib.call('rl_ski_pivchol_info', self._h, ctypes.byref(used), host_ptr(piv),
                      host_ptr(val), dev_ptr(resid))
        return int(used.value), piv[:k], val[:k], resid

    def pivchol_factor(self):
        """L^T as a (rank_used, n) device tensor in the caller's row order: row j is column j of
        the pivoted-Cholesky factor (rl_ski_pivchol_factor)."""
        used = self.pivchol_info()[0]
        out = torch.empty((used, self.n), dtype=torch.float64, device=self.device)
        self.lib.call('rl_ski_pivchol_factor', self._h, dev_ptr(out))
        return out

    def project(self, X):
        """(k, D, r) tensor of Phi^T W^T x per output on the orthonormal polynomials of the
        operator's polynomial form (rl_ski_project); NotImplementedError outside the form."""
        k = X.shape[0]
        r = ctypes.c_int()
        flat = torch.empty((k * self.grid.D * 48,), dtype=torch.float64, device=self.device)
        self.lib.call('rl_ski_project', self._h, dev_ptr(X.contiguous()), k, dev_ptr(flat),
                      ctypes.byref(r), self.lib.stream_ptr(self.device))
        return flat[:k * self.grid.D * r.value].reshape(k, self.grid.D, r.value)

    def precond_sample(self, W):
        """(P^1/2 W rows, log det P): rows of identity covariance (+-1 probes) become rows with the
        covariance P of the operator's current factorisation (rl_ski_precond_sample)."""
        W = W.contiguous()
        out = torch.empty_like(W)
        ld = ctypes.c_double()
        self.lib.call('rl_ski_precond_sample', self._h, dev_ptr(W), dev_ptr(out), W.shape[0],
                      ctypes.byref(ld), self.lib.stream_ptr(self.device))
        return out, float(ld.value)

    def inverse_diag(self):
        """(d, exact): the diagonal of the inverse of the matrix the factorisation inverts, a
        device tensor (n,) in the caller's row order, from one pass over the table of F
        (rl_ski_inverse_diag) -- diag(K~^-1) when exact, diag(P^-1) of the preconditioner when
        not.  NotImplementedError, with the handle's reason, where there is no such diagonal."""
        out = torch.empty((self.n,), dtype=torch.float64, device=self.device)
        exact = ctypes.c_int()
        self.lib.call('rl_ski_inverse_diag', self._h, dev_ptr(out), ctypes.byref(exact),
                      self.lib.stream_ptr(self.device))
        return out, bool(exact.value)

    def precond_apply(self, B):
        """P^-1 B: one application of the operator's factorisation to the rows of B, a (k, n)
        device tensor in the caller's row order (rl_ski_precond_apply)."""
        if B.dim() != 2 or B.shape[1] != self.n:
            raise ValueError('expected rows of length %d, got shape %s' % (self.n, tuple(B.shape)))
        B = B.contiguous()
        out = torch.empty_like(B)
        self.lib.call('rl_ski_precond_apply', self._h, dev_ptr(B), dev_ptr(out), B.shape[0],
                      self.lib.stream_ptr(self.device))
        return out

    def mvm(self, X, out=None):
        if out is None:
            out = torch.empty_like(X)
        self.lib.call('rl_ski_mvm', self._h, dev_ptr(X), dev_ptr(out),
                      X.shape[0], self.lib.stream_ptr(self.device))
        return out

    def apply_wt(self, X, term=0):
        out = torch.empty((X.shape[0], self.grids[term].width), dtype=torch.float64,
                          device=self.device)
        self.lib.call('rl_ski_apply_wt_term', self._h, int(term), dev_ptr(X),
                      dev_ptr(out), X.shape[0], self.lib.stream_ptr(self.device))
        return out

    def apply_w(self, G, term=0):
        out = torch.empty((G.shape[0], self.n), dtype=torch.float64,
                          device=self.device)
        self.lib.call('rl_ski_apply_w_term', self._h, int(term), dev_ptr(G),
                      dev_ptr(out), G.shape[0], self.lib.stream_ptr(self.device))
        return out

    def matmat_host(self, X):
        t, single = _vec_batch(self.lib, X, self.n, self.device)
        y = self.mvm(t).cpu().numpy()
        return y[0] if single else y


MINRES, CG = 0, 1
MINRES_RULE = 2     # MINRES with SciPy's own stopping tests off (include/runlmc_hip.h)


def solve_batch(ski, B, method=MINRES, tol=1e-4, check_every=100, maxiter=0,
                lanczos_cap=0):
    """Device batched solve K~ X = B.  B: (k, n) tensor on ski.device.
    Returns (X tensor, iterations int[k], residuals float[k], istop int[k]);
    with lanczos_cap > 0 (MINRES only) a fifth item, the (k, cap, 2) array of
    Lanczos coefficients (alfa_j, beta_{j+1}) of every system."""
    k = B.shape[0]
    X = torch.empty_like(B)
    iters = np.zeros(k, dtype=np.int32)
    istop = np.zeros(k, dtype=np.int32)
    resid = np.zeros(k, dtype=np.float64)
    if lanczos_cap > 0:
        if method not in (MINRES, MINRES_RULE):
            raise ValueError('Lanczos coefficients come from MINRES only')
        lz = np.zeros((k, int(lanczos_cap), 2), dtype=np.float64)
        ski.lib.call('rl_solve_batch_lanczos', ski.handle, dev_ptr(B), dev_ptr(X),
                     k, int(method), float(tol), int(check_every), int(maxiter),
                     host_ptr(iters), host_ptr(resid), host_ptr(istop),
                     host_ptr(lz), int(lanczos_cap), ski.lib.stream_ptr(ski.device))
        return X, iters, resid, istop, lz
    ski.lib.call('rl_solve_batch', ski.handle, dev_ptr(B), dev_ptr(X), k,
                 int(method), float(tol), int(check_every), int(maxiter),
                 host_ptr(iters), host_ptr(resid), host_ptr(istop),
                 ski.lib.stream_ptr(ski.device))
    return X, iters, resid, istop


def solve_direct(ski, B, tol=1e-4, max_refine=4):
    """Device batched solve K~ X = B through the polynomial form's Woodbury
    factorisation + iterative refinement to the reference's residual rule
    (include/runlmc_hip.h: rl_solve_direct).  Returns (X, iterations, residuals,
    istop); NotImplementedError when the operator has no such form."""
    k = B.shape[0]
    X = torch.empty_like(B)
    iters = np.zeros(k, dtype=np.int32)
    istop = np.zeros(k, dtype=np.int32)
    resid = np.zeros(k, dtype=np.float64)
    if k == 0:
        return X, iters, resid, istop
    ski.lib.call('rl_solve_direct', ski.handle, dev_ptr(B), dev_ptr(X), k, float(tol),
                 int(max_refine), host_ptr(iters), host_ptr(resid), host_ptr(istop),
                 ski.lib.stream_ptr(ski.device))
    return X, iters, resid, istop


def solve_pcg(ski, B, tol=1e-4, maxiter=0):
    """Device batched solve K~ X = B by conjugate gradients preconditioned with the Woodbury
    inverse of the operator's projection on the polynomial subspace (include/runlmc_hip.h:
    rl_solve_pcg).  Returns (X, iterations, residuals, istop)."""
    k = B.shape[0]
    X = torch.empty_like(B)
    iters = np.zeros(k, dtype=np.int32)
    istop = np.zeros(k, dtype=np.int32)
    resid = np.zeros(k, dtype=np.float64)
    if k == 0:
        return X, iters, resid, istop
    ski.lib.call('rl_solve_pcg', ski.handle, dev_ptr(B), dev_ptr(X), k, float(tol), int(maxiter),
                 host_ptr(iters), host_ptr(resid), host_ptr(istop), ski.lib.stream_ptr(ski.device))
    return X, iters, resid, istop


def solve_pcg_lanczos(ski, B, tol=1e-4, maxiter=0, cap=1024):
    """solve_pcg that also returns each system's Lanczos matrix of the PRECONDITIONED operator
    (host (k, cap, 2): diagonal, off-diagonal) and r0^T P^-1 r0 (rl_solve_pcg_lanczos): what
    slq_quadratic_forms takes.  Returns (X, iterations, residuals, istop, lanczos, sqnorms)."""
    k = B.shape[0]
    X = torch.empty_like(B)
    iters = np.zeros(k, dtype=np.int32)
    istop = np.zeros(k, dtype=np.int32)
    resid = np.zeros(k, dtype=np.float64)
    lanczos = np.zeros((k, int(cap), 2), dtype=np.float64)
    sq = np.zeros(k, dtype=np.float64)
    if k == 0:
        return X, iters, resid, istop, lanczos, sq
    ski.lib.call('rl_solve_pcg_lanczos', ski.handle, dev_ptr(B), dev_ptr(X), k, float(tol), int(maxiter),
                 host_ptr(iters), host_ptr(resid), host_ptr(istop), host_ptr(lanczos), int(cap),
                 host_ptr(sq), ski.lib.stream_ptr(ski.device))
    return X, iters, resid, istop, lanczos, sq


def slq_quadratic_forms(lanczos, iters, sqnorms, lib=None):
    """r^T log(K) r for each system from its Lanczos tridiagonal (Gauss
    quadrature): ||r||^2 * sum_j tau_j^2 log(theta_j), (theta, first
    eigenvector components tau) the eigenpairs of T_k.  The library's host helper
    (rl_slq_log_quadrature: implicit QL carrying one eigenvector row, O(k^2) per system, the
    systems over the host's cores) -- LAPACK through SciPy returns whole eigenvector matrices:
    16 ms per system at the 420 steps of a C5 solve, 2 s for its 128 probes."""
    import os
    lib = lib or _lib.get_library()
    lanczos = np.ascontiguousarray(lanczos, dtype=np.float64)
    k = lanczos.shape[0]
    out = np.zeros(k)
    if k == 0:
        return out
    its = np.ascontiguousarray(np.asarray(iters), dtype=np.int32)
    sq = np.ascontiguousarray(np.asarray(sqnorms), dtype=np.float64)
    try:
        cores = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        cores = os.cpu_count() or 1
    lib.call('rl_slq_log_quadrature', host_ptr(lanczos), int(k), int(lanczos.shape[1]),
             host_ptr(its), host_ptr(sq), host_ptr(out), int(max(1, min(cores, 32))))
    failed = np.flatnonzero(np.isnan(out))
    if len(failed):          # (an iteration that did not settle: LAPACK takes those systems)
        out[failed] = slq_quadratic_forms_scipy(lanczos[failed], its[failed], sq[failed])
    return out


def slq_quadratic_forms_scipy(lanczos, iters, sqnorms):
    """The same through SciPy's eigh_tridiagonal (whole eigenvector matrices): the check of
    the library's helper in the tests."""
    from scipy.linalg import eigh_tridiagonal
    out = np.zeros(len(iters))
    for i, k in enumerate(iters):
        k = int(min(k, lanczos.shape[1]))
        if k < 1:
            continue
        d = lanczos[i, :k, 0]
        e = lanczos[i, :k - 1, 1]
        if k == 1:
            theta, tau2 = d[:1], np.ones(1)
        else:
            if not (np.all(np.isfinite(d)) and np.all(np.isfinite(e))):
                out[i] = np.nan          # (a recurrence that left the finite numbers)
                continue
            try:
                theta, vecs = eigh_tridiagonal(d, e)
            except np.linalg.LinAlgError:
                try:
                    theta, vecs = eigh_tridiagonal(d, e, lapack_driver='stev')
                except np.linalg.LinAlgError:
                    out[i] = np.nan
                    continue
            tau2 = vecs[0] ** 2
        keep = theta > 0
        out[i] = sqnorms[i] * np.sum(tau2[keep] * np.log(theta[keep]))
    return out


def cross_dots(lib, U, V, D, m):
    """out[v, a, b] = <U[v, a-th block], V[v, b-th block]> on the device."""
    k = U.shape[0]
    out = torch.empty((k, D, D), dtype=torch.float64, device=U.device)
    lib.call('rl_cross_dots', dev_ptr(U), dev_ptr(V), k, int(D), int(m),
             dev_ptr(out), lib.stream_ptr(U.device))
    return out


def segment_dots(lib, U, V, offsets_dev, D):
    """out[v, d] = sum over output d's slice of U[v] * V[v]."""
    k, n = U.shape
    out = torch.empty((k, D), dtype=torch.float64, device=U.device)
    lib.call('rl_segment_dots', dev_ptr(U), dev_ptr(V), dev_ptr(offsets_dev),
             k, int(n), int(D), dev_ptr(out), lib.stream_ptr(U.device))
    return out


ROW_DOTS_WS = 128       # include/runlmc_hip.h: RL_ROW_DOTS_WS


def row_dots(lib, B, X):
    """(dots, sqnorms) device tensors (k,): sum_i B[v, i] X[v, i] and sum_i X[v, i]^2 in one
    pass, a fixed order of summation (rl_row_dots)."""
    if B.shape != X.shape or B.dim() != 2:
        raise ValueError('row_dots: B and X must be (k, n) tensors of one shape')
    k, n = B.shape
    out = torch.empty((2, k), dtype=torch.float64, device=B.device)
    ws = torch.empty((max(k, 1), ROW_DOTS_WS), dtype=torch.float64, device=B.device)
    lib.call('rl_row_dots', dev_ptr(B), dev_ptr(X), int(k), int(n), dev_ptr(out[0]),
             dev_ptr(out[1]), dev_ptr(ws), lib.stream_ptr(B.device))
    return out[0], out[1]


LOO_PARTIALS = 256      # include/runlmc_hip.h: RL_LOO_PARTIALS


def diag_accumulate(lib, Z, X, C, sum, sumsq):
    """sum[i] += t, sumsq[i] += t^2 for t = Z[v, i] (X[v, i] - C[v, i]), v ascending, in place
    (rl_diag_accumulate).  Z, X, C: (k, n) device tensors, C may be None; sum, sumsq: (n,)."""
    if Z.dim() != 2 or X.shape != Z.shape or (C is not None and C.shape != Z.shape):
        raise ValueError('diag_accumulate: Z, X and C must be (k, n) tensors of one shape')
    k, n = Z.shape
    if sum.shape != (n,) or sumsq.shape != (n,):
        raise ValueError('diag_accumulate: sum and sumsq must have %d entries' % n)
    lib.call('rl_diag_accumulate', dev_ptr(Z), dev_ptr(X),
             dev_ptr(C) if C is not None else ctypes.c_void_p(0), int(k), int(n),
             dev_ptr(sum), dev_ptr(sumsq), lib.stream_ptr(Z.device))
    return sum, sumsq


def loo_reduce(lib, y, alpha, dinv, logscale=None):
    """(mean, var, logp, bad): leave-one-out means y - alpha / d and variances 1 / d as device
    tensors (n,), the sum of the log densities of y under them (minus logscale per row) and
    the count of rows whose d is not a positive finite number -- those hold NaN and are left
    out of the sum (rl_loo_reduce; the block sums are added here in block order)."""
    n = y.shape[0]
    for t in (alpha, dinv) + ((logscale,) if logscale is not None else ()):
        if t.shape != (n,) or y.dim() != 1:
            raise ValueError('loo_reduce: y, alpha, dinv and logscale must be vectors of one length')
    mean, var = torch.empty_like(y), torch.empty_like(y)
    part = torch.zeros((2, LOO_PARTIALS), dtype=torch.float64, device=y.device)
    nblk = ctypes.c_int()
    lib.call('rl_loo_reduce', dev_ptr(y), dev_ptr(alpha), dev_ptr(dinv),
             dev_ptr(logscale) if logscale is not None else ctypes.c_void_p(0), int(n),
             dev_ptr(mean), dev_ptr(var), dev_ptr(part), ctypes.byref(nblk),
             lib.stream_ptr(y.device))
    host = part.cpu().numpy()
    logp = 0.0
    for b in range(nblk.value):
        logp += float(host[0, b])
    return mean, var, logp, int(round(host[1, :nblk.value].sum()))


# ---- exact (dense) likelihood: include/runlmc_hip.h rl_exact_* ----------------------------------
RL_EXACT_SCALED = 16
EXACT_MAX_COLS = 4


def _exact_cols(k):
    ad = list(k.active_dims)
    if not ad:
        raise ValueError('kernel %s has no active dimensions' % k.name)
    if len(ad) > EXACT_MAX_COLS:
        raise NotImplementedError('the exact likelihood takes kernels on at most %d input '
                                  'dimensions, %s has %d' % (EXACT_MAX_COLS, k.name, len(ad)))
    return ad + [-1] * (EXACT_MAX_COLS - len(ad))


def exact_descriptors(kernels):
    """(kinds [Q], params [Q, 4], active columns [Q, 4], parameters per kernel) of the package's
    kernels for rl_exact_set.  A kernel class without a device formula raises
    NotImplementedError naming it: there is no host fallback."""
    from .kern.stationary import RBF, Matern32, Matern52, StdPeriodic, Scaled
    base = {RBF: 0, Matern32: 1, StdPeriodic: 2, Matern52: 3}
    kinds, params, cols, nder = [], [], [], []
    for k in kernels:
        scaled = type(k) is Scaled
        inner = k.k if scaled else k
        if type(inner) not in base:
            raise NotImplementedError(
                'the exact likelihood has no device kernel for %s' % type(inner if scaled else k).__name__)
        kind = base[type(inner)] | (RL_EXACT_SCALED if scaled else 0)
        period = inner.period if type(inner) is StdPeriodic else 0.0
        params.append([inner.inv_lengthscale, period, k.scale if scaled else 0.0, 0.0])
        cols.append(_exact_cols(k))
        kinds.append(kind)
        nder.append((2 if kind & 15 == 2 else 1) + (1 if scaled else 0))
    return (np.array(kinds, dtype=np.int32), np.array(params, dtype=np.float64),
            np.array(cols, dtype=np.int32), nder)


EXACT_MAX_FACT = 3
_EXACT_LEAVES = None


def _exact_leaf_codes():
    global _EXACT_LEAVES
    if _EXACT_LEAVES is None:
        from .kern.stationary import RBF, Matern32, Matern52, StdPeriodic, Cosine
        _EXACT_LEAVES = {RBF: 0, Matern32: 1, StdPeriodic: 2, Matern52: 3, Cosine: 4}
    return _EXACT_LEAVES


def exact_is_composite(kernels):
    """Whether a kernel set needs rl_exact_set_factors: a Product or a Cosine anywhere in it."""
    from .kern.stationary import Cosine, Product, Scaled
    inner = [k.k if type(k) is Scaled else k for k in kernels]
    return any(type(k) in (Product, Cosine) for k in inner)


def exact_factor_descriptors(kernels):
    """(factors per kernel [Q], leaf kinds [Q, 3], leaf parameters [Q, 3, 2], scale flags [Q],
    scales [Q], active columns [Q, 4], parameters per kernel) for rl_exact_set_factors: every
    kernel a (Scaled) leaf or Product of leaves.  Derivatives per kernel: the factors' parameters
    in order, the scale's last.  A class without a device formula raises NotImplementedError
    naming it."""
    from .kern.stationary import Cosine, Product, Scaled, StdPeriodic
    codes = _exact_leaf_codes()
    Q = len(kernels)
    nfact = np.zeros(Q, dtype=np.int32)
    leaves = np.zeros((Q, EXACT_MAX_FACT), dtype=np.int32)
    params = np.zeros((Q, EXACT_MAX_FACT, 2), dtype=np.float64)
    scaled = np.zeros(Q, dtype=np.int32)
    scales = np.zeros(Q, dtype=np.float64)
    cols, nder = [], []
    for q, k in enumerate(kernels):
        inner = k.k if type(k) is Scaled else k
        factors = inner.factors if type(inner) is Product else [inner]
        if len(factors) > EXACT_MAX_FACT:
            raise NotImplementedError('the exact likelihood takes products of at most %d factors, '
                                      '%s has %d' % (EXACT_MAX_FACT, k.name, len(factors)))
        for f, leaf in enumerate(factors):
            if type(leaf) not in codes:
                raise NotImplementedError(
                    'the exact likelihood has no device kernel for %s' % type(leaf).__name__)
            leaves[q, f] = codes[type(leaf)]
            if type(leaf) is Cosine:
                params[q, f, 0] = leaf.frequency
            else:
                params[q, f, 0] = leaf.inv_lengthscale
            if type(leaf) is StdPeriodic:
                params[q, f, 1] = leaf.period
        nfact[q] = len(factors)
        if type(k) is Scaled:
            scaled[q], scales[q] = 1, k.scale
        cols.append(_exact_cols(k))
        nder.append(sum(2 if type(leaf) is StdPeriodic else 1 for leaf in factors) + int(scaled[q]))
    return nfact, leaves, params, scaled, scales, np.array(cols, dtype=np.int32), nder


def exact_is_separable(kernels):
    """Whether a kernel set needs rl_exact_set_separable: a Separable anywhere in it."""
    from .kern.stationary import Scaled, Separable
    return any(type(k.k if type(k) is Scaled else k) is Separable for k in kernels)


def exact_separable_descriptors(kernels):
    """(factors per kernel [Q], leaf kinds [Q, 3], leaf parameters [Q, 3, 2], leaf columns
    [Q, 3, 4], scale flags [Q], scales [Q], parameters per kernel) for rl_exact_set_separable:
    every kernel a (Scaled) leaf, Product of leaves or Separable; the leaves of a kernel on one
    distance all list that kernel's columns.  Derivatives per kernel as exact_factor_descriptors'.
    A kernel the device cannot take raises NotImplementedError naming it."""
    from .kern.stationary import Cosine, Product, Scaled, Separable, StdPeriodic
    codes = _exact_leaf_codes()
    Q = len(kernels)
    nfact = np.zeros(Q, dtype=np.int32)
    leaves = np.zeros((Q, EXACT_MAX_FACT), dtype=np.int32)
    params = np.zeros((Q, EXACT_MAX_FACT, 2), dtype=np.float64)
    lcols = np.full((Q, EXACT_MAX_FACT, EXACT_MAX_COLS), -1, dtype=np.int32)
    scaled = np.zeros(Q, dtype=np.int32)
    scales = np.zeros(Q, dtype=np.float64)
    nder = []
    for q, k in enumerate(kernels):
        inner = k.k if type(k) is Scaled else k
        if type(inner) is Separable:
            pairs = inner.leaves()
        else:
            pairs = [(leaf, k.active_dims) for leaf in
                     (inner.factors if type(inner) is Product else [inner])]
        if len(pairs) > EXACT_MAX_FACT:
            raise NotImplementedError('the exact likelihood takes products of at most %d leaves, '
                                      '%s has %d' % (EXACT_MAX_FACT, k.name, len(pairs)))
        for f, (leaf, dims) in enumerate(pairs):
            if type(leaf) not in codes:
                raise NotImplementedError(
                    'the exact likelihood has no device kernel for %s (in %s)'
                    % (type(leaf).__name__, k.name))
            dims = list(dims if dims is not None else ())
            if not dims:
                raise ValueError('kernel %s has no active dimensions' % k.name)
            if len(dims) > EXACT_MAX_COLS:
                raise NotImplementedError('the exact likelihood takes leaves on at most %d input '
                                          'dimensions, %s of %s has %d'
                                          % (EXACT_MAX_COLS, leaf.name, k.name, len(dims)))
            leaves[q, f] = codes[type(leaf)]
            params[q, f, 0] = leaf.frequency if type(leaf) is Cosine else leaf.inv_lengthscale
            if type(leaf) is StdPeriodic:
                params[q, f, 1] = leaf.period
            lcols[q, f, :len(dims)] = dims
        nfact[q] = len(pairs)
        if type(k) is Scaled:
            scaled[q], scales[q] = 1, k.scale
        nder.append(sum(2 if type(leaf) is StdPeriodic else 1 for leaf, _ in pairs) + int(scaled[q]))
    return nfact, leaves, params, lcols, scaled, scales, nder


class ExactOp:
    """Device handle of the dense exact LMC covariance, its Cholesky factor and K^-1
    (include/runlmc_hip.h: rl_exact_*)."""

    def __init__(self, n, P, device_index=0, lib=None):
        self.lib = lib or _lib.get_library()
        self.n, self.P = int(n), int(P)
        self.device = self.lib.torch_device(device_index)
        self._h = ctypes.c_void_p()
        self.lib.call('rl_exact_create', device_index, self.n, self.P, ctypes.byref(self._h))
        self.D = self.Q = None
        self.nder = []

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self.lib.cdll.rl_exact_destroy(h)
            self._h = ctypes.c_void_p()

    def _rows(self, X, lens, what):
        lens = np.ascontiguousarray(np.asarray(lens), dtype=np.int32)
        if self.D is not None and lens.shape != (self.D,):
            raise ValueError('%s: expected %d output lengths, got shape %s'
                             % (what, self.D, lens.shape))
        X = as_f64(X)
        if X.ndim == 1 and self.P == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape != (int(lens.sum()), self.P):
            raise ValueError('%s: expected inputs of shape (%d, %d), got %s'
                             % (what, int(lens.sum()), self.P, X.shape))
        return np.ascontiguousarray(X), lens

    def set(self, X, lens, kernels, coreg_mats, noise):
        """Data X (n, P) with rows the outputs concatenated, `lens` per output, the kernels
        (runlmc_amd.kern), B_q (Q, D, D) and the noise (D,) -- rl_exact_set, or
        rl_exact_set_factors when the set holds a Product or a Cosine, or rl_exact_set_separable
        when it holds a Separable."""
        separable = exact_is_separable(kernels)
        composite = not separable and exact_is_composite(kernels)
        if separable:
            nfact, leaves, lparams, lcols, scaled, scales, nder = exact_separable_descriptors(kernels)
            kinds = nfact
        elif composite:
            nfact, leaves, lparams, scaled, scales, cols, nder = exact_factor_descriptors(kernels)
            kinds = nfact
        else:
            kinds, params, cols, nder = exact_descriptors(kernels)
        B = as_f64(np.asarray(coreg_mats, dtype=np.float64))
        D = int(np.size(lens))
        if B.shape != (len(kinds), D, D):
            raise ValueError('expected %d coregionalisation matrices of %d x %d, got %s'
                             % (len(kinds), D, D, B.shape))
        noise = as_f64(noise).reshape(-1)
        if noise.shape != (D,):
            raise ValueError('expected %d noise values, got %d' % (D, noise.size))
        self.D = None
        X, lens = self._rows(X, lens, 'rl_exact_set')
        if X.shape[0] != self.n:
            raise ValueError('the handle holds %d points, got %d' % (self.n, X.shape[0]))
        if separable:
            self.lib.call('rl_exact_set_separable', self._h, host_ptr(X), host_ptr(lens), D, len(kinds),
                          host_ptr(nfact), host_ptr(leaves), host_ptr(lparams), host_ptr(lcols),
                          host_ptr(scaled), host_ptr(scales), host_ptr(B), host_ptr(noise))
        elif composite:
            self.lib.call('rl_exact_set_factors', self._h, host_ptr(X), host_ptr(lens), D, len(kinds),
                          host_ptr(nfact), host_ptr(leaves), host_ptr(lparams), host_ptr(scaled),
                          host_ptr(scales), host_ptr(cols), host_ptr(B), host_ptr(noise))
        else:
            self.lib.call('rl_exact_set', self._h, host_ptr(X), host_ptr(lens), D, len(kinds),
                          host_ptr(kinds), host_ptr(params), host_ptr(cols), host_ptr(B), host_ptr(noise))
        self.D, self.Q, self.nder = D, len(kinds), nder

    def set_row_noise(self, extra):
        """Known per-observation variances (n values >= 0, rows as in `set`; None clears them) on
        the diagonal next to the per-output noise: rl_exact_set_row_noise.  Kept across `set`."""
        if extra is None:
            self.lib.call('rl_exact_set_row_noise', self._h, None)
            return
        extra = np.ascontiguousarray(as_f64(extra).reshape(-1))
        if extra.shape != (self.n,):
            raise ValueError('extra must have one entry per observation (%d), got %d'
                             % (self.n, extra.size))
        self.lib.call('rl_exact_set_row_noise', self._h, host_ptr(extra))

    def assemble(self):
        self.lib.call('rl_exact_assemble', self._h)

    def factor(self):
        """log det K; numpy.linalg.LinAlgError naming the column of a bad pivot (as
        scipy.linalg.cho_factor does)."""
        ld, bad = ctypes.c_double(), ctypes.c_int(-1)
        rc = self.lib.cdll.rl_exact_factor(self._h, ctypes.byref(ld), ctypes.byref(bad))
        if rc == _lib.RL_ENOTPD:
            raise np.linalg.LinAlgError(
                '%d-th leading minor of the array is not positive definite (column %d)'
                % (bad.value + 1, bad.value))
        self.lib.check(rc)
        return ld.value

    def solve(self, B):
        """K^-1 B[v] for the rows of B ((k, n) or (n,), numpy or device tensor); a device tensor."""
        t, single = _vec_batch(self.lib, B, self.n, self.device)
        out = torch.empty_like(t)
        self.lib.call('rl_exact_solve', self._h, dev_ptr(t), dev_ptr(out), t.shape[0],
                      self.lib.stream_ptr(self.device))
        return out[0] if single else out

    def explained_variance(self, Xt, test_lens):
        """diag(K_*X K^-1 K_X*) for test rows Xt (nt, P) of outputs test_lens."""
        Xt, tl = self._rows(Xt, test_lens, 'explained_variance')
        out = np.zeros(Xt.shape[0])
        self.lib.call('rl_exact_explained_variance', self._h, host_ptr(Xt), host_ptr(tl),
                      host_ptr(out))
        return out

    def cross(self, Xt, test_lens):
        """Noise-free K(Xt, X), (nt, n)."""
        Xt, tl = self._rows(Xt, test_lens, 'cross')
        out = np.zeros((Xt.shape[0], self.n))
        self.lib.call('rl_exact_cross_host', self._h, host_ptr(Xt), host_ptr(tl), host_ptr(out))
        return out

    def cross_device(self, Xt, test_out_or_lens, row0, nrows, out=None):
        """Rows row0 .. row0 + nrows of the noise-free K(Xt, X) as a DEVICE tensor (nrows, n):
        rl_exact_cross_dev.  Xt (nt, P) holds all test rows, the outputs concatenated;
        `test_out_or_lens` is their length per output (D values).  `out`: a contiguous float64
        device tensor with room for the rows, reused from tile to tile."""
        Xt, tl = self._rows(Xt, test_out_or_lens, 'cross_device')
        row0, nrows = int(row0), int(nrows)
        if out is None:
            out = torch.empty((max(nrows, 1), self.n), dtype=torch.float64, device=self.device)
        elif (out.dtype != torch.float64 or out.device != self.device or not out.is_contiguous()
              or out.numel() < max(nrows, 0) * self.n):
            raise ValueError('out must be a contiguous float64 tensor of >= %d x %d values on %s'
                             % (nrows, self.n, self.device))
        self.lib.call('rl_exact_cross_dev', self._h, host_ptr(Xt), host_ptr(tl), row0, nrows,
                      dev_ptr(out), self.lib.stream_ptr(self.device))
        return out.reshape(-1)[:max(nrows, 0) * self.n].reshape(max(nrows, 0), self.n)

    def dense(self):
        """The whole K, (n, n) on the host."""
        out = np.zeros((self.n, self.n))
        self.lib.call('rl_exact_dense_host', self._h, host_ptr(out))
        return out

    def invert(self):
        self.lib.call('rl_exact_invert', self._h)

    def grad_sums(self, alpha):
        """(S, noise_sums): S[s] = sum over output blocks of M * v_s, M = alpha alpha^T - K^-1,
        v_s = k_q (s = q < Q) then dk_q / dtheta_p in order; noise_sums[d] = sum_{i in d} M_ii
        (rl_exact_grad_sums)."""
        a = alpha if isinstance(alpha, torch.Tensor) else torch.from_numpy(as_f64(alpha))
        a = a.to(self.device, torch.float64).contiguous()
        if a.shape != (self.n,):
            raise ValueError('alpha must have %d entries' % self.n)
        ns, D = self.Q + sum(self.nder), self.D
        out = np.zeros(ns * D * D + D)
        self.lib.call('rl_exact_grad_sums', self._h, dev_ptr(a), host_ptr(out))
        return out[:ns * D * D].reshape(ns, D, D), out[ns * D * D:].copy()


# -- function draws (include/runlmc_hip.h: rl_sampler_*) -------------------------------------------
def sampler_length(lib, want):
    """The smallest embedding length the sampler allows that is >= want (rl_sampler_length)."""
    out = ctypes.c_int()
    lib.call('rl_sampler_length', int(want), ctypes.byref(out))
    return out.value


def normal_fill(lib, seed, draw0, ndraws, zlen, device, out=None):
    """(ndraws, zlen) tensor of standard normals: element (i, j) is a function of
    (seed, draw0 + i, j) only (rl_normal_fill)."""
    ndraws, zlen = int(ndraws), int(zlen)
    if out is None:
        out = torch.empty((ndraws, zlen), dtype=torch.float64, device=device)
    elif tuple(out.shape) != (ndraws, zlen) or out.dtype != torch.float64:
        raise ValueError('out must be a float64 tensor of shape (%d, %d)' % (ndraws, zlen))
    lib.call('rl_normal_fill', int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw0), ndraws, zlen,
             dev_ptr(out), lib.stream_ptr(out.device))
    return out


def pathwise_residual(lib, y, WU, E, sqrt_eps_rows):
    """R[s] = y - WU[s] - sqrt_eps_rows * E[s] on the device (rl_pathwise_residual)."""
    k, n = WU.shape
    if tuple(E.shape) != (k, n) or y.shape[0] != n or sqrt_eps_rows.shape[0] != n:
        raise ValueError('shapes of y, WU, E and sqrt_eps_rows do not match')
    R = torch.empty_like(WU)
    lib.call('rl_pathwise_residual', dev_ptr(y), dev_ptr(WU.contiguous()), dev_ptr(E.contiguous()),
             dev_ptr(sqrt_eps_rows), dev_ptr(R), k, n, lib.stream_ptr(WU.device))
    return R


class Sampler:
    """Device handle of the prior draws u ~ N(0, K_UU) of a grid operator (rl_sampler_*)."""

    def __init__(self, gridop):
        self.lib = gridop.lib
        self.grid = gridop                  # kept alive: the handle borrows it
        self.device = gridop.device
        self._h = ctypes.c_void_p()
        self.lib.call('rl_sampler_create', gridop.handle, ctypes.byref(self._h))
        self.zlen = 0

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self.lib.cdll.rl_sampler_destroy(h)
            self._h = ctypes.c_void_p()

    @property
    def handle(self):
        return self._h

    def set(self, channels, forms, lengths=None, ext_rows=None, poly_rank=0, poly_sqrt=None):
        """channels[q]: F_q (D, C_q); forms[q]: 0 embedding / 1 polynomial; lengths: (Ls,) or
        (N1s, N2s); ext_rows: one array per embedding row; poly_sqrt: one (r, r) array per
        polynomial row.  Returns clipped (Q,) and sets .zlen."""
        Q = len(channels)
        if len(forms) != Q:
            raise ValueError('need one form per row')
        D = self.grid.D
        Fs = [as_f64(f) for f in channels]
        for f in Fs:
            if f.ndim != 2 or f.shape[0] != D or f.shape[1] < 1:
                raise ValueError('channel matrices must be (%d, C) with C >= 1' % D)
        nchan = np.ascontiguousarray([f.shape[1] for f in Fs], dtype=np.int32)
        F = np.ascontiguousarray(np.concatenate([f.reshape(-1) for f in Fs]))
        forms = np.ascontiguousarray(forms, dtype=np.int32)
        lengths = tuple(int(v) for v in (lengths or ()))
        N1s = lengths[0] if lengths else 0
        N2s = lengths[1] if len(lengths) > 1 else 0
        ext = (np.ascontiguousarray(np.concatenate([as_f64(r).reshape(-1) for r in ext_rows]))
               if ext_rows else None)
        if ext is not None:
            per = (N1s // 2 + 1) * ((N2s // 2 + 1) if N2s else 1)
            if ext.size != per * int((forms == 0).sum()):
                raise ValueError('ext_rows must hold %d values per embedding row' % per)
        sq = None
        if poly_sqrt:
            sq = np.ascontiguousarray(np.stack([as_f64(g) for g in poly_sqrt]))
            if sq.shape != (int((forms == 1).sum()), int(poly_rank), int(poly_rank)):
                raise ValueError('poly_sqrt must hold one (r, r) matrix per polynomial row')
        clipped = np.zeros(Q)
        zlen = ctypes.c_longlong()
        self.lib.call('rl_sampler_set', self._h, Q, host_ptr(nchan), host_ptr(F), host_ptr(forms),
                      N1s, N2s, host_ptr(ext), int(poly_rank), host_ptr(sq), host_ptr(clipped),
                      ctypes.byref(zlen))
        self.zlen = int(zlen.value)
        return clipped

    def spectrum(self, q, length):
        """The clipped spectrum of embedding row q (`length` values, natural order): test hook."""
        out = np.empty(int(length))
        self.lib.call('rl_sampler_spectrum_host', self._h, int(q), host_ptr(out))
        return out

    def draw(self, Z, nsamp=None):
        """Z: (2 ceil(nsamp / 2), zlen) noise on the device -> (nsamp, D * m) draws."""
        rows = Z.shape[0]
        nsamp = rows if nsamp is None else int(nsamp)
        if Z.dtype != torch.float64 or Z.dim() != 2 or Z.shape[1] != self.zlen:
            raise ValueError('noise must be a float64 tensor of %d columns' % self.zlen)
        if nsamp < 0 or rows != 2 * ((nsamp + 1) // 2):
            raise ValueError('%d draws need %d rows of noise, got %d'
                             % (nsamp, 2 * ((nsamp + 1) // 2), rows))
        U = torch.empty((nsamp, self.grid.width), dtype=torch.float64, device=self.device)
        self.lib.call('rl_sampler_draw', self._h, dev_ptr(Z.contiguous()), dev_ptr(U), nsamp,
                      self.lib.stream_ptr(self.device))
        return U
