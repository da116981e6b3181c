// Per-observation noise variances (rl_ski_set_noise_rows, rl_exact_set_row_noise).
//
// With e_i = eps_d(i) + v_i (v_i >= 0 given by the caller, never a parameter) the operator is
//
//     K~ = F M F^T + diag(e) = E^1/2 (F~ M F~^T + I) E^1/2,     F~ = diag(e^-1/2) F,
//
// so the factorisation of rl_direct.h runs unchanged on a UNIT-noise problem whose table is F~:
//
//     K~^-1 b    = e^-1/2 (.) A (e^-1/2 (.) b),   A = (F~ M F~^T + I)^-1 = I + F~_q Zs F~_q^T
//     log det K~ = sum_i log e_i + log det (I + L^T M L),   L L^T = F~_d^T F~_d per output
//     (K~^-1)_ii = (1 + f~_i^T Zs[d, d] f~_i) / e_i
//
// The projection, the dense map and the expansion (k_rp_project / k_dz_mix / k_rp_expand,
// k_dz_diag) are the kernels of the constant-noise path with F~ as their table and a diagonal of
// ones; what is new is below: the scaled table (once per noise update), the two row scalings
// around the apply, and the diagonal of the dense exact matrix.  Plain loads, stores and
// multiplies: the emulator compiles them as they stand.
#pragma once
#include "rl_device.h"

// ---------------------------------------------------------------------------
// k_rn_table: Ft[k][i] = isq[i] F[k][i]  (degree-major tables of R columns, n rows; isq = e^-1/2
// in the handle's internal row order).   grid (ceil(n / 256), R)   block 256
// ---------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_rn_table(const double* __restrict__ F, const double* __restrict__ isq, int n, double* __restrict__ Ft) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t e = (size_t)blockIdx.y * n + i;
    Ft[e] = isq[i] * F[e];
}

// ---------------------------------------------------------------------------
// k_rn_scale: X[v][i] *= d[i], in place (the e^-1/2 on either side of the unit-noise apply, the
// e^1/2 behind its square-root factor).   grid (nblk, nvec)   block 256
// ---------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_rn_scale(double* __restrict__ X, const double* __restrict__ d, int n) {
    const int v = blockIdx.y;
    const int per = (n + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    double* px = X + (size_t)v * n;
    for (int i = lo + threadIdx.x; i < hi; i += 256) px[i] *= d[i];
}

// ---------------------------------------------------------------------------
// k_rn_scale_rows: out[row(i)] *= d[i], row(i) = perm[i] (perm != nullptr: out is in the caller's
// order, d in the internal one, as k_dz_diag leaves its result) or i.   grid (ceil(n / 256))   block 256
// ---------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_rn_scale_rows(double* __restrict__ out, const double* __restrict__ d, const int* __restrict__ perm, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[perm != nullptr ? perm[i] : i] *= d[i];
}

// ---------------------------------------------------------------------------
// k_rn_add_diag: out[i][i + diag_off] += extra[i + diag_off] for i < nrows with i + diag_off < ncols
// (the rows [diag_off, diag_off + nrows) of the dense exact matrix, leading dimension ldo).
//   grid (ceil(nrows / 256))   block 256
// ---------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_rn_add_diag(double* __restrict__ out, long long ldo, int nrows, int ncols,
              const double* __restrict__ extra, int diag_off) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows) return;
    const long long j = (long long)i + diag_off;
    if (j >= ncols) return;
    out[(long long)i * ldo + j] += extra[j];
}
