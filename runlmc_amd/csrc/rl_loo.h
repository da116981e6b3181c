// Leave-one-out cross-validation from the factorisation of rl_direct.h.
//
// With alpha = K~^-1 y and d = diag(K~^-1) the prediction of observation y_i from all the others
// has mean y_i - alpha_i / d_i and variance 1 / d_i (Rasmussen & Williams 5.4.2).  Everywhere else
// d costs n solves; the Woodbury form K~^-1 = E^-1 + F_q Zs F_q^T (Zs: the scaled map the host
// uploads, dz_Zt) with F block-diagonal by output gives it in ONE pass over the table:
//
//     (K~^-1)_ii = 1 / eps_d(i) + f_i^T Zs[d(i), d(i)] f_i
//
// f_i the R values of row i in the table rp_F, Zs[d, d] the R x R diagonal block of the map: a
// row of F lives in one output's columns, so no other block enters.  When the factorisation is
// a preconditioner P (rl_ski_factor: *available = 2) the same pass is diag(P^-1), the control
// variate of a probe estimate of diag(K~^-1 - P^-1) (k_loo_accumulate).
//
// Cancellation: Zs[d, d] is negative semi-definite, the result is 1 / eps minus a quadratic form
// of almost the same size when eps << K_ii -- its absolute error is a few ulp of 1 / eps, its
// relative error that times K_ii / eps.
#pragma once
#include "rl_device.h"

// ---------------------------------------------------------------------------
// k_dz_diag<R>: out[row(i)] = dinv[i] + sum_j f_i[j] (sum_k Zt[(d, j)][(d, k)] f_i[k]),  d = d(i).
//   grid (ceil(n / 256))   block 256
// A thread owns a data row (the handle's sorted order) and keeps its R table values in registers
// (k_rp_expand's layout).  A wave's 64 rows lie in one output except at an output border, so row
// j of the diagonal block is wave-uniform and comes through scalar loads; the wave at a border
// reads its own output's block per lane.  The outer index j stays a loop (f_i[j] is read again
// from the table, a cache hit: indexing the registers by j would spill them).  Order of
// summation: k ascending in two interleaved chains, then j ascending -- fixed.
//   perm != nullptr: out in the caller's order (row(i) = perm[i]), else row(i) = i.
// ---------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(256)
k_dz_diag(const double* __restrict__ F, int n, int D, const int* __restrict__ out_end,
          const double* __restrict__ Zt, const double* __restrict__ dinv,
          const int* __restrict__ perm, double* __restrict__ out) {
    const int tid = threadIdx.x;
    const int i = blockIdx.x * 256 + tid;
    const int ic = i < n ? i : n - 1;
    double p[R];
#pragma unroll
    for (int k = 0; k < R; ++k) p[k] = F[(size_t)k * n + ic];
    const int wf = blockIdx.x * 256 + (tid & ~63);
    const int wl = wf + 63 < n ? wf + 63 : n - 1;
    const int dfirst = RL_LR_UNIFORM(rp_output_of(out_end, D, wf < n ? wf : n - 1));
    const int dlast = RL_LR_UNIFORM(rp_output_of(out_end, D, wl));
    const size_t Dr = (size_t)D * R;
    double acc = 0.0;
    if (dfirst == dlast) {
        rl_kconst z = RL_KCONST(Zt) + ((size_t)dfirst * R) * Dr + (size_t)dfirst * R;
#pragma unroll 1
        for (int j = 0; j < R; ++j) {
            double zz[R];
#pragma unroll
            for (int k = 0; k < R; ++k) zz[k] = z[k];
            double ev = 0.0, od = 0.0;
#pragma unroll
            for (int k = 0; k + 1 < R; k += 2) {
                ev = fma(zz[k], p[k], ev);
                od = fma(zz[k + 1], p[k + 1], od);
            }
            acc = fma(F[(size_t)j * n + ic], ev + od, acc);
            z += Dr;
        }
    } else {
        const int dmine = rp_output_of(out_end, D, ic);
        const double* z = Zt + ((size_t)dmine * R) * Dr + (size_t)dmine * R;
#pragma unroll 1
        for (int j = 0; j < R; ++j) {
            double ev = 0.0, od = 0.0;
#pragma unroll
            for (int k = 0; k + 1 < R; k += 2) {
                ev = fma(z[k], p[k], ev);
                od = fma(z[k + 1], p[k + 1], od);
            }
            acc = fma(F[(size_t)j * n + ic], ev + od, acc);
            z += Dr;
        }
    }
    if (i < n) out[perm != nullptr ? perm[i] : i] = dinv[i] + acc;
}

// ---------------------------------------------------------------------------
// k_loo_accumulate: with t = Z[v][i] (X[v][i] - C[v][i]) for v = 0 .. nvec - 1 in that order,
//     sum[i] += t,   sumsq[i] += t^2
// -- the running sums of a probe estimate of a diagonal (Z: +-1 rows, X = K~^-1 Z, C = P^-1 Z the
// control variate or nullptr).  A thread owns entry i: rows coalesced, every entry's order over
// v is that of the probes, whatever tiles they arrive in.
//   grid (ceil(n / 256))   block 256
// ---------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_loo_accumulate(const double* __restrict__ Z, const double* __restrict__ X,
                 const double* __restrict__ C, int nvec, long long n, double* __restrict__ sum,
                 double* __restrict__ sumsq) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = sum[i], q = sumsq[i];
    for (int v = 0; v < nvec; ++v) {
        const size_t at = (size_t)v * (size_t)n + (size_t)i;
        const double x = C != nullptr ? X[at] - C[at] : X[at];
        const double t = Z[at] * x;
        s += t;
        q = fma(t, t, q);
    }
    sum[i] = s;
    sumsq[i] = q;
}

// ---------------------------------------------------------------------------
// k_loo_reduce: mean[i] = y[i] - alpha[i] / d[i], var[i] = 1 / d[i] and the log density of y[i]
// under N(mean, var), -log(2 pi var) / 2 - (y - mean)^2 / (2 var) - logscale[i], summed per block
// in a fixed order (block b owns rows [b per, (b + 1) per); thread t rows t, t + 256, ... of
// them; a tree over the 256 threads): part[b] = the block's sum over its valid rows,
// part[RL_LOO_PARTIALS + b] = its count of rows whose d is not a positive finite number.  Such
// a row gets mean = var = NaN and stays out of the sum: reported, never clamped.
//   grid (nblk <= RL_LOO_PARTIALS, include/runlmc_hip.h)   block 256   LDS: 2 x 256 doubles
// ---------------------------------------------------------------------------
static __global__ void __launch_bounds__(256)
k_loo_reduce(const double* __restrict__ y, const double* __restrict__ alpha,
             const double* __restrict__ d, const double* __restrict__ logscale, long long n,
             double* __restrict__ mean, double* __restrict__ var, double* __restrict__ part) {
    RL_SMEM(smem);
    double* red = reinterpret_cast<double*>(smem);        // [2][256]
    const long long per = (n + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    double acc = 0.0, bad = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        const double di = d[i];
        if (!(di > 0.0) || !(di <= 1.79769313486231570e308)) {
            mean[i] = NAN;
            var[i] = NAN;
            bad += 1.0;
            continue;
        }
        const double v = 1.0 / di, dev = alpha[i] / di;
        mean[i] = y[i] - dev;
        var[i] = v;
        // (y - mean)^2 / (2 var) = (alpha / d)^2 d / 2
        double lp = -0.5 * log(6.283185307179586477 * v) - 0.5 * dev * dev * di;
        if (logscale != nullptr) lp -= logscale[i];
        acc += lp;
    }
    red[threadIdx.x] = acc;
    red[256 + threadIdx.x] = bad;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[threadIdx.x] += red[threadIdx.x + h];
            red[256 + threadIdx.x] += red[256 + threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[blockIdx.x] = red[0];
        part[RL_LOO_PARTIALS + blockIdx.x] = red[256];
    }
}
