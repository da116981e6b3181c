// Dense fp64 kernels of the exact LMC likelihood (rl_exact.hip) and the blocked Cholesky they
// are built around.  The factorisation kernels (k_ex_potrf_diag, k_ex_trsm_panel, k_ex_gemm,
// k_ex_reduce, k_ex_trsv_diag, k_ex_trtri_diag) know nothing of the likelihood: a symmetric
// positive definite n x n matrix, row-major, leading dimension lda, lower triangle used.
//
// Layout and limits (rl_exact.hip checks them and answers RL_ELIMIT / RL_ENOMEM past them):
//   - tiles of EX_T = 64 rows / columns; every offset is 64-bit (n^2 > 2^31 from n ~ 46 000);
//   - one n x n buffer, plus O(n * 64) workspaces: n is bounded by free device memory;
//   - kernel descriptors: at most EX_MAX_SLOT = 32 values of k_q and dk_q / dtheta_p in all
//     (Q + sum_q p_q), EX_MAX_COLS = 4 active input columns per kernel, D <= EX_MAX_D = 64;
//   - a latent kernel is c prod_f k_f(r) of 1 .. EX_MAX_FACT = 3 leaf kernels on one distance
//     (ex_desc / ex_eval_fact below): at most 2 * 3 + 1 = 7 derivatives per kernel; a separable
//     set gives every leaf a distance over its own <= EX_MAX_COLS columns (ex_eval_sep).
//
// k_ex_gemm is the one update every blocked step uses (trailing SYRK of the factorisation,
// off-diagonal blocks of the triangular solves, L^-1 and L^-T L^-1): C (+)= s A B^T on 64 x 64
// tiles of C, A and B addressed through (row, k) strides so that transposed operands need no
// copy.  On gfx950 the tile runs on v_mfma_f64_16x16x4_f64 (four waves, a 32 x 32 quadrant
// each); under RL_EMU (tests/emu) a thread sums 16 entries of the tile itself -- the matrix-core
// body is exercised only by the GPU tests.
#pragma once
#include "rl_device.h"

#define EX_T 64
#define EX_KC 32                    // k columns of A and B staged in LDS per step
#define EX_LDK (EX_KC + 1)          // padded LDS row (odd: rows of a quarter wave on other banks)
#define EX_LDT (EX_T + 1)
#define EX_MAX_SLOT 32
#define EX_MAX_COLS 4
#define EX_MAX_D 64

#define EX_RBF 0
#define EX_MATERN32 1
#define EX_STDPERIODIC 2
#define EX_MATERN52 3
#define EX_COSINE 4                 // cos(2 pi f r), prm[0] = f: only as a factor (rl_exact_set_factors)
#define EX_SCALED 16
#define EX_MAX_FACT 3
#define EX_PRM2 (4 * EX_MAX_SLOT)    // where the parameters of factors 1, 2 begin, see ex_desc

#if !defined(RL_EMU)
typedef double ex_d4 __attribute__((ext_vector_type(4)));
#endif

// not a positive finite number (NaN included)
__device__ __forceinline__ bool ex_bad_pivot(double p) { return !(p > 0.0 && p <= 1.7976931348623157e308); }

// ---------------------------------------------------------------------------
// one stationary kernel at distance r: v[0] = k(r), v[1 ..] = dk / dtheta_p in the order of
// runlmc_amd/kern/stationary.py (kernel_gradient), the same formulas term by term.
// prm: [inverse lengthscale, period, scale, -].  Returns the number of derivatives.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int ex_eval(int kind, const double* prm, double r, double v[4]) {
    const double g = prm[0];
    int np;
    switch (kind & 15) {
    case EX_RBF: {
        const double sq = r * r;
        const double e = exp(-0.5 * sq * g);
        v[0] = e;
        v[1] = e * (-0.5 * sq);
        np = 1;
        break;
    }
    case EX_MATERN32: {
        const double root3r = r * 1.7320508075688772;
        const double s = root3r * g;
        const double e = exp(-s);
        v[0] = (1.0 + s) * e;
        v[1] = (1.0 + s) * (-root3r * e) + root3r * e;
        np = 1;
        break;
    }
    case EX_MATERN52: {
        const double root5r = r * 2.23606797749979;
        const double s = root5r * g;
        const double e = exp(-s);
        v[0] = (1.0 + s + s * s / 3.0) * e;
        v[1] = -(root5r * s / 3.0) * (1.0 + s) * e;
        np = 1;
        break;
    }
    default: {      // EX_STDPERIODIC (rl_exact_set admits no other kind)
        const double T = prm[1];
        const double arg = 3.141592653589793 / T * r;
        const double s = sin(arg);
        const double ds = cos(arg) * arg * (-1.0 / T * g);
        const double sq = s * s;
        const double e = exp(-0.5 * sq * g);
        v[0] = log(T) < -200.0 ? __builtin_nan("") : e;     // stationary.py: from_dist
        v[1] = e * (-0.5 * sq);
        v[2] = e * (-1.0 * s * ds);
        np = 2;
        break;
    }
    }
    if (kind & EX_SCALED) {
        const double c = prm[2];
        v[np + 1] = v[0];
        for (int p = 1; p <= np; ++p) v[p] = c * v[p];
        v[0] = c * v[0];
        ++np;
    }
    return np;
}

// number of parameters of a kernel kind (derivatives ex_eval returns)
__device__ __host__ __forceinline__ int ex_nder(int kind) {
    return ((kind & 15) == EX_STDPERIODIC ? 2 : 1) + ((kind & EX_SCALED) ? 1 : 0);
}

// ---------------------------------------------------------------------------
// The descriptor of one latent kernel c prod_{f < nf} k_f(r) on the device: an int
//   leaf_0 | (scaled ? EX_SCALED : 0) | (nf - 1) << 5 | leaf_1 << 8 | leaf_2 << 12
// with its parameters in two places of one array: prm[4 q ..] = [g_0, T_0, c, -], ex_eval's
// own layout, and prm[EX_PRM2 + 4 q ..] = [g_1, T_1, g_2, T_2] (g: the leaf's first parameter,
// T: a periodic leaf's period).  With one factor these are ex_eval's kind and prm.
// ---------------------------------------------------------------------------
__device__ __host__ __forceinline__ int ex_desc(const int* leaf, int nf, bool scaled) {
    return leaf[0] | (scaled ? EX_SCALED : 0) | (nf - 1) << 5 | (nf > 1 ? leaf[1] << 8 : 0) |
           (nf > 2 ? leaf[2] << 12 : 0);
}
__device__ __host__ __forceinline__ int ex_desc_nf(int desc) { return ((desc >> 5) & 3) + 1; }
__device__ __host__ __forceinline__ int ex_desc_leaf(int desc, int f) {
    return f == 0 ? desc & 15 : (desc >> (4 + 4 * f)) & 15;
}
__device__ __host__ __forceinline__ int ex_leaf_nder(int leaf) { return leaf == EX_STDPERIODIC ? 2 : 1; }
// one leaf of a factor list: ex_eval's four, or the cosine (kept out of ex_eval: the kernels of
// plain sets compile without it)
__device__ __forceinline__ void ex_leaf(int leaf, const double* prm, double r, double v[4]) {
    if (leaf == EX_COSINE) {
        const double w = 6.283185307179586 * prm[0] * r;
        v[0] = cos(w);
        v[1] = -(6.283185307179586 * r) * sin(w);
    } else {
        ex_eval(leaf, prm, r, v);
    }
}
// derivatives of a descriptor: the factors' parameters in order, then the scale
__device__ __host__ __forceinline__ int ex_desc_nder(int desc) {
    int np = (desc & EX_SCALED) ? 1 : 0;
    for (int f = 0; f < ex_desc_nf(desc); ++f) np += ex_leaf_nder(ex_desc_leaf(desc, f));
    return np;
}

// ---------------------------------------------------------------------------
// Value and every derivative of c prod_f k_f(r) for a descriptor of at most NF factors, in
// FIXED places (registers, no indexed array):
//   v[0] = c prod_f k_f,   v[1 + 2 f + p] = c dk_f / dtheta_p prod_{g != f} k_g   (product rule),
//   v[7] = prod_f k_f  (the scale's derivative; 0 without a scale).
// Places of absent factors and parameters hold 0.  Every old leaf goes through ex_eval; an absent
// factor counts as the exact constant 1, so a single factor keeps ex_eval's bits, the scale is
// applied as ex_eval applies it, and a NaN leaf value (StdPeriodic's convention) stays NaN.
// ---------------------------------------------------------------------------
// SEP (separable sets, see ex_eval_sep): leaf 0 at r, leaves 1 and 2 at r1 and r2 -- a distance
// per leaf; otherwise every leaf at r and r1, r2 are not read.
template <int NF, bool SEP = false>
__device__ __forceinline__ void ex_eval_fact(int desc, const double* prm, int q, double r, double v[8],
                                             double r1 = 0.0, double r2 = 0.0) {
    const double* p0 = prm + 4 * q;
    const double* p1 = prm + EX_PRM2 + 4 * q;
    const int nf = ex_desc_nf(desc);
    double k[NF], d[NF][2];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        k[f] = 1.0;
        d[f][0] = 0.0;
        d[f][1] = 0.0;
        if (f < nf) {
            const int leaf = ex_desc_leaf(desc, f);
            double t[4];
            ex_leaf(leaf, f == 0 ? p0 : p1 + 2 * (f - 1), SEP ? (f == 0 ? r : f == 1 ? r1 : r2) : r, t);
            k[f] = t[0];
            d[f][0] = t[1];
            if (leaf == EX_STDPERIODIC) d[f][1] = t[2];
        }
    }
    double val = k[0];
#pragma unroll
    for (int f = 1; f < NF; ++f) val = val * k[f];
#pragma unroll
    for (int p = 1; p < 8; ++p) v[p] = 0.0;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        double others = 1.0;
#pragma unroll
        for (int g = 0; g < NF; ++g)
            if (g != f) others = others * k[g];
        v[1 + 2 * f] = d[f][0] * others;
        v[2 + 2 * f] = d[f][1] * others;
    }
    v[0] = val;
    if (desc & EX_SCALED) {
        const double c = p0[2];
        v[7] = val;
#pragma unroll
        for (int p = 1; p < 7; ++p) v[p] = c * v[p];
        v[0] = c * val;
    }
}

// the value alone (kernels of more than one factor; the <1> bodies call ex_eval themselves)
template <int NF>
__device__ __forceinline__ double ex_value(int desc, const double* prm, int q, double r) {
    double v[8];
    ex_eval_fact<NF>(desc, prm, q, r, v);
    return v[0];
}

__device__ __forceinline__ double ex_dist(const double* xa, const double* xb, const int* cols) {
    double s = 0.0;
    for (int c = 0; c < EX_MAX_COLS; ++c) {
        const int col = cols[c];
        if (col < 0) break;
        const double d = xa[col] - xb[col];
        s += d * d;
    }
    return sqrt(s);
}

// ---------------------------------------------------------------------------
// Separable sets (rl_exact_set_separable): a latent kernel is c prod_f k_f(r_f), every leaf on the
// distance over ITS OWN columns.  The kernels below take SEP = true and, in place of the column
// table of the kernels [Q][EX_MAX_COLS], the table of the leaves [Q][EX_MAX_FACT][EX_MAX_COLS]
// (-1 after a leaf's last column).  Each leaf's distance is ex_dist itself, so leaves that share
// their kernel's columns get the bits of the one-distance path.
// ---------------------------------------------------------------------------
#define EX_LEAF_COLS (EX_MAX_FACT * EX_MAX_COLS)

// value and derivatives (ex_eval_fact's fixed places) of separable kernel q between xa and xb;
// lq: the kernel's EX_MAX_FACT column lists
__device__ __forceinline__ void ex_eval_sep(int desc, const double* prm, int q, const double* xa,
                                            const double* xb, const int* lq, double v[8]) {
    const int nf = ex_desc_nf(desc);
    const double r0 = ex_dist(xa, xb, lq);
    const double r1 = nf > 1 ? ex_dist(xa, xb, lq + EX_MAX_COLS) : 0.0;
    const double r2 = nf > 2 ? ex_dist(xa, xb, lq + 2 * EX_MAX_COLS) : 0.0;
    ex_eval_fact<EX_MAX_FACT, true>(desc, prm, q, r0, v, r1, r2);
}

// ---------------------------------------------------------------------------
// out[i][j] = sum_q B_q[oa(i), ob(j)] k_q(r_q(xa_i, xb_j))  (+ noise[oa(i)] where i + diag_off == j)
// for i < nrows, j < ncols; lower != 0 skips tiles above the diagonal.  grid (ceil(ncols / 64),
// ceil(nrows / 64)), block 256: a thread fills 16 entries of a 64 x 64 tile, rows of 64
// consecutive columns per quarter of the block.  NF: the most factors of any kernel of the
// handle (1: plain kernels, ex_eval as it stands; EX_MAX_FACT otherwise).  SEP: see ex_eval_sep
// (NF = EX_MAX_FACT, cols the table of the leaves).
// ---------------------------------------------------------------------------
template <int NF, bool SEP = false>
__global__ void __launch_bounds__(256)
k_ex_assemble(double* __restrict__ out, long long ldo, int nrows, int ncols,
              const double* __restrict__ Xa, const int* __restrict__ oa,
              const double* __restrict__ Xb, const int* __restrict__ ob, int P, int Q,
              const int* __restrict__ kinds, const double* __restrict__ prm,
              const int* __restrict__ cols, const double* __restrict__ Bm, int D,
              const double* __restrict__ noise, int diag_off, int lower) {
    if (lower && blockIdx.x > blockIdx.y) return;
    const int i0 = blockIdx.y * EX_T, j0 = blockIdx.x * EX_T;
    for (int u = 0; u < 16; ++u) {
        const int e = threadIdx.x + 256 * u;
        const int i = i0 + e / EX_T, j = j0 + e % EX_T;
        if (i >= nrows || j >= ncols) continue;
        const int a = oa[i], b = ob[j];
        double acc = 0.0;
        for (int q = 0; q < Q; ++q) {
            if constexpr (SEP) {
                double v[8];
                ex_eval_sep(kinds[q], prm, q, Xa + (long long)i * P, Xb + (long long)j * P,
                            cols + q * EX_LEAF_COLS, v);
                acc += Bm[((long long)q * D + a) * D + b] * v[0];
                continue;
            }
            const double r = ex_dist(Xa + (long long)i * P, Xb + (long long)j * P, cols + q * EX_MAX_COLS);
            if constexpr (NF == 1) {
                double v[4];
                ex_eval(kinds[q], prm + 4 * q, r, v);
                acc += Bm[((long long)q * D + a) * D + b] * v[0];
            } else {
                acc += Bm[((long long)q * D + a) * D + b] * ex_value<NF>(kinds[q], prm, q, r);
            }
        }
        if (noise && i + diag_off == j) acc += noise[a];
        out[(long long)i * ldo + j] = acc;
    }
}

// ---------------------------------------------------------------------------
// The same entries for the wide and short shape of prediction: a few hundred test rows by up to
// 10^6 training columns.  out[t][j] = sum_q B_q[ot(t), ob(j)] k_q(r_q(xt_t, xb_j)), t < nrows,
// j < ncols, no noise.  grid (ceil(ncols / EX_CR_COLS), ceil(nrows / rg)), block EX_CR_COLS.
// A workgroup stages its rg test rows once in LDS -- coordinates and the Q gathered rows
// B_q[ot(t), :] -- and, when stage_cols, the coordinates of its EX_CR_COLS training columns
// (leading dimension ldx, odd: neighbouring threads on other banks).  A thread owns column
// j = blockIdx.x EX_CR_COLS + threadIdx.x: it reads x_j and ob(j) once, loops over the staged
// rows and stores out[t][j], consecutive along j across the wave.  Every entry goes through
// ex_dist / ex_eval (ex_value<NF> past one factor) with the sum over q in k_ex_assemble's order.
// LDS: rg (P + Q D) + (stage_cols ? EX_CR_COLS ldx : 0) doubles (ex_cross_rows sizes rg); SEP
// (ex_eval_sep) reads the leaves' column table where the others read the kernels', nothing more
// is staged.
// ---------------------------------------------------------------------------
#define EX_CR_COLS 256
template <int NF, bool SEP = false>
__global__ void __launch_bounds__(EX_CR_COLS)
k_ex_cross_rows(double* __restrict__ out, long long ldo, int nrows, int ncols, int rg,
                const double* __restrict__ Xt, const int* __restrict__ ot,
                const double* __restrict__ Xb, const int* __restrict__ ob, int P, int Q,
                const int* __restrict__ kinds, const double* __restrict__ prm,
                const int* __restrict__ cols, const double* __restrict__ Bm, int D,
                int stage_cols, int ldx) {
    RL_SMEM(smem);
    double* sx = reinterpret_cast<double*>(smem);      // [rg][P]
    double* sb = sx + (long long)rg * P;               // [rg][Q][D]
    double* sc = sb + (long long)rg * Q * D;           // [EX_CR_COLS][ldx]
    const int tid = threadIdx.x;
    const int t0 = blockIdx.y * rg;
    const int nt = nrows - t0 < rg ? nrows - t0 : rg;
    const long long j = (long long)blockIdx.x * EX_CR_COLS + tid;
    for (int e = tid; e < nt * P; e += EX_CR_COLS) sx[e] = Xt[(long long)t0 * P + e];
    const int QD = Q * D;
    for (int e = tid; e < nt * QD; e += EX_CR_COLS) {
        const int t = e / QD, r = e % QD, q = r / D, b = r % D;
        sb[e] = Bm[((long long)q * D + ot[t0 + t]) * D + b];
    }
    const double* xb = Xb + j * P;
    if (stage_cols) {
        if (j < ncols)
            for (int c = 0; c < P; ++c) sc[tid * ldx + c] = xb[c];
        xb = sc + tid * ldx;
    }
    __syncthreads();
    if (j >= ncols) return;
    const int b = ob[j];
    for (int t = 0; t < nt; ++t) {
        const double* xa = sx + t * P;
        const double* bt = sb + (long long)t * QD + b;
        double acc = 0.0;
        for (int q = 0; q < Q; ++q) {
            if constexpr (SEP) {
                double v[8];
                ex_eval_sep(kinds[q], prm, q, xa, xb, cols + q * EX_LEAF_COLS, v);
                acc += bt[q * D] * v[0];
                continue;
            }
            const double r = ex_dist(xa, xb, cols + q * EX_MAX_COLS);
            if constexpr (NF == 1) {
                double v[4];
                ex_eval(kinds[q], prm + 4 * q, r, v);
                acc += bt[q * D] * v[0];
            } else {
                acc += bt[q * D] * ex_value<NF>(kinds[q], prm, q, r);
            }
        }
        out[(long long)(t0 + t) * ldo + j] = acc;
    }
}

// ---------------------------------------------------------------------------
// Fused row reduction, stage 1: for row v = blockIdx.y and chunk c = blockIdx.x of EX_RD_CHUNKS
// equal chunks of the row, part[v][c] = (sum B[v][i] X[v][i], sum X[v][i]^2) over the chunk:
// threads stride the chunk, then a tree over the block -- a fixed order.  block 256, LDS 512
// doubles.  Stage 2 (k_ex_rowdot_sum): grid ceil(k / 64), block 64, a thread sums its row's
// chunks in order.  No atomics: the same bits from call to call.
// ---------------------------------------------------------------------------
#define EX_RD_CHUNKS 64
__global__ void __launch_bounds__(256)
k_ex_rowdot_part(const double* __restrict__ B, const double* __restrict__ X, long long n,
                 double* __restrict__ part) {
    RL_SMEM(smem);
    double* rd = reinterpret_cast<double*>(smem);      // [256] dots, [256] squares
    const int tid = threadIdx.x;
    const long long len = (n + EX_RD_CHUNKS - 1) / EX_RD_CHUNKS;
    const long long i0 = (long long)blockIdx.x * len;
    const long long i1 = i0 + len < n ? i0 + len : n;
    const double* b = B + (long long)blockIdx.y * n;
    const double* x = X + (long long)blockIdx.y * n;
    double dot = 0.0, sq = 0.0;
    for (long long i = i0 + tid; i < i1; i += 256) {
        const double xi = x[i];
        dot += b[i] * xi;
        sq += xi * xi;
    }
    rd[tid] = dot;
    rd[256 + tid] = sq;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            rd[tid] += rd[tid + w];
            rd[256 + tid] += rd[256 + tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* p = part + ((long long)blockIdx.y * EX_RD_CHUNKS + blockIdx.x) * 2;
        p[0] = rd[0];
        p[1] = rd[256];
    }
}

__global__ void __launch_bounds__(64)
k_ex_rowdot_sum(const double* __restrict__ part, int k, double* __restrict__ dots,
                double* __restrict__ sqn) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= k) return;
    double dot = 0.0, sq = 0.0;
    for (int c = 0; c < EX_RD_CHUNKS; ++c) {
        dot += part[((long long)v * EX_RD_CHUNKS + c) * 2];
        sq += part[((long long)v * EX_RD_CHUNKS + c) * 2 + 1];
    }
    dots[v] = dot;
    sqn[v] = sq;
}

// ---------------------------------------------------------------------------
// Cholesky of the nk x nk diagonal block at (k0, k0) in one workgroup (LDS), in place (lower).
// logd[k0 + r] = log L_rr.  The first column whose pivot is not a positive finite number goes to
// *flag (if smaller than what is there: blocks run in order, one workgroup each); the
// factorisation goes on through NaNs -- nothing traps.  grid 1, block 256.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_ex_potrf_diag(double* __restrict__ A, long long lda, int k0, int nk, double* __restrict__ logd,
                int* __restrict__ flag) {
    RL_SMEM(smem);
    double* s = reinterpret_cast<double*>(smem);       // [64][65]
    const int tid = threadIdx.x;
    double* base = A + (long long)k0 * lda + k0;
    for (int e = tid; e < nk * nk; e += 256) {
        const int r = e / nk, c = e % nk;
        s[r * EX_LDT + c] = c <= r ? base[(long long)r * lda + c] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < nk; ++j) {
        const double piv = s[j * EX_LDT + j];
        const double d = sqrt(piv);
        if (tid == 0 && ex_bad_pivot(piv) && *flag > k0 + j) *flag = k0 + j;
        if (tid > j && tid < nk) s[tid * EX_LDT + j] /= d;
        __syncthreads();
        const int m = nk - j - 1;
        for (int e = tid; e < m * m; e += 256) {
            const int r = j + 1 + e / m, c = j + 1 + e % m;
            if (c <= r) s[r * EX_LDT + c] -= s[r * EX_LDT + j] * s[c * EX_LDT + j];
        }
        if (tid == 0) s[j * EX_LDT + j] = d;
        __syncthreads();
    }
    for (int e = tid; e < nk * nk; e += 256) {
        const int r = e / nk, c = e % nk;
        if (c <= r) base[(long long)r * lda + c] = s[r * EX_LDT + c];
    }
    if (tid < nk) logd[k0 + tid] = log(s[tid * EX_LDT + tid]);
}

// ---------------------------------------------------------------------------
// Panel solve below a factored diagonal block: rows r0 .. r0 + nrows - 1, columns k0 .. k0 + nk - 1
// become  A L_kk^-T.  One 64-row tile per workgroup (block 64: a thread solves its row).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_ex_trsm_panel(double* __restrict__ A, long long lda, int k0, int nk, int r0, int nrows) {
    RL_SMEM(smem);
    double* L = reinterpret_cast<double*>(smem);       // [64][65]
    double* X = L + EX_T * EX_LDT;                     // [64][65]
    const int tid = threadIdx.x;
    const int row0 = r0 + blockIdx.x * EX_T;
    const int rows = nrows - blockIdx.x * EX_T < EX_T ? nrows - blockIdx.x * EX_T : EX_T;
    const double* Lg = A + (long long)k0 * lda + k0;
    double* Xg = A + (long long)row0 * lda + k0;
    for (int e = tid; e < nk * nk; e += 64) {
        const int r = e / nk, c = e % nk;
        L[r * EX_LDT + c] = c <= r ? Lg[(long long)r * lda + c] : 0.0;
    }
    for (int e = tid; e < rows * nk; e += 64) {
        const int r = e / nk, c = e % nk;
        X[r * EX_LDT + c] = Xg[(long long)r * lda + c];
    }
    __syncthreads();
    if (tid < rows) {
        double* x = X + tid * EX_LDT;
        for (int c = 0; c < nk; ++c) {
            double v = x[c];
            for (int t = 0; t < c; ++t) v -= x[t] * L[c * EX_LDT + t];
            x[c] = v / L[c * EX_LDT + c];
        }
    }
    __syncthreads();
    for (int e = tid; e < rows * nk; e += 64) {
        const int r = e / nk, c = e % nk;
        Xg[(long long)r * lda + c] = X[r * EX_LDT + c];
    }
}

// ---------------------------------------------------------------------------
// Inverse of the lower nk x nk diagonal block at (j0, j0), in place, strict upper part of the
// block set to 0 (the blocked L^-1 and L^-T L^-1 read whole diagonal tiles).  grid 1, block 64:
// thread c forms column c by forward substitution.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_ex_trtri_diag(double* __restrict__ A, long long lda, int j0, int nk) {
    RL_SMEM(smem);
    double* L = reinterpret_cast<double*>(smem);       // [64][65]
    double* W = L + EX_T * EX_LDT;
    const int tid = threadIdx.x;
    double* base = A + (long long)j0 * lda + j0;
    for (int e = tid; e < nk * nk; e += 64) {
        const int r = e / nk, c = e % nk;
        L[r * EX_LDT + c] = c <= r ? base[(long long)r * lda + c] : 0.0;
    }
    __syncthreads();
    if (tid < nk) {
        const int c = tid;
        for (int r = 0; r < c; ++r) W[r * EX_LDT + c] = 0.0;
        W[c * EX_LDT + c] = 1.0 / L[c * EX_LDT + c];
        for (int r = c + 1; r < nk; ++r) {
            double v = 0.0;
            for (int t = c; t < r; ++t) v += L[r * EX_LDT + t] * W[t * EX_LDT + c];
            W[r * EX_LDT + c] = -v / L[r * EX_LDT + r];
        }
    }
    __syncthreads();
    for (int e = tid; e < nk * nk; e += 64) {
        const int r = e / nk, c = e % nk;
        base[(long long)r * lda + c] = W[r * EX_LDT + c];
    }
}

// ---------------------------------------------------------------------------
// Triangular solve of the diagonal block (k0, k0) for many right-hand sides stored as rows:
// R[v][k0 .. k0 + nk) := L_kk^-1 (trans = 0) or L_kk^-T (trans = 1) of itself, v < nrhs.
// grid ceil(nrhs / 64), block 64: a thread solves one right-hand side.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_ex_trsv_diag(const double* __restrict__ A, long long lda, int k0, int nk, double* __restrict__ R,
               long long ldr, int nrhs, int trans) {
    RL_SMEM(smem);
    double* L = reinterpret_cast<double*>(smem);
    double* X = L + EX_T * EX_LDT;
    const int tid = threadIdx.x;
    const int v0 = blockIdx.x * EX_T;
    const int nv = nrhs - v0 < EX_T ? nrhs - v0 : EX_T;
    const double* Lg = A + (long long)k0 * lda + k0;
    for (int e = tid; e < nk * nk; e += 64) {
        const int r = e / nk, c = e % nk;
        L[r * EX_LDT + c] = c <= r ? Lg[(long long)r * lda + c] : 0.0;
    }
    for (int e = tid; e < nv * nk; e += 64) {
        const int v = e / nk, c = e % nk;
        X[v * EX_LDT + c] = R[(long long)(v0 + v) * ldr + k0 + c];
    }
    __syncthreads();
    if (tid < nv) {
        double* x = X + tid * EX_LDT;
        if (!trans) {
            for (int c = 0; c < nk; ++c) {
                double s = x[c];
                for (int t = 0; t < c; ++t) s -= L[c * EX_LDT + t] * x[t];
                x[c] = s / L[c * EX_LDT + c];
            }
        } else {
            for (int c = nk - 1; c >= 0; --c) {
                double s = x[c];
                for (int t = c + 1; t < nk; ++t) s -= L[t * EX_LDT + c] * x[t];
                x[c] = s / L[c * EX_LDT + c];
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < nv * nk; e += 64) {
        const int v = e / nk, c = e % nk;
        R[(long long)(v0 + v) * ldr + k0 + c] = X[v * EX_LDT + c];
    }
}

// ---------------------------------------------------------------------------
// k_ex_gemm: for the 64 x 64 tile (blockIdx.y, blockIdx.x) of an M x N result
//   acc[i][j] = sum_{k in split z} A(i, k) B(j, k),   A(i, k) = A[i sai + k sak], B(j, k) = B[j sbj + k sbk]
// over k in [z kchunk, min(K, (z + 1) kchunk)), cut at k < 64 (tile row + 1) when a_lower (A lower
// triangular with explicit zeros above the diagonal of its diagonal tiles).  Then
//   P == NULL:  C[i ldc + j] = (beta ? C : 0) + s acc     (lower_tiles: tiles with column > row skipped)
//   P != NULL:  P[z][i][j] = acc                           (k_ex_reduce sums the splits in order)
// grid (ceil(N / 64), ceil(M / 64), splits), block 256, LDS 2 x 64 x EX_LDK doubles.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_ex_gemm(double* __restrict__ C, long long ldc, const double* __restrict__ A, long long sai,
          long long sak, const double* __restrict__ B, long long sbj, long long sbk, int M, int N,
          int K, int kchunk, int a_lower, double s, int beta, int lower_tiles,
          double* __restrict__ P) {
    const int tn = blockIdx.x, tm = blockIdx.y, z = blockIdx.z;
    if (lower_tiles && tn > tm) return;
    const int i0 = tm * EX_T, j0 = tn * EX_T;
    const int kb = z * kchunk;
    int ke = K < kb + kchunk ? K : kb + kchunk;
    if (a_lower && ke > i0 + EX_T) ke = i0 + EX_T;
    RL_SMEM(smem);
    double* sA = reinterpret_cast<double*>(smem);
    double* sB = sA + EX_T * EX_LDK;
    const int tid = threadIdx.x;
#if !defined(RL_EMU)
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    ex_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = ex_d4{0.0, 0.0, 0.0, 0.0};
#else
    const int er = tid >> 2, ec = (tid & 3) * 16;      // a thread: row er, columns ec .. ec + 15
    double acc[16];
    for (int c = 0; c < 16; ++c) acc[c] = 0.0;
#endif
    for (int k0 = kb; k0 < ke; k0 += EX_KC) {
        // stage A(i0 .. +64, k0 .. +KC) and B(j0 .. +64, k0 .. +KC), the unit-stride index fastest
        for (int e = tid; e < EX_T * EX_KC; e += 256) {
            int r, k;
            if (sak == 1) { r = e / EX_KC; k = e % EX_KC; } else { k = e / EX_T; r = e % EX_T; }
            const int gi = i0 + r, gk = k0 + k;
            sA[r * EX_LDK + k] = gi < M && gk < ke ? A[(long long)gi * sai + (long long)gk * sak] : 0.0;
            if (sbk == 1) { r = e / EX_KC; k = e % EX_KC; } else { k = e / EX_T; r = e % EX_T; }
            const int gj = j0 + r, gk2 = k0 + k;
            sB[r * EX_LDK + k] = gj < N && gk2 < ke ? B[(long long)gj * sbj + (long long)gk2 * sbk] : 0.0;
        }
        __syncthreads();
#if !defined(RL_EMU)
#pragma unroll
        for (int kk = 0; kk < EX_KC; kk += 4) {
            const double a0 = sA[(wm + li) * EX_LDK + kk + lk];
            const double a1 = sA[(wm + 16 + li) * EX_LDK + kk + lk];
            const double b0 = sB[(wn + li) * EX_LDK + kk + lk];
            const double b1 = sB[(wn + 16 + li) * EX_LDK + kk + lk];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
#else
        for (int c = 0; c < 16; ++c)
            for (int kk = 0; kk < EX_KC; ++kk) acc[c] += sA[er * EX_LDK + kk] * sB[(ec + c) * EX_LDK + kk];
#endif
        __syncthreads();
    }
    auto put = [&](int i, int j, double v) {
        if (i >= M || j >= N) return;
        if (P) {
            P[(long long)z * M * N + (long long)i * N + j] = v;
        } else {
            double* c = C + (long long)i * ldc + j;
            *c = beta ? *c + s * v : s * v;
        }
    };
#if !defined(RL_EMU)
    // D of v_mfma_f64_16x16x4_f64: register r of lane l = row (l >> 4) + 4 r, column l & 15
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                put(i0 + wm + 16 * a + lk + 4 * r, j0 + wn + 16 * b + li, acc[a][b][r]);
#else
    for (int c = 0; c < 16; ++c) put(i0 + er, j0 + ec + c, acc[c]);
#endif
}

// C[i ldc + j] = (beta ? C : 0) + s sum_{z < nsplit} P[z][i][j], the splits in order.
__global__ void __launch_bounds__(256)
k_ex_reduce(double* __restrict__ C, long long ldc, const double* __restrict__ P, int M, int N,
            int nsplit, double s, int beta) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long MN = (long long)M * N;
    if (e >= MN) return;
    double acc = 0.0;
    for (int z = 0; z < nsplit; ++z) acc += P[z * MN + e];
    const long long i = e / N, j = e % N;
    double* c = C + i * ldc + j;
    *c = beta ? *c + s * acc : s * acc;
}

// out[v] = sum_i V[v][i]^2 (fixed order); grid nvec, block 256.
__global__ void __launch_bounds__(256)
k_ex_rownorm2(const double* __restrict__ V, long long n, double* __restrict__ out) {
    RL_SMEM(smem);
    double* red = reinterpret_cast<double*>(smem);
    const double* row = V + (long long)blockIdx.x * n;
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) acc += row[i] * row[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// *out = 2 sum_i x[i] (fixed order); grid 1, block 256.
__global__ void __launch_bounds__(256)
k_ex_sum2(const double* __restrict__ x, int n, double* __restrict__ out) {
    RL_SMEM(smem);
    double* red = reinterpret_cast<double*>(smem);
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += x[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = 2.0 * red[0];
}

// ---------------------------------------------------------------------------
// Gradient block sums: one workgroup per entry of `tiles` (r0, c0, a, b): a tile of rows
// [r0, min(r0 + 64, end_a)) and columns [c0, min(c0 + 64, end_b)) of output block (a, b), a >= b,
// of the lower triangle of Kinv.  With M_ij = alpha_i alpha_j - Kinv_ij, weight 2 for i > j
// inside a diagonal block (the upper twin), 1 otherwise, it sums M_ij k_q(r_ij) into slot q,
// M_ij dk_q / dtheta_p into slot dslot[q] + p, and M_ii into slot nslot (noise).  The
// workgroup's nslot + 1 sums go to part[w][.] (fixed order: threads by index).
// block 256, LDS (nslot + 1) x 256 doubles.
// NF == 1 (plain kernels): up to three derivatives from ex_eval, four sums per thread.
// NF > 1: ex_eval_fact's eight fixed places summed in eight registers, then stored to the slots
// dslot[q] + p in the derivative order (factors in order, the scale last).  SEP: the same sums
// with every leaf on its own distance (ex_eval_sep; cols the table of the leaves).
// ---------------------------------------------------------------------------
template <int NF, bool SEP = false>
__global__ void __launch_bounds__(256)
k_ex_grad_tiles(const double* __restrict__ Kinv, long long n, const double* __restrict__ alpha,
                const int* __restrict__ tiles, const int* __restrict__ bounds,
                const double* __restrict__ X, int P, int Q, const int* __restrict__ kinds,
                const double* __restrict__ prm, const int* __restrict__ cols,
                const int* __restrict__ dslot, int nslot, double* __restrict__ part) {
    RL_SMEM(smem);
    double* red = reinterpret_cast<double*>(smem);     // [nslot + 1][256]
    const int tid = threadIdx.x, w = blockIdx.x;
    const int r0 = tiles[4 * w], c0 = tiles[4 * w + 1], a = tiles[4 * w + 2], b = tiles[4 * w + 3];
    const int re = bounds[a + 1] < r0 + EX_T ? bounds[a + 1] : r0 + EX_T;
    const int ce = bounds[b + 1] < c0 + EX_T ? bounds[b + 1] : c0 + EX_T;
    double mw[16];
    double dsum = 0.0;
    for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u;
        const int i = r0 + e / EX_T, j = c0 + e % EX_T;
        double m = 0.0;
        if (i < re && j < ce && (a != b || j <= i)) {
            m = alpha[i] * alpha[j] - Kinv[(long long)i * n + j];
            if (i == j) dsum += m;
            else if (a == b) m *= 2.0;
        }
        mw[u] = m;
    }
    red[nslot * 256 + tid] = dsum;
    for (int q = 0; q < Q; ++q) {
        const int kind = kinds[q];
        const double* pq = prm + 4 * q;
        const int* cq = cols + q * (SEP ? EX_LEAF_COLS : EX_MAX_COLS);
        if constexpr (NF == 1) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int np = 0;
            for (int u = 0; u < 16; ++u) {
                const int e = tid + 256 * u;
                const int i = r0 + e / EX_T, j = c0 + e % EX_T;
                if (i >= re || j >= ce || (a == b && j > i)) continue;
                double v[4];
                np = ex_eval(kind, pq, ex_dist(X + (long long)i * P, X + (long long)j * P, cq), v);
                const double m = mw[u];
                s0 += m * v[0];
                s1 += m * v[1];
                if (np > 1) s2 += m * v[2];
                if (np > 2) s3 += m * v[3];
            }
            np = ex_nder(kind);       // (a thread without entries has summed zeros)
            red[q * 256 + tid] = s0;
            red[(dslot[q] + 0) * 256 + tid] = s1;
            if (np > 1) red[(dslot[q] + 1) * 256 + tid] = s2;
            if (np > 2) red[(dslot[q] + 2) * 256 + tid] = s3;
        } else {
            double s[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) s[p] = 0.0;
            for (int u = 0; u < 16; ++u) {
                const int e = tid + 256 * u;
                const int i = r0 + e / EX_T, j = c0 + e % EX_T;
                if (i >= re || j >= ce || (a == b && j > i)) continue;
                double v[8];
                if constexpr (SEP)
                    ex_eval_sep(kind, prm, q, X + (long long)i * P, X + (long long)j * P, cq, v);
                else
                    ex_eval_fact<NF>(kind, prm, q, ex_dist(X + (long long)i * P, X + (long long)j * P, cq), v);
                const double m = mw[u];
#pragma unroll
                for (int p = 0; p < 8; ++p) s[p] += m * v[p];
            }
            red[q * 256 + tid] = s[0];
            int slot = dslot[q];
            const int nf = ex_desc_nf(kind);
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                if (f >= nf) continue;
                red[slot * 256 + tid] = s[1 + 2 * f];
                if (ex_leaf_nder(ex_desc_leaf(kind, f)) > 1) red[(slot + 1) * 256 + tid] = s[2 + 2 * f];
                slot += ex_leaf_nder(ex_desc_leaf(kind, f));
            }
            if (kind & EX_SCALED) red[slot * 256 + tid] = s[7];
        }
    }
    __syncthreads();
    if (tid <= nslot) {
        double acc = 0.0;
        for (int t = 0; t < 256; ++t) acc += red[tid * 256 + t];
        part[(long long)w * (nslot + 1) + tid] = acc;
    }
}

// out[s][a][b] = out[s][b][a] = sum of the pair's workgroups' slot s (in order), s < nslot;
// out[nslot D^2 + a] = noise slot of pair (a, a).  grid D (D + 1) / 2 pairs, block 64.
__global__ void __launch_bounds__(64)
k_ex_grad_reduce(const double* __restrict__ part, const int* __restrict__ pair_start, int D,
                 int nslot, double* __restrict__ out) {
    const int p = blockIdx.x;
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= p) ++a;
    const int b = p - a * (a + 1) / 2;
    for (int s = threadIdx.x; s <= nslot; s += 64) {
        double acc = 0.0;
        for (int w = pair_start[p]; w < pair_start[p + 1]; ++w) acc += part[(long long)w * (nslot + 1) + s];
        if (s < nslot) {
            out[((long long)s * D + a) * D + b] = acc;
            out[((long long)s * D + b) * D + a] = acc;
        } else if (a == b) {
            out[(long long)nslot * D * D + a] = acc;
        }
    }
}
