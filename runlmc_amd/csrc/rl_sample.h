// Kernels of the function draws (include/runlmc_hip.h: rl_sampler_*, rl_normal_fill,
// rl_pathwise_residual).
//
// A draw of u ~ N(0, sum_q B_q (x) T_q) is u = sum_q (F_q (x) S_q) z_q.  Rows in the embedding
// form take S_q from the circulant of the EXTENDED kernel row: a pair of draws (2p, 2p + 1) is
// the real and the imaginary part of ONE complex inverse transform of
//     Y_a(w) = sum_q s_q(w) sum_c F_q[a][c] (z_{2p} + i z_{2p+1})_{q,c}(w),  s_q = sqrt(lambda_q / Ls).
// The inverse transform runs as the FORWARD flow graph of rl_fft.h on the conjugated input
// (ifft(Y) = conj(fft(conj Y)) without the 1 / Ls, which s_q carries): natural order in -- the
// noise, by far the largest operand, is read in its own order --, digit-scrambled order out,
// and the crop to the grid reads the m positions it needs through a table.
//   k_smp_embed1   Ls <= RL_SAMPLER_LDS_MAX: scale, mix, transform and crop of one (pair, output)
//                  in one workgroup, the transform in LDS.
//   k_smp_cols     longer Ls = N1 N2 (w = n1 N2 + n2, x = k1 + N1 k2): scale, mix and the N1-point
//                  pass over a tile of adjacent columns n2, the inter-pass twiddle
//                  exp(-2 pi i n2 k1 / Ls), intermediates T[pair][a][p1][n2] (p1: scrambled k1).
//   k_smp_rows     the N2-point pass over the rows of `rows` consecutive k1 (each a contiguous
//                  row of T, found through the position table) and the crop: consecutive threads
//                  write consecutive grid points.
// A 2-D grid (N1s x N2s circulant, grid index k1 m2 + k2) is the same two kernels without the
// twiddle.  Rows in the polynomial form (k_smp_poly_coef) only mix r coefficients per channel;
// rl_lowrank.h's k_lr_expand turns them into grid values, accumulating onto the embedding part.
// What bounds them: every kernel streams the noise once per OUTPUT (the D workgroups of a tile
// each read it; they are adjacent in launch order but spread over the XCDs, so they share no L2)
// and does C_q multiply-adds per value read: memory-bound on the noise, DESIGN.md section 7d.
#pragma once
#include "rl_fft.h"

#define RL_SMP_THREADS 256

// one embedding row of the sampler as the kernels see it
struct SmpRows {
    int nemb;               // rows in the embedding form
    const int* C;           // [nemb] channels
    const int* foff;        // [nemb] offset of F_q ([D][C]) in F
    const long long* zoff;  // [nemb] offset of the row's noise inside a draw
    const double* F;
    const double* slam;     // [nemb][Ltot] sqrt(lambda_+ / Ltot), natural frequency order
};

// conj(Y_a(w)) for the pair whose noise rows are z0, z1
__device__ __forceinline__ cplx smp_mixed(const SmpRows& R, const double* __restrict__ z0,
                                          const double* __restrict__ z1, int a, long long w,
                                          long long Ltot) {
    double re = 0.0, im = 0.0;
    for (int e = 0; e < R.nemb; ++e) {
        const int C = R.C[e];
        const double* f = R.F + R.foff[e] + (size_t)a * C;
        const double* p0 = z0 + R.zoff[e] + w;
        const double* p1 = z1 + R.zoff[e] + w;
        double sr = 0.0, si = 0.0;
        for (int c = 0; c < C; ++c) {
            sr = fma(f[c], p0[(size_t)c * Ltot], sr);
            si = fma(f[c], p1[(size_t)c * Ltot], si);
        }
        const double s = R.slam[(size_t)e * Ltot + w];
        re = fma(s, sr, re);
        im = fma(s, si, im);
    }
    return c_make(re, -im);
}

// grid (D, npairs), block RL_SMP_THREADS, LDS Ls * sizeof(cplx)
// (the output index runs fastest: the D workgroups that read one pair's noise are adjacent in
// launch order -- the same in the two kernels below.  Measured, that does not make them share a
// read: consecutive workgroups go to different XCDs, each with an L2 of its own)
static __global__ void __launch_bounds__(RL_SMP_THREADS)
k_smp_embed1(const double* __restrict__ Z, long long zlen, SmpRows R, int D, int m, FftPlan plan,
             const cplx* __restrict__ tw, const int* __restrict__ posof, double* __restrict__ U,
             int nsamp) {
    RL_SMEM(smem);
    cplx* tile = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int a = blockIdx.x, pair = blockIdx.y, Ls = plan.n;
    const double* z0 = Z + (size_t)(2 * pair) * zlen;
    const double* z1 = z0 + zlen;
    for (int w = tid; w < Ls; w += nthr) tile[w] = smp_mixed(R, z0, z1, a, w, Ls);
    __syncthreads();
    fft_tile_forward(tile, plan, 1, 1, tw, tid, nthr);
    double* u0 = U + ((size_t)(2 * pair) * D + a) * m;
    const bool second = 2 * pair + 1 < nsamp;
    double* u1 = u0 + (size_t)D * m;
    for (int x = tid; x < m; x += nthr) {
        const cplx v = tile[posof[x]];
        u0[x] = v.x;
        if (second) u1[x] = -v.y;
    }
}

// grid (D, ceil(N2 / cols), npairs), block RL_SMP_THREADS, LDS N1 * cols * sizeof(cplx)
//   twist: 1-D (the twiddle between the passes); tw1[k] = exp(-2 pi i k / N1), twlo[k] =
//   exp(-2 pi i k / (N1 N2)), k < N2:  n2 k1 = hi N2 + lo  ->  tw1[hi] * twlo[lo]
static __global__ void __launch_bounds__(RL_SMP_THREADS)
k_smp_cols(const double* __restrict__ Z, long long zlen, SmpRows R, int D, FftPlan plan1, int N2,
           int cols, const cplx* __restrict__ tw1, const cplx* __restrict__ twlo,
           const int* __restrict__ freq1, int twist, cplx* __restrict__ T) {
    RL_SMEM(smem);
    cplx* tile = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int a = blockIdx.x, c0 = blockIdx.y * cols, pair = blockIdx.z, N1 = plan1.n;
    const long long Ltot = (long long)N1 * N2;
    const double* z0 = Z + (size_t)(2 * pair) * zlen;
    const double* z1 = z0 + zlen;
    const int work = N1 * cols;
    for (int w = tid; w < work; w += nthr) {
        const int n1 = w / cols, c = w - n1 * cols, n2 = c0 + c;
        tile[w] = n2 < N2 ? smp_mixed(R, z0, z1, a, (long long)n1 * N2 + n2, Ltot) : c_make(0.0, 0.0);
    }
    __syncthreads();
    fft_tile_forward(tile, plan1, cols, cols, tw1, tid, nthr);
    cplx* t = T + ((size_t)pair * D + a) * (size_t)Ltot;
    for (int w = tid; w < work; w += nthr) {
        const int p1 = w / cols, c = w - p1 * cols, n2 = c0 + c;
        if (n2 >= N2) continue;
        cplx v = tile[w];
        if (twist) {
            const long long idx = (long long)n2 * freq1[p1];
            const int hi = (int)(idx / N2), lo = (int)(idx - (long long)hi * N2);
            v = c_mul(v, c_mul(tw1[hi], twlo[lo]));
        }
        t[(size_t)p1 * N2 + n2] = v;
    }
}

// grid (D, ceil(K1 / rows), npairs), block RL_SMP_THREADS, LDS N2 * ld * sizeof(cplx), ld = rows | 1
//   K1: the k1 that reach the grid (1-D: min(N1, m); 2-D: m1);  m2 == 0: 1-D, x = k1 + N1 k2 < m;
//   else x = k1 m2 + k2 with k2 < m2
static __global__ void __launch_bounds__(RL_SMP_THREADS)
k_smp_rows(const cplx* __restrict__ T, int D, int N1, FftPlan plan2, int rows, int ld, int K1,
           const cplx* __restrict__ tw2, const int* __restrict__ pos1, const int* __restrict__ freq2,
           int m, int m2, double* __restrict__ U, int nsamp) {
    RL_SMEM(smem);
    cplx* tile = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int a = blockIdx.x, k0 = blockIdx.y * rows, pair = blockIdx.z, N2 = plan2.n;
    const cplx* t = T + ((size_t)pair * D + a) * ((size_t)N1 * N2);
    const int work = rows * N2;
    for (int w = tid; w < work; w += nthr) {
        const int r = w / N2, n2 = w - r * N2, k1 = k0 + r;
        tile[(size_t)n2 * ld + r] = k1 < K1 ? t[(size_t)pos1[k1] * N2 + n2] : c_make(0.0, 0.0);
    }
    __syncthreads();
    fft_tile_forward(tile, plan2, rows, ld, tw2, tid, nthr);
    double* u0 = U + ((size_t)(2 * pair) * D + a) * m;
    const bool second = 2 * pair + 1 < nsamp;
    double* u1 = u0 + (size_t)D * m;
    for (int w = tid; w < work; w += nthr) {
        const int p2 = w / rows, r = w - p2 * rows, k1 = k0 + r, k2 = freq2[p2];
        if (k1 >= K1) continue;
        long long x;
        if (m2 == 0) {
            x = (long long)k1 + (long long)N1 * k2;
            if (x >= m) continue;
        } else {
            if (k2 >= m2) continue;
            x = (long long)k1 * m2 + k2;
        }
        const cplx v = tile[(size_t)p2 * ld + r];
        u0[x] = v.x;
        if (second) u1[x] = -v.y;
    }
}

// Zhat[s][a][j] = nu_j sum_e sum_c F_e[a][c] sum_i G_e[j][i] z[s][zoff_e + c r + i]: the mixed
// coefficients of the polynomial rows on the unnormalised basis k_lr_expand evaluates.
//   grid ceil(nsamp D r / 256), block 256
static __global__ void __launch_bounds__(RL_SMP_THREADS)
k_smp_poly_coef(const double* __restrict__ Z, long long zlen, int npoly, const int* __restrict__ C,
                const int* __restrict__ foff, const long long* __restrict__ zoff,
                const double* __restrict__ F, const double* __restrict__ G,
                const double* __restrict__ nu, int D, int r, int nsamp, double* __restrict__ Zhat) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)nsamp * D * r) return;
    const int j = (int)(e % r), a = (int)((e / r) % D), s = (int)(e / ((long long)r * D));
    const double* z = Z + (size_t)s * zlen;
    double acc = 0.0;
    for (int p = 0; p < npoly; ++p) {
        const int Cp = C[p];
        const double* f = F + foff[p] + (size_t)a * Cp;
        const double* g = G + ((size_t)p * r + j) * r;
        for (int c = 0; c < Cp; ++c) {
            const double* zc = z + zoff[p] + (size_t)c * r;
            double t = 0.0;
            for (int i = 0; i < r; ++i) t = fma(g[i], zc[i], t);
            acc = fma(f[c], t, acc);
        }
    }
    Zhat[e] = nu[j] * acc;
}

// --- noise ---------------------------------------------------------------------------------------
// splitmix64's finaliser: a bijection of 64-bit words with full avalanche
__host__ __device__ __forceinline__ unsigned long long smp_mix64(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// Element (s, j) of the stream `seed`: the Box-Muller pair of counter (s, j / 2), its cosine
// branch for even j and its sine branch for odd j.
__device__ __forceinline__ double smp_normal(unsigned long long seed, unsigned long long s,
                                             unsigned long long j) {
    const unsigned long long k0 = smp_mix64(seed + 0x9E3779B97F4A7C15ull);
    const unsigned long long k1 = smp_mix64(k0 ^ (s * 0xD1342543DE82EF95ull + 0x632BE59BD9B4E019ull));
    const unsigned long long k2 = smp_mix64(k1 + (j >> 1) * 0x9E3779B97F4A7C15ull);
    const unsigned long long r1 = smp_mix64(k2), r2 = smp_mix64(k2 ^ 0xD6E8FEB86659FD93ull);
    const double u1 = ((double)(r1 >> 11) + 1.0) * (1.0 / 9007199254740992.0);   // (0, 1]
    const double u2 = (double)(r2 >> 11) * (1.0 / 9007199254740992.0);           // [0, 1)
    const double rad = sqrt(-2.0 * log(u1));
    const double ang = 6.283185307179586476925286766559 * u2;
    return rad * ((j & 1ull) ? sin(ang) : cos(ang));
}

// grid (ceil(zlen / 256) capped, ndraws), block 256: grid-stride over j
static __global__ void __launch_bounds__(RL_SMP_THREADS)
k_smp_normal(unsigned long long seed, long long draw0, long long zlen, double* __restrict__ Z) {
    const unsigned long long s = (unsigned long long)(draw0 + blockIdx.y);
    double* z = Z + (size_t)blockIdx.y * zlen;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < zlen; j += step)
        z[j] = smp_normal(seed, s, (unsigned long long)j);
}

// grid (ceil(n / 256) capped, nsamp), block 256
static __global__ void __launch_bounds__(RL_SMP_THREADS)
k_smp_residual(const double* __restrict__ y, const double* WU, const double* E,
               const double* __restrict__ sq, double* R, long long n) {
    const size_t row = (size_t)blockIdx.y * n;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
        R[row + i] = y[i] - WU[row + i] - sq[i] * E[row + i];
}
