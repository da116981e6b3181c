// Leading-axis transforms of a three-level block-Toeplitz product (3-D grids, rl_gridop::lead).
//
// Grid m0 x m1 x m2, grid index (i0 m1 + i1) m2 + i2; M = m1 m2 inner points.  The circulant
// embedding of the LEADING axis has N0 points (power of two >= 2 m0, >= 4), H = N0 / 2 and
// F = H + 1 real-input frequencies.  Zero-padding x along axis 0 and taking the real-to-complex
// DFT along it turns K x into F independent 2-D BTTB products over (m1, m2) -- the children of
// the handle (rl_gridop.hip: lead_mvm) -- with the real top rows
//     T^_q[f] = t_q[0] + 2 sum_{j = 1 .. m0-1} t_q[j] cos(2 pi f j / N0)
// applied to the real and the imaginary slab of x^_f alike.
//
//   k_lead_fwd<N0>:  X [v][d][i0][i12]  ->  Xh [f][re|im][v][d][i12]
//   k_lead_inv<N0>:  Yh [f][re|im][v][d][i12]  ->  Y [v][d][j0][i12],  rows j0 < m0, scaled 1 / N0
//
// Every frequency owns 2 nvec D M doubles of Xh / Yh (f = 0 and f = H use the real half only),
// so a frequency's batch is the contiguous (2 nvec, D M) input of its child as it stands.
//
// One lane owns one column (v, d, i12): consecutive lanes take consecutive i12, so each load
// and store of a wave is one contiguous 512-byte run of a slab.  The lane holds its column in
// registers as H / 2 complex numbers z[k] = x[2k] + i x[2k+1] (only the m0 <= H values that are
// not padding are ever loaded), runs a length-H complex FFT on them and separates the two
// interleaved real transforms afterwards; the inverse undoes the separation, runs the
// inverse FFT and keeps the first half.  The padding is never materialised:
//   forward (decimation in frequency): the first stage's lower inputs are all zero, so it is a
//     copy and a twiddle;
//   inverse (decimation in time): only outputs n < H / 2 are wanted, so the last stage
//     computes its sums and not its differences.
// All indices into the register arrays are compile-time constants after unrolling (one
// instantiation per N0: 4 ... 128), the bit reversal costs nothing, and the twiddles
// exp(-2 pi i k / N0), k < H, come from a host-computed fp64 table through scalar loads
// (k_lead_inv at N0 = 128: through LDS).
// Registers: H complex = N0 doubles = 2 N0 VGPRs of the 512 a wave may take.  At N0 = 128 the forward
// transform fits (256 + temporaries, the overflow in AGPRs); the inverse, which also holds its
// input loads in flight, does not, and runs as two half transforms of H / 2 complex numbers with
// one half parked in LDS (k_lead_inv, N0 >= 128).  No instantiation uses scratch.
//
// Bytes per column: forward reads 8 m0, writes 8 N0; inverse reads 8 N0, writes 8 m0.
#pragma once
#include "rl_device.h"

#define RL_LEAD_MAX_M0 64
#define RL_LEAD_MAX_N0 128

// The large transforms (N0 >= 64) fill the register file with the column itself, and their
// twiddles, uniform values that come through scalar loads, are more than the scalar registers
// hold at once.  Left alone, the compiler moves the loads of a phase to the phase's start to
// hide their latency, and the values waiting there spill (measured: without the fence
// k_lead_fwd<64> spills 8 scalar registers and k_lead_fwd<128> 176).  A compiler-level memory
// fence after every few butterflies keeps loads next to their use; it emits no instruction.
// Whether it is still needed is a question for -Rpass-analysis=kernel-resource-usage after a
// compiler update (profiles/grid3d/README.md has the figures of the recorded build).
// k_lead_inv<128> does without: it keeps its twiddles in LDS (below).
#define RL_LEAD_FENCE(cond) do { if (cond) asm volatile("" ::: "memory"); } while (0)

__host__ __device__ constexpr int rl_lead_brev(int i, int bits) {
    int r = 0;
    for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}
__host__ __device__ constexpr int rl_lead_log2(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

// threads per workgroup: the large transforms hold one wave per SIMD, so narrow workgroups
// spread a launch over more compute units
__host__ __device__ constexpr int rl_lead_threads(int N0) { return N0 >= 64 ? 64 : 256; }

// tw[k] = exp(-2 pi i k / N0), k < H, as (re, im) pairs
template <int N0>
__global__ void __launch_bounds__(rl_lead_threads(N0))
k_lead_fwd(const double* __restrict__ X, int m0, long long M, long long ncol, rl_kconst tw,
           double* __restrict__ Xh) {
    constexpr int H = N0 / 2, LG = rl_lead_log2(H);
    const long long c = (long long)blockIdx.x * rl_lead_threads(N0) + threadIdx.x;
    if (c >= ncol) return;
    const long long vd = c / M, i12 = c - vd * M;
    const double* x = X + vd * (long long)m0 * M + i12;
    double re[H], im[H];
    // z[k] = x[2k] + i x[2k+1] for the rows that exist (2k < m0 <= H)
#pragma unroll
    for (int k = 0; k < H / 2; ++k) {
        re[k] = 2 * k < m0 ? x[(long long)(2 * k) * M] : 0.0;
        im[k] = 2 * k + 1 < m0 ? x[(long long)(2 * k + 1) * M] : 0.0;
    }
    // first stage: the lower inputs z[k + H/2] are padding
#pragma unroll
    for (int k = 0; k < H / 2; ++k) {
        const double wr = tw[4 * k], wi = tw[4 * k + 1];        // W_H^k = tw[2k]
        re[k + H / 2] = re[k] * wr - im[k] * wi;
        im[k + H / 2] = re[k] * wi + im[k] * wr;
        RL_LEAD_FENCE(N0 >= 64 && k % 8 == 7);
    }
    // remaining stages, blocks of len = H/2 ... 2
#pragma unroll
    for (int len = H / 2; len >= 2; len >>= 1) {
#pragma unroll
        for (int b = 0; b < H; b += len) {
#pragma unroll
            for (int k = 0; k < len / 2; ++k) {
                const int i = b + k, j = b + k + len / 2;
                const int t = k * (N0 / len);                   // W_len^k = tw[k N0 / len]
                const double ur = re[i], ui = im[i], vr = re[j], vi = im[j];
                re[i] = ur + vr;
                im[i] = ui + vi;
                const double dr = ur - vr, di = ui - vi;
                if (t == 0) {
                    re[j] = dr;
                    im[j] = di;
                } else {
                    const double wr = tw[2 * t], wi = tw[2 * t + 1];
                    re[j] = dr * wr - di * wi;
                    im[j] = dr * wi + di * wr;
                }
                RL_LEAD_FENCE(N0 >= 64 && (b / 2 + k) % 8 == 7);
            }
        }
    }
    // Z[f] sits at position brev(f).  With a = Z[f], b = conj Z[H-f], e = (a + b) / 2 and
    // g = w^f (a - b) / 2:   X^[f] = e - i g,   X^[H-f] = conj(e) - i conj(g)
    const long long DM = ncol;               // nvec * D * M: one real (or imaginary) slab
    double* out = Xh + c;
    {
        const double zr = re[0], zi = im[0];
        out[0] = zr + zi;                                         // f = 0 (real)
        out[(long long)H * 2 * DM] = zr - zi;                     // f = H (real)
    }
#pragma unroll
    for (int f = 1; f < H / 2; ++f) {
        const int p = rl_lead_brev(f, LG), q = rl_lead_brev(H - f, LG);
        const double ar = re[p], ai = im[p], br = re[q], bi = -im[q];
        const double er = 0.5 * (ar + br), ei = 0.5 * (ai + bi);
        const double dr = 0.5 * (ar - br), di = 0.5 * (ai - bi);
        const double wr = tw[2 * f], wi = tw[2 * f + 1];
        const double gr = wr * dr - wi * di, gi = wr * di + wi * dr;
        out[(long long)f * 2 * DM] = er + gi;
        out[(long long)f * 2 * DM + DM] = ei - gr;
        out[(long long)(H - f) * 2 * DM] = er - gi;
        out[(long long)(H - f) * 2 * DM + DM] = -ei - gr;
        RL_LEAD_FENCE(N0 >= 64 && f % 4 == 3);
    }
    if (H >= 2) {                                                 // f = H / 2: conj Z[H/2]
        const int p = rl_lead_brev(H / 2, LG);
        out[(long long)(H / 2) * 2 * DM] = re[p];
        out[(long long)(H / 2) * 2 * DM + DM] = -im[p];
    }
}

// One half of the inverse at N0 = 128.  The decimation-in-time stages below the last one never
// mix the even-frequency positions brev(k) < H/2 with the odd-frequency ones, so each half is a
// transform of H/2 complex numbers of its own: the separation of the frequencies k = PAR (mod 2)
// and the stages len = 2 ... H/2 on them, left in re / im [0, H/2) in natural order.
template <int N0, int PAR>
__device__ __forceinline__ void lead_inv_half(const double* in, long long DM, const double* tw,
                                              double (&re)[N0 / 4], double (&im)[N0 / 4]) {
    constexpr int H = N0 / 2, Q = H / 2, LG = rl_lead_log2(Q);
    static_assert(H >= 4, "the halves split by parity from H = 4 on");
    if (PAR == 0) {
        const double r0 = in[0], rH = in[(long long)H * 2 * DM];
        re[0] = r0 + rH;
        im[0] = r0 - rH;
        const int p = rl_lead_brev(H / 4, LG);                    // k = H / 2: 2 conj Y^[H/2]
        re[p] = 2.0 * in[(long long)(H / 2) * 2 * DM];
        im[p] = -2.0 * in[(long long)(H / 2) * 2 * DM + DM];
    }
#pragma unroll
    for (int k = 1; k < H / 2; ++k) {
        if ((k & 1) != PAR) continue;
        const double ar = in[(long long)k * 2 * DM], ai = in[(long long)k * 2 * DM + DM];
        const double br = in[(long long)(H - k) * 2 * DM], bi = -in[(long long)(H - k) * 2 * DM + DM];
        const double er = ar + br, ei = ai + bi, dr = ar - br, di = ai - bi;
        const double wr = tw[2 * k], wi = -tw[2 * k + 1];         // conj(w^k)
        const double gr = wr * dr - wi * di, gi = wr * di + wi * dr;
        const int p = rl_lead_brev(k >> 1, LG), q = rl_lead_brev((H - k) >> 1, LG);
        re[p] = er - gi;
        im[p] = ei + gr;
        re[q] = er + gi;
        im[q] = gr - ei;
    }
#pragma unroll
    for (int len = 2; len <= Q; len <<= 1) {
#pragma unroll
        for (int b = 0; b < Q; b += len) {
#pragma unroll
            for (int k = 0; k < len / 2; ++k) {
                const int i = b + k, j = b + k + len / 2;
                const int t = k * (N0 / len);
                double vr = re[j], vi = im[j];
                if (t != 0) {
                    const double wr = tw[2 * t], wi = -tw[2 * t + 1];
                    const double tr = vr * wr - vi * wi;
                    vi = vr * wi + vi * wr;
                    vr = tr;
                }
                const double ur = re[i], ui = im[i];
                re[i] = ur + vr;
                im[i] = ui + vi;
                re[j] = ur - vr;
                im[j] = ui - vi;
            }
        }
    }
}

// LDS of one k_lead_inv workgroup: none up to N0 = 64; at N0 = 128 the twiddle table (N0 doubles)
// and the odd half of every lane's column, H / 2 complex numbers, while the even half is
// transformed
__host__ __device__ constexpr int rl_lead_inv_lds(int N0) {
    return N0 >= 128 ? (N0 + (N0 / 2) * rl_lead_threads(N0)) * (int)sizeof(double) : 0;
}

template <int N0>
__global__ void __launch_bounds__(rl_lead_threads(N0))
k_lead_inv(const double* Yh, int m0, long long M, long long ncol, rl_kconst tw,
           double* __restrict__ Y) {
    constexpr int H = N0 / 2, LG = rl_lead_log2(H);
    const long long c = (long long)blockIdx.x * rl_lead_threads(N0) + threadIdx.x;
    const long long DM = ncol;
    if constexpr (N0 >= 128) {
        // The whole column is 2 N0 VGPRs, the arch half of the register file, and does not fit
        // beside its temporaries; nor does the twiddle table fit the scalar registers.  The last
        // stage is  out[k] = E[k] + conj(W_H^k) O[k], k < H/2,  of the even- and the
        // odd-frequency half transforms: the lane runs O, parks the twiddled result in LDS
        // ([k][lane]: conflict-free, and no lane reads another's, so no barrier), then runs E in
        // the same registers and adds.  The twiddles sit in LDS too: every lane reads the same
        // address, a broadcast.
        constexpr int Q = H / 2, T = rl_lead_threads(N0);
        RL_SMEM(smem);
        double* twl = reinterpret_cast<double*>(smem);
        for (int i = threadIdx.x; i < N0; i += T) twl[i] = tw[i];
        __syncthreads();
        if (c >= ncol) return;
        const double* in = Yh + c;
        double* park = twl + N0 + threadIdx.x;
        {
            double re[Q], im[Q];
            lead_inv_half<N0, 1>(in, DM, twl, re, im);
#pragma unroll
            for (int k = 0; k < Q; ++k) {
                double vr = re[k], vi = im[k];
                if (k != 0) {
                    const double wr = twl[4 * k], wi = -twl[4 * k + 1];   // conj(W_H^k)
                    const double tr = vr * wr - vi * wi;
                    vi = vr * wi + vi * wr;
                    vr = tr;
                }
                park[(2 * k) * T] = vr;
                park[(2 * k + 1) * T] = vi;
            }
        }
        {
            double re[Q], im[Q];
            lead_inv_half<N0, 0>(in, DM, twl, re, im);
            const long long vd = c / M, i12 = c - vd * M;
            double* y = Y + vd * (long long)m0 * M + i12;
            const double scale = 1.0 / (double)N0;
#pragma unroll
            for (int k = 0; k < Q; ++k) {
                if (2 * k < m0) y[(long long)(2 * k) * M] = (re[k] + park[(2 * k) * T]) * scale;
                if (2 * k + 1 < m0) y[(long long)(2 * k + 1) * M] = (im[k] + park[(2 * k + 1) * T]) * scale;
            }
        }
        return;
    }
    if (c >= ncol) return;
    const double* in = Yh + c;
    double re[H], im[H];
    // With A = Y^[k], B = conj Y^[H-k], E = A + B and G = conj(w^k) (A - B):
    //   Z[k] = E + i G,   Z[H-k] = conj(E) + i conj(G),   stored at brev(k), brev(H-k):
    // twice the transform of z = even rows + i odd rows (the factor goes into the scale)
    {
        const double r0 = in[0], rH = in[(long long)H * 2 * DM];
        re[0] = r0 + rH;
        im[0] = r0 - rH;
    }
#pragma unroll
    for (int k = 1; k < H / 2; ++k) {
        const double ar = in[(long long)k * 2 * DM], ai = in[(long long)k * 2 * DM + DM];
        const double br = in[(long long)(H - k) * 2 * DM], bi = -in[(long long)(H - k) * 2 * DM + DM];
        const double er = ar + br, ei = ai + bi, dr = ar - br, di = ai - bi;
        const double wr = tw[2 * k], wi = -tw[2 * k + 1];         // conj(w^k)
        const double gr = wr * dr - wi * di, gi = wr * di + wi * dr;
        const int p = rl_lead_brev(k, LG), q = rl_lead_brev(H - k, LG);
        re[p] = er - gi;
        im[p] = ei + gr;
        re[q] = er + gi;
        im[q] = gr - ei;
        RL_LEAD_FENCE(N0 >= 64 && k % 4 == 3);
    }
    if (H >= 2) {                                                 // k = H / 2: 2 conj Y^[H/2]
        const int p = rl_lead_brev(H / 2, LG);
        re[p] = 2.0 * in[(long long)(H / 2) * 2 * DM];
        im[p] = -2.0 * in[(long long)(H / 2) * 2 * DM + DM];
    }
    // decimation in time with exp(+): blocks of len = 2 ... H/2 in full
#pragma unroll
    for (int len = 2; len <= H / 2; len <<= 1) {
#pragma unroll
        for (int b = 0; b < H; b += len) {
#pragma unroll
            for (int k = 0; k < len / 2; ++k) {
                const int i = b + k, j = b + k + len / 2;
                const int t = k * (N0 / len);
                double vr = re[j], vi = im[j];
                if (t != 0) {
                    const double wr = tw[2 * t], wi = -tw[2 * t + 1];
                    const double tr = vr * wr - vi * wi;
                    vi = vr * wi + vi * wr;
                    vr = tr;
                }
                const double ur = re[i], ui = im[i];
                re[i] = ur + vr;
                im[i] = ui + vi;
                re[j] = ur - vr;
                im[j] = ui - vi;
                RL_LEAD_FENCE(N0 >= 64 && (b / 2 + k) % 8 == 7);
            }
        }
    }
    // last stage (len = H): sums only, outputs n < H / 2; rows 2n and 2n + 1 of the column
    const long long vd = c / M, i12 = c - vd * M;
    double* y = Y + vd * (long long)m0 * M + i12;
    const double scale = 1.0 / (double)N0;
#pragma unroll
    for (int k = 0; k < H / 2; ++k) {
        const int j = k + H / 2;
        double vr = re[j], vi = im[j];
        if (k != 0) {
            const double wr = tw[4 * k], wi = -tw[4 * k + 1];     // conj(W_H^k)
            const double tr = vr * wr - vi * wi;
            vi = vr * wi + vi * wr;
            vr = tr;
        }
        if (2 * k < m0) y[(long long)(2 * k) * M] = (re[k] + vr) * scale;
        if (2 * k + 1 < m0) y[(long long)(2 * k + 1) * M] = (im[k] + vi) * scale;
        RL_LEAD_FENCE(N0 >= 64 && k % 8 == 7);
    }
}
