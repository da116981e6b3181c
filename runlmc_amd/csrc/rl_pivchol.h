// Pivoted-Cholesky preconditioner of a SKI operator (rl_ski_set_pivchol):
//     P = L L^T + E,   L (n x k) the rank-k pivoted Cholesky factor of  K = sum_t W_t K_t W_t^T,
// applied through the Woodbury identity.  It needs the operator's product and its diagonal and
// nothing else, so it exists for every operator rl_ski_factor otherwise declines (2-D and 3-D
// grids, several grids, D > 16, rows outside the polynomial subspace).
//
// L is stored [kp][n], kp = k rounded up to 16, column j of the factor a contiguous stream (the
// rows k .. kp - 1 and every column after an early stop are zero).  Every sum below runs in a
// fixed order -- rows in chunks, chunks by index, no atomics -- so that two builds of one
// operator give the same bits.
//
// Build (per parameter / noise update):
//   k_pc_diag     d_i = (W_t K_t W_t^T)_ii from the row's own interpolation entries
//   k_pc_argmax   per-block arg-max of d (ties: the lowest index)
//   k_pc_pick     finishes the arg-max, records (p_j, d_pj), writes the one-hot vector e_pj
//   k_pc_step     column j from the product K e_pj, the update of d, the next arg-max partials
//   k_pc_project  with X = L: the Gram matrix L^T E^-1 L (k_pc_reduce sums its chunks)
// Apply (every PCG iteration), z = a (.) r + b (.) L M L^T (s (.) r):
//   k_pc_project  part[chunk][v][j] = sum_{i in chunk} L[j][i] s_i X[v][i]      (matrix cores)
//   k_pc_map      c'[j][v] = sum_j' M[j][j'] sum_chunks part[chunk][v][j']
//   k_pc_expand   out[v][i] = a_i X[v][i] + b_i sum_j L[j][i] c'[j][v]           (matrix cores)
// (emulator: no matrix instruction -- scalar bodies under RL_EMU, same indexing and masks)
#pragma once
#include "rl_device.h"
#include "rl_rowpoly.h"

#define RL_PC_MAXRANK 256
#define RL_PC_NBLK 256          // blocks of k_pc_step / k_pc_argmax at most (partials per step)
#define RL_PC_CHUNKS 512        // row chunks of k_pc_project at most (about)

// one W K_UU W^T term as k_pc_diag reads it: the interpolant in CSR (internal row order), the
// top rows [Q][m] on the e0 x e1 x e2 grid (a 1-D grid is 1 x 1 x m, a 2-D one 1 x m1 x m2) and
// the couplings [Q][D][D]
struct PcTerm {
    const int* indptr;
    const int* indices;
    const double* w;
    const double* tops;
    const double* B;
    int m, e1, e2, Q;
};

// d_i (+)= sum_{a, b} w_a w_b sum_q B_q[d_a][d_b] t_q[lag(a, b)] over the pairs of the row's own
// entries (4, 16 or 64), each unordered pair once: the exact diagonal of W K_UU W^T, which the
// kernel's value at lag 0 is not (the residual diagonal has to stay non-negative).
static __global__ void __launch_bounds__(256)
k_pc_diag(PcTerm t, int n, int D, int accumulate, double* __restrict__ d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k0 = t.indptr[i], k1 = t.indptr[i + 1];
    const int e12 = t.e1 * t.e2;
    double acc = 0.0;
    for (int a = k0; a < k1; ++a) {
        const int ca = t.indices[a], da = ca / t.m, ga = ca - da * t.m;
        const int a0 = ga / e12, ra = ga - a0 * e12, a1 = ra / t.e2, a2 = ra - a1 * t.e2;
        const double wa = t.w[a];
        for (int b = a; b < k1; ++b) {
            const int cb = t.indices[b], db = cb / t.m, gb = cb - db * t.m;
            const int b0 = gb / e12, rb = gb - b0 * e12, b1 = rb / t.e2, b2 = rb - b1 * t.e2;
            const int l0 = a0 > b0 ? a0 - b0 : b0 - a0, l1 = a1 > b1 ? a1 - b1 : b1 - a1;
            const int l2 = a2 > b2 ? a2 - b2 : b2 - a2;
            const size_t lag = ((size_t)l0 * t.e1 + l1) * t.e2 + l2;
            double kv = 0.0;
            for (int q = 0; q < t.Q; ++q)
                kv = fma(t.B[((size_t)q * D + da) * D + db], t.tops[(size_t)q * t.m + lag], kv);
            acc = fma((a == b ? 1.0 : 2.0) * wa * t.w[b], kv, acc);
        }
    }
    d[i] = accumulate ? d[i] + acc : acc;
}

// arg-max of (v, i) over the workgroup's 256 threads, ties to the lowest index; valid in every
// thread.  scr: 256 doubles, then 256 ints.
__device__ __forceinline__ void pc_block_argmax(double& v, int& i, double* sv, int* si, int tid) {
    sv[tid] = v;
    si[tid] = i;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) {
            const double ov = sv[tid + h];
            const int oi = si[tid + h];
            if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) {
                sv[tid] = ov;
                si[tid] = oi;
            }
        }
        __syncthreads();
    }
    v = sv[0];
    i = si[0];
    __syncthreads();
}

// rows of block b of nb: a contiguous range (whole multiples of 256 rows but the last)
__device__ __forceinline__ void pc_block_rows(int n, int b, int nb, int* lo, int* hi) {
    const int per = ((n + nb - 1) / nb + 255) / 256 * 256;
    const long a = (long)b * per;
    *lo = a < n ? (int)a : n;
    *hi = a + per < n ? (int)(a + per) : n;
}

static __global__ void __launch_bounds__(256)
k_pc_argmax(const double* __restrict__ d, int n, double* __restrict__ pv, int* __restrict__ pi) {
    RL_SMEM(smem);
    double* sv = reinterpret_cast<double*>(smem);
    int* si = reinterpret_cast<int*>(sv + 256);
    const int tid = threadIdx.x;
    int lo, hi;
    pc_block_rows(n, blockIdx.x, gridDim.x, &lo, &hi);
    double bv = -1.0;
    int bi = 0x7fffffff;
    for (int i = lo + tid; i < hi; i += 256) {
        const double v = d[i];
        if (v > bv) { bv = v; bi = i; }          // (ascending i: the first of equal values stays)
    }
    pc_block_argmax(bv, bi, sv, si, tid);
    if (tid == 0) { pv[blockIdx.x] = bv; pi[blockIdx.x] = bi; }
}

// one workgroup: pivot of step j = arg-max of the nb partials; records it, moves the one-hot
// vector from the previous pivot to this one, and at step 0 keeps max_i d_i^(0)
static __global__ void __launch_bounds__(256)
k_pc_pick(const double* __restrict__ pv, const int* __restrict__ pi, int nb, int j, int n,
          int* __restrict__ piv, double* __restrict__ pivval, double* __restrict__ d0max,
          double* __restrict__ e) {
    RL_SMEM(smem);
    double* sv = reinterpret_cast<double*>(smem);
    int* si = reinterpret_cast<int*>(sv + 256);
    const int tid = threadIdx.x;
    double bv = -1.0;
    int bi = 0x7fffffff;
    for (int b = tid; b < nb; b += 256) {
        const double v = pv[b];
        const int i = pi[b];
        if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
    }
    pc_block_argmax(bv, bi, sv, si, tid);
    if (tid == 0) {
        if (bi < 0 || bi >= n) { bi = 0; bv = 0.0; }       // (no finite value anywhere: a zero column follows)
        if (j > 0) e[piv[j - 1]] = 0.0;
        e[bi] = 1.0;
        piv[j] = bi;
        pivval[j] = bv;
        if (j == 0) *d0max = bv;
    }
}

// Step j with pivot p = piv[j], d_p = pivval[j], row = K e_p (noise-free):
//   l_i = (row_i - sum_{t < j} L[t][i] L[t][p]) / sqrt(d_p),  l_p = sqrt(d_p),  l = 0 exactly on
//   earlier pivots;  d_i <- max(d_i - l_i^2, 0),  d_p = 0;  arg-max partials of the new d.
// d_p <= rel_tol * max d^(0): a zero column, d unchanged (every later step finds the same).
// LDS: L[0..j)[p] (256 doubles) + the arg-max scratch.
static __global__ void __launch_bounds__(256)
k_pc_step(int j, const double* __restrict__ row, double* __restrict__ L, int n,
          const int* __restrict__ piv, const double* __restrict__ pivval,
          const double* __restrict__ d0max, double rel_tol, double* __restrict__ d,
          int* __restrict__ mark, double* __restrict__ pv, int* __restrict__ pi) {
    RL_SMEM(smem);
    double* Lp = reinterpret_cast<double*>(smem);
    double* sv = Lp + RL_PC_MAXRANK;
    int* si = reinterpret_cast<int*>(sv + 256);
    const int tid = threadIdx.x;
    const int p = piv[j];
    const double dp = pivval[j];
    const bool stop = !(dp > rel_tol * *d0max) || !(dp > 0.0);
    if (tid < j) Lp[tid] = L[(size_t)tid * n + p];
    __syncthreads();
    const double sq = sqrt(dp);
    double* Lj = L + (size_t)j * n;
    int lo, hi;
    pc_block_rows(n, blockIdx.x, gridDim.x, &lo, &hi);
    double bv = -1.0;
    int bi = 0x7fffffff;
    for (int i = lo + tid; i < hi; i += 256) {
        double dn = d[i];
        if (stop) {
            Lj[i] = 0.0;
        } else {
            const bool old = mark[i] != 0;
            double acc = row[i];
            for (int t = 0; t < j; ++t) acc = fma(-L[(size_t)t * n + i], Lp[t], acc);
            double l = acc / sq;
            if (i == p) l = sq;
            else if (old) l = 0.0;
            Lj[i] = l;
            dn = (i == p || old) ? 0.0 : fmax(dn - l * l, 0.0);
            d[i] = dn;
            if (i == p) mark[i] = 1;
        }
        if (dn > bv) { bv = dn; bi = i; }
    }
    pc_block_argmax(bv, bi, sv, si, tid);
    if (tid == 0) { pv[blockIdx.x] = bv; pi[blockIdx.x] = bi; }
}

// out[e] = sum_c part[c][e] (+ 0 in a fixed order): the Gram matrix from k_pc_project's chunks
static __global__ void __launch_bounds__(256)
k_pc_reduce(const double* __restrict__ part, int nchunk, size_t total, double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += part[(size_t)c * total + e];
    out[e] = s;
}

// rows to the caller's order (rl_ski_pivchol_factor / _info): out[v][perm[i]] = in[v][i]
static __global__ void __launch_bounds__(256)
k_pc_unpermute(const double* __restrict__ in, const int* __restrict__ perm, int n,
               double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t v = blockIdx.y;
    out[v * n + (perm ? perm[i] : i)] = in[v * n + i];
}

// ---------------------------------------------------------------------------
// k_pc_project<NVT, JT>: part[chunk][v][j] = sum_{i in chunk} L[j][i] s_i X[v][i]
//   grid (ceil(nvp / (16 NVT)), nchunk)   block 256: wave w owns the column tiles jt = w, w + 4,
//   ... (JT of them: kp <= 64 JT) and 16 NVT vectors, and walks the chunk's rows four at a time:
//   D(vectors x columns) += A(vectors x rows) B(rows x columns) on v_mfma_f64_16x16x4_f64,
//     A[v][k] = s X[v0 + v][i + k]  in lane v + 16 k,   B[k][j] = L[j0 + j][i + k]  in lane j + 16 k,
//     D: register r of lane l = vector (l >> 4) + 4 r, column l & 15   (layouts: rl_rowpoly.h).
//   The accumulators stay in registers over the chunk (4 JT NVT doubles a lane); no LDS, no
//   barrier; every wave writes the entries it owns.  s may be NULL (= 1).
// ---------------------------------------------------------------------------
template <int NVT, int JT>
__global__ void __launch_bounds__(256)
k_pc_project(const double* __restrict__ X, const double* __restrict__ sc, const double* __restrict__ L,
             int n, int nvec, int nvp, int kp, int rows_per_chunk, double* __restrict__ part) {
    const int tid = threadIdx.x;
    const int chunk = blockIdx.y;
    const long ib = (long)chunk * rows_per_chunk;
    const int i_begin = ib < n ? (int)ib : n;
    const int i_end = ib + rows_per_chunk < n ? (int)(ib + rows_per_chunk) : n;
    const int v0 = blockIdx.x * 16 * NVT;
    double* out = part + (size_t)chunk * nvp * kp;
#if !defined(RL_EMU)
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int njt = kp / 16;
    rp_double4 C[JT][NVT];
#pragma unroll
    for (int jj = 0; jj < JT; ++jj)
#pragma unroll
        for (int t = 0; t < NVT; ++t) C[jj][t] = rp_double4{0.0, 0.0, 0.0, 0.0};
    bool von[NVT], jon[JT];
    const double* xp[NVT];
    const double* lp[JT];
#pragma unroll
    for (int t = 0; t < NVT; ++t) {
        const int v = v0 + 16 * t + li;
        von[t] = v < nvec;
        xp[t] = X + (size_t)(von[t] ? v : 0) * n;
    }
#pragma unroll
    for (int jj = 0; jj < JT; ++jj) {
        const int jt = jj * 4 + wave;
        jon[jj] = jt < njt;
        lp[jj] = L + (size_t)((jon[jj] ? jt : 0) * 16 + li) * n;
    }
    for (int i = i_begin; i < i_end; i += 4) {
        const int ii = i + lk;
        const bool ok = ii < i_end;
        const int ic = ok ? ii : i_begin;
        const double s = sc ? sc[ic] : 1.0;
        double a[NVT], b[JT];
#pragma unroll
        for (int t = 0; t < NVT; ++t) a[t] = ok && von[t] ? s * xp[t][ic] : 0.0;
#pragma unroll
        for (int jj = 0; jj < JT; ++jj) b[jj] = ok && jon[jj] ? lp[jj][ic] : 0.0;
#pragma unroll
        for (int jj = 0; jj < JT; ++jj)
#pragma unroll
            for (int t = 0; t < NVT; ++t)
                C[jj][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[jj], C[jj][t], 0, 0, 0);
    }
#pragma unroll
    for (int jj = 0; jj < JT; ++jj) {
        if (!jon[jj]) continue;
        const int j = (jj * 4 + wave) * 16 + li;
#pragma unroll
        for (int t = 0; t < NVT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int v = v0 + 16 * t + lk + 4 * r;
                if (v < nvp) out[(size_t)v * kp + j] = C[jj][t][r];
            }
    }
#else
    for (int e = tid; e < 16 * NVT * kp; e += 256) {
        const int v = v0 + e / kp, j = e % kp;
        if (v >= nvp) continue;
        double acc = 0.0;
        if (v < nvec && j / 64 < JT)
            for (int i = i_begin; i < i_end; ++i)
                acc = fma((sc ? sc[i] : 1.0) * X[(size_t)v * n + i], L[(size_t)j * n + i], acc);
        out[(size_t)v * kp + j] = acc;
    }
#endif
}

// c'[j][v] = sum_j' Mt[j'][j] c[v][j'],  c[v][j'] = sum_chunks part[chunk][v][j']  (chunks in order).
// Mt is the map TRANSPOSED, [kp][kp] (thread j reads Mt[j'][j]: coalesced).  One workgroup per
// vector, v < nvp (vectors past nvec carry zeros); LDS: kp doubles.
static __global__ void __launch_bounds__(256)
k_pc_map(const double* __restrict__ part, int nchunk, int nvp, int kp, const double* __restrict__ Mt,
         double* __restrict__ cT) {
    RL_SMEM(smem);
    double* c = reinterpret_cast<double*>(smem);
    const int v = blockIdx.x, j = threadIdx.x;
    if (j < kp) {
        double s = 0.0;
        for (int ch = 0; ch < nchunk; ++ch) s += part[((size_t)ch * nvp + v) * kp + j];
        c[j] = s;
    }
    __syncthreads();
    if (j < kp) {
        double s = 0.0;
        for (int q = 0; q < kp; ++q) s = fma(Mt[(size_t)q * kp + j], c[q], s);
        cT[(size_t)j * nvp + v] = s;
    }
}

// ---------------------------------------------------------------------------
// k_pc_expand<NVT>: out[v][i] = a_i X[v][i] + b_i sum_{j < kp} L[j][i] cT[j][v]    (b NULL: 1)
//   grid (ceil(n / 128), ceil(nvp / (16 NVT)))   block 256: wave w owns 32 rows and 16 NVT vectors
//   and walks the columns four at a time (the scheme of k_hz_expand_mm, rl_direct.h):
//     A[v][k] = cT[j + k][v0 + v]  in lane v + 16 k,   B[k][i] = L[j + k][i0 + i]  in lane i + 16 k
//     (16 consecutive rows of one column per quarter wave),
//     D: register r of lane l = vector (l >> 4) + 4 r, row l & 15: loads of X and stores of out
//     are 16 consecutive rows of one vector per quarter wave.
// ---------------------------------------------------------------------------
template <int NVT>
__global__ void __launch_bounds__(256)
k_pc_expand(const double* __restrict__ cT, const double* __restrict__ L, int n, int nvec, int nvp, int kp,
            const double* __restrict__ X, const double* __restrict__ da, const double* __restrict__ db,
            double* __restrict__ out) {
    const int tid = threadIdx.x;
    const int v0 = blockIdx.y * 16 * NVT;
    constexpr int RT = 2, WR = 16 * RT;
#if !defined(RL_EMU)
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int r0 = blockIdx.x * (4 * WR) + wave * WR;
    if (r0 >= n) return;
    rp_double4 C[RT][NVT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NVT; ++t) C[rt][t] = rp_double4{0.0, 0.0, 0.0, 0.0};
    bool ron[RT], von[NVT];
    const double* lr[RT];
    const double* cp[NVT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int i = r0 + 16 * rt + li;
        ron[rt] = i < n;
        lr[rt] = L + (size_t)lk * n + (ron[rt] ? i : n - 1);
    }
#pragma unroll
    for (int t = 0; t < NVT; ++t) {
        const int v = v0 + 16 * t + li;
        von[t] = v < nvp;
        cp[t] = cT + (size_t)lk * nvp + (von[t] ? v : 0);
    }
    for (int j = 0; j < kp; j += 4) {
        double a[NVT], b[RT];
#pragma unroll
        for (int t = 0; t < NVT; ++t) a[t] = von[t] ? cp[t][(size_t)j * nvp] : 0.0;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) b[rt] = ron[rt] ? lr[rt][(size_t)j * n] : 0.0;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int t = 0; t < NVT; ++t)
                C[rt][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[rt], C[rt][t], 0, 0, 0);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int i = r0 + 16 * rt + li;
        if (i >= n) continue;
        const double ai = da[i], bi = db ? db[i] : 1.0;
#pragma unroll
        for (int t = 0; t < NVT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int v = v0 + 16 * t + lk + 4 * r;
                if (v < nvec) out[(size_t)v * n + i] = fma(bi, C[rt][t][r], ai * X[(size_t)v * n + i]);
            }
    }
#else
    if (tid >= 4 * WR) return;
    const int i = blockIdx.x * (4 * WR) + tid;
    if (i >= n) return;
    const double ai = da[i], bi = db ? db[i] : 1.0;
    for (int q = 0; q < 16 * NVT; ++q) {
        const int v = v0 + q;
        if (v >= nvec) continue;
        double acc = 0.0;
        for (int j = 0; j < kp; ++j) acc = fma(L[(size_t)j * n + i], cT[(size_t)j * nvp + v], acc);
        out[(size_t)v * n + i] = fma(bi, acc, ai * X[(size_t)v * n + i]);
    }
#endif
}
