// Exact (dense) LMC likelihood on the device: the handle rl_exact of include/runlmc_hip.h.
// Kernels: rl_exact.h.  Every step is fp64; the n x n matrix lives in ONE device buffer that is
// K, then its Cholesky factor L, then (for gradients) the lower triangle of K^-1.
#include "rl_host.h"
#include "rl_exact.h"
#include "rl_rownoise.h"

enum { EX_EMPTY = 0, EX_SET, EX_ASSEMBLED, EX_FACTORED, EX_INVERTED };

struct rl_exact {
    int device = 0, n = 0, P = 0, D = 0, Q = 0, nslot = 0, ncu = 1;
    int maxf = 1;                   // most factors of any kernel (3 with any cosine leaf): 1 runs the kernels' <1> bodies
    int sep = 0;                    // rl_exact_set_separable: cols holds the leaves' column lists, the kernels run <., true>
    int state = EX_EMPTY;
    DevBuf<double> A;               // n x n
    DevBuf<double> X;               // n x P
    DevBuf<int> out_of;             // n: output of each row
    DevBuf<int> bounds;             // D + 1 row offsets of the outputs
    DevBuf<int> kinds;              // descriptors (rl_exact.h: ex_desc; capacity EX_MAX_SLOT kernels)
    DevBuf<double> prm;
    DevBuf<int> cols;               // [Q][EX_MAX_COLS], or [Q][EX_MAX_FACT][EX_MAX_COLS] when sep
    DevBuf<int> dslot;
    DevBuf<double> Bm;              // Q x D x D
    DevBuf<double> noise;           // D
    DevBuf<double> row_noise;       // n: known per-observation variances on top (rl_exact_set_row_noise) ...
    bool has_row_noise = false;     // ... kept across rl_exact_set* calls until cleared
    DevBuf<double> logd;            // n
    DevBuf<double> scal;            // 1
    DevBuf<int> flag;               // first bad pivot
    DevBuf<double> ws;              // split-k partial sums / gradient partials
    DevBuf<int> tiles;              // gradient workgroups (r0, c0, a, b)
    DevBuf<int> pair_start;
    int ntiles = 0;
    DevBuf<double> gout;            // gradient sums
    DevBuf<double> xt;              // test rows of rl_exact_cross_dev (kept between calls)
    DevBuf<int> ot;
    std::vector<int> lens, hbounds;
};

static int ex_ws(rl_exact* h, size_t doubles) {
    if (h->ws.reserve(doubles) != RL_OK) {
        (void)hipGetLastError();
        return fail(RL_ENOMEM, "rl_exact: no device memory for a workspace of " +
                                   std::to_string(doubles * 8 >> 20) + " MB");
    }
    return RL_OK;
}

// a kernel templated on the factor count, at the handle's: plain sets run <1>, separable sets
// the per-leaf distances
#define EX_LAUNCH_FACT(h, kern, grid, block, smem, stream, ...)                         \
    do {                                                                                \
        if ((h)->sep)                                                                   \
            RL_LAUNCH((kern<EX_MAX_FACT, true>), grid, block, smem, stream, __VA_ARGS__); \
        else if ((h)->maxf == 1)                                                        \
            RL_LAUNCH(kern<1>, grid, block, smem, stream, __VA_ARGS__);                 \
        else                                                                            \
            RL_LAUNCH(kern<EX_MAX_FACT>, grid, block, smem, stream, __VA_ARGS__);       \
    } while (0)

static inline int ex_tiles(long long v) { return (int)((v + EX_T - 1) / EX_T); }
static const size_t kGemmLds = 2 * EX_T * EX_LDK * sizeof(double);
static const size_t kTileLds = 2 * EX_T * EX_LDT * sizeof(double);

// C (+)= s A B^T through k_ex_gemm (see rl_exact.h).  via_partials: the result goes through the
// split-k workspace and k_ex_reduce (needed when C overlaps A or B); otherwise K is split only
// when the tiles alone leave the chip idle.
static int ex_gemm(rl_exact* h, hipStream_t st, double* C, long long ldc, const double* A,
                   long long sai, long long sak, const double* B, long long sbj, long long sbk,
                   int M, int N, int K, double s, int beta, int lower_tiles, int a_lower,
                   bool via_partials) {
    if (M <= 0 || N <= 0) return RL_OK;
    const int tm = ex_tiles(M), tn = ex_tiles(N);
    const long long ntile = lower_tiles ? (long long)tm * (tm + 1) / 2 : (long long)tm * tn;
    const long long target = 2LL * h->ncu;
    int nsplit = 1;
    if (!lower_tiles && ntile < target) {
        const long long want = (target + ntile - 1) / ntile;
        const int kmax = ex_tiles(K);
        nsplit = (int)(want < kmax ? want : kmax);
    }
    if (nsplit < 1) nsplit = 1;
    int kchunk = (K + nsplit - 1) / nsplit;
    kchunk = (kchunk + EX_KC - 1) / EX_KC * EX_KC;
    if (kchunk < EX_KC) kchunk = EX_KC;
    nsplit = (K + kchunk - 1) / kchunk;
    if (nsplit < 1) nsplit = 1;
    if (nsplit == 1 && !via_partials) {
        RL_LAUNCH(k_ex_gemm, dim3(tn, tm, 1), dim3(256), kGemmLds, st, C, ldc, A, sai, sak, B, sbj,
                  sbk, M, N, K, kchunk, a_lower, s, beta, lower_tiles, (double*)nullptr);
        RL_HIP(hipGetLastError());
        return RL_OK;
    }
    RL_TRY(ex_ws(h, (size_t)nsplit * M * N));
    RL_LAUNCH(k_ex_gemm, dim3(tn, tm, nsplit), dim3(256), kGemmLds, st, C, ldc, A, sai, sak, B, sbj,
              sbk, M, N, K, kchunk, a_lower, s, beta, 0, h->ws);
    RL_HIP(hipGetLastError());
    const long long MN = (long long)M * N;
    RL_LAUNCH(k_ex_reduce, dim3((unsigned)((MN + 255) / 256)), dim3(256), 0, st, C, ldc,
              (const double*)h->ws, M, N, nsplit, s, beta);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

// rows R[v][.] (v < nrhs, leading dimension n) := L^-1 R[v]  (then L^-T when both)
static int ex_trsv(rl_exact* h, hipStream_t st, double* R, int nrhs, bool forward, bool backward) {
    const int n = h->n, nb = ex_tiles(n);
    const dim3 g(ex_tiles(nrhs));
    if (forward) {
        for (int k = 0; k < nb; ++k) {
            const int k0 = k * EX_T, nk = std::min(EX_T, n - k0), rest = n - k0 - nk;
            RL_LAUNCH(k_ex_trsv_diag, g, dim3(64), kTileLds, st, (const double*)h->A, (long long)n,
                      k0, nk, R, (long long)n, nrhs, 0);
            RL_HIP(hipGetLastError());
            RL_TRY(ex_gemm(h, st, R + k0 + nk, n, R + k0, n, 1, h->A + (long long)(k0 + nk) * n + k0,
                           n, 1, nrhs, rest, nk, -1.0, 1, 0, 0, false));
        }
    }
    if (backward) {
        for (int k = nb - 1; k >= 0; --k) {
            const int k0 = k * EX_T, nk = std::min(EX_T, n - k0);
            RL_LAUNCH(k_ex_trsv_diag, g, dim3(64), kTileLds, st, (const double*)h->A, (long long)n,
                      k0, nk, R, (long long)n, nrhs, 1);
            RL_HIP(hipGetLastError());
            RL_TRY(ex_gemm(h, st, R, n, R + k0, n, 1, h->A + (long long)k0 * n, 1, n, nrhs, k0, nk,
                           -1.0, 1, 0, 0, false));
        }
    }
    return RL_OK;
}

// K(Xa, X) (+ noise on the diagonal i + diag_off == j) of nrows rows into `out` (nrows x n)
static int ex_cross(rl_exact* h, hipStream_t st, double* out, const double* Xa, const int* oa,
                    int nrows, const double* noise, int diag_off) {
    if (nrows <= 0) return RL_OK;
    EX_LAUNCH_FACT(h, k_ex_assemble, dim3(ex_tiles(h->n), ex_tiles(nrows)), dim3(256), 0, st, out,
              (long long)h->n, nrows, h->n, Xa, oa, (const double*)h->X, (const int*)h->out_of,
              h->P, h->Q, (const int*)h->kinds, (const double*)h->prm, (const int*)h->cols,
              (const double*)h->Bm, h->D, noise, diag_off, 0);
    RL_HIP(hipGetLastError());
    // (the per-observation variances go where the noise goes: not on the noise-free cross-covariances)
    if (noise && h->has_row_noise) {
        RL_LAUNCH(k_rn_add_diag, dim3((nrows + 255) / 256), dim3(256), 0, st, out, (long long)h->n, nrows,
                  h->n, (const double*)h->row_noise, diag_off);
        RL_HIP(hipGetLastError());
    }
    return RL_OK;
}

extern "C" int rl_exact_create(int device, int n, int P, rl_exact** out) {
    if (!out) return fail(RL_EINVAL, "rl_exact_create: out is NULL");
    *out = nullptr;
    if (n < 1 || P < 1) return fail(RL_EINVAL, "rl_exact_create: n and P must be >= 1");
    if ((long long)n * P > (1LL << 31)) return fail(RL_ELIMIT, "rl_exact_create: n * P too large");
    RL_HIP(hipSetDevice(device));
    rl_exact* h = new rl_exact;
    HandleGuard<rl_exact, rl_exact_destroy> guard(h);
    h->device = device;
    h->n = n;
    h->P = P;
    hipDeviceProp_t prop;
    RL_HIP(hipGetDeviceProperties(&prop, device));
    h->ncu = std::max(1, prop.multiProcessorCount);
    RL_TRY(h->X.reserve((size_t)n * P));
    RL_TRY(h->out_of.reserve((size_t)n));
    RL_TRY(h->bounds.reserve(EX_MAX_D + 1));
    RL_TRY(h->kinds.reserve(EX_MAX_SLOT));
    RL_TRY(h->prm.reserve(2 * EX_PRM2));
    RL_TRY(h->cols.reserve(EX_MAX_SLOT * EX_LEAF_COLS));
    RL_TRY(h->dslot.reserve(EX_MAX_SLOT));
    RL_TRY(h->Bm.reserve((size_t)EX_MAX_SLOT * EX_MAX_D * EX_MAX_D));
    RL_TRY(h->noise.reserve(EX_MAX_D));
    RL_TRY(h->logd.reserve((size_t)n));
    RL_TRY(h->scal.reserve(1));
    RL_TRY(h->flag.reserve(1));
    RL_TRY(h->gout.reserve((size_t)EX_MAX_SLOT * EX_MAX_D * EX_MAX_D + EX_MAX_D));
    (void)hipFuncSetAttribute((const void*)k_ex_grad_tiles<1>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (EX_MAX_SLOT + 1) * 256 * (int)sizeof(double));
    (void)hipFuncSetAttribute((const void*)k_ex_grad_tiles<EX_MAX_FACT>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (EX_MAX_SLOT + 1) * 256 * (int)sizeof(double));
    (void)hipFuncSetAttribute((const void*)k_ex_grad_tiles<EX_MAX_FACT, true>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (EX_MAX_SLOT + 1) * 256 * (int)sizeof(double));
    *out = guard.release();
    return RL_OK;
}

extern "C" int rl_exact_destroy(rl_exact* h) {
    if (!h) return RL_OK;
    (void)hipSetDevice(h->device);
    delete h;
    return RL_OK;
}

// What rl_exact_set and rl_exact_set_factors share.  `describe(q, desc, p0, p1)` validates kernel q
// of the caller's arguments and writes its device descriptor (rl_exact.h: ex_desc) and its two
// parameter groups, [g_0, T_0, c, -] and [g_1, T_1, g_2, T_2]; it runs per kernel where
// rl_exact_set has always checked the kind, so every error keeps its precedence.  Nothing indexed
// by q is written past EX_MAX_SLOT kernels: a larger Q only counts, and is refused with the count.
// `what` names the entry point in messages.  sep: active_cols holds a column list per LEAF,
// [Q][EX_MAX_FACT][EX_MAX_COLS]; those of a kernel's factors are checked as a kernel's list is
// (the lists past its last factor are not read) and go to the device in that layout.
template <class Describe>
static int ex_set(rl_exact* h, const char* what, const double* X, const int* lens, int D, int Q,
                  Describe describe, const int* active_cols, const double* B, const double* noise,
                  bool sep = false) {
    const std::string fn = what;
    const int stride = sep ? EX_LEAF_COLS : EX_MAX_COLS;
    if (D > EX_MAX_D) return fail(RL_ELIMIT, fn + ": D > 64 outputs");
    long long total = 0;
    for (int d = 0; d < D; ++d) {
        if (lens[d] < 0) return fail(RL_EINVAL, fn + ": negative output length");
        total += lens[d];
    }
    if (total != h->n)
        return fail(RL_EINVAL, fn + ": lens sum to " + std::to_string(total) + ", handle has n = " +
                                   std::to_string(h->n));
    long long nslot = Q;
    int maxf = 1;
    std::vector<int> descs(EX_MAX_SLOT, 0), dslot(EX_MAX_SLOT, 0), cols((size_t)EX_MAX_SLOT * EX_LEAF_COLS, -1);
    std::vector<double> prm(2 * EX_PRM2, 0.0);
    for (int q = 0; q < Q; ++q) {
        int desc = 0;
        double p0[4] = {0.0, 0.0, 0.0, 0.0}, p1[4] = {0.0, 0.0, 0.0, 0.0};
        RL_TRY(describe(q, &desc, p0, p1));
        const int slot = (int)std::min<long long>(nslot, EX_MAX_SLOT);
        nslot += ex_desc_nder(desc);
        maxf = std::max(maxf, ex_desc_nf(desc));
        // (a cosine leaf has no formula in ex_eval: even alone it runs the factor-list bodies)
        if (ex_desc_leaf(desc, 0) == EX_COSINE) maxf = EX_MAX_FACT;
        const bool keep = q < EX_MAX_SLOT;
        if (keep) {
            descs[q] = desc;
            dslot[q] = slot;
            for (int p = 0; p < 4; ++p) {
                prm[4 * q + p] = p0[p];
                prm[EX_PRM2 + 4 * q + p] = p1[p];
            }
        }
        for (int f = 0; f < (sep ? ex_desc_nf(desc) : 1); ++f) {
            const int* list = active_cols + (size_t)q * stride + f * EX_MAX_COLS;
            int nc = 0;
            for (int c = 0; c < EX_MAX_COLS; ++c) {
                const int col = list[c];
                if (col >= h->P) return fail(RL_EINVAL, fn + ": active column beyond P");
                if (col < 0) break;
                ++nc;
            }
            if (nc == 0)
                return fail(RL_EINVAL, fn + (sep ? ": leaf " + std::to_string(f) + " of kernel " + std::to_string(q) +
                                                       " without active columns"
                                                 : std::string(": a kernel without active columns")));
            if (keep)
                for (int c = 0; c < EX_MAX_COLS; ++c)
                    cols[(size_t)q * stride + f * EX_MAX_COLS + c] = c < nc ? list[c] : -1;
        }
    }
    if (nslot > EX_MAX_SLOT)
        return fail(RL_ELIMIT, fn + ": Q + sum of kernel parameters = " + std::to_string(nslot) +
                                   " > 32");
    RL_HIP(hipSetDevice(h->device));
    std::vector<int> out_of(h->n), bounds(D + 1, 0);
    for (int d = 0, i = 0; d < D; ++d) {
        for (int k = 0; k < lens[d]; ++k) out_of[i++] = d;
        bounds[d + 1] = bounds[d] + lens[d];
    }
    RL_HIP(hipMemcpy(h->X, X, (size_t)h->n * h->P * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(h->out_of, out_of.data(), (size_t)h->n * sizeof(int), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(h->bounds, bounds.data(), (D + 1) * sizeof(int), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(h->kinds, descs.data(), Q * sizeof(int), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(h->prm, prm.data(), 2 * EX_PRM2 * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(h->cols, cols.data(), (size_t)Q * stride * sizeof(int), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(h->dslot, dslot.data(), Q * sizeof(int), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(h->Bm, B, (size_t)Q * D * D * sizeof(double), hipMemcpyHostToDevice));
    RL_HIP(hipMemcpy(h->noise, noise, D * sizeof(double), hipMemcpyHostToDevice));
    // gradient workgroups: tiles of every output block (a, b), a >= b, of the lower triangle
    if (h->lens != std::vector<int>(lens, lens + D) || h->D != D) {
        std::vector<int> tl, ps(1, 0);
        for (int a = 0; a < D; ++a)
            for (int b = 0; b <= a; ++b) {
                for (int r0 = bounds[a]; r0 < bounds[a + 1]; r0 += EX_T)
                    for (int c0 = bounds[b]; c0 < bounds[b + 1]; c0 += EX_T) {
                        if (a == b && c0 - bounds[b] > r0 - bounds[a]) continue;
                        tl.insert(tl.end(), {r0, c0, a, b});
                    }
                ps.push_back((int)tl.size() / 4);
            }
        h->tiles.reset();
        h->pair_start.reset();
        RL_TRY(h->tiles.upload(tl));
        RL_TRY(h->pair_start.upload(ps));
        h->ntiles = (int)tl.size() / 4;
        h->lens.assign(lens, lens + D);
    }
    h->D = D;
    h->Q = Q;
    h->nslot = (int)nslot;
    h->maxf = sep ? EX_MAX_FACT : maxf;
    h->sep = sep ? 1 : 0;
    h->hbounds = bounds;
    h->state = EX_SET;
    return RL_OK;
}

extern "C" int rl_exact_set(rl_exact* h, const double* X, const int* lens, int D, int Q,
                            const int* kinds, const double* params, const int* active_cols,
                            const double* B, const double* noise) {
    if (!h || !X || !lens || !kinds || !params || !active_cols || !B || !noise)
        return fail(RL_EINVAL, "rl_exact_set: NULL argument");
    if (D < 1 || Q < 1) return fail(RL_EINVAL, "rl_exact_set: D and Q must be >= 1");
    auto describe = [&](int q, int* desc, double* p0, double*) -> int {
        const int base = kinds[q] & ~EX_SCALED;
        if (base != EX_RBF && base != EX_MATERN32 && base != EX_STDPERIODIC && base != EX_MATERN52)
            return fail(RL_EINVAL, "rl_exact_set: unknown kernel kind " + std::to_string(kinds[q]));
        *desc = kinds[q];
        for (int p = 0; p < 4; ++p) p0[p] = params[q * 4 + p];
        return RL_OK;
    };
    return ex_set(h, "rl_exact_set", X, lens, D, Q, describe, active_cols, B, noise);
}

extern "C" int rl_exact_set_factors(rl_exact* h, const double* X, const int* lens, int D, int Q,
                                    const int* nfact, const int* leaf_kinds,
                                    const double* leaf_params, const int* scaled,
                                    const double* scales, const int* active_cols, const double* B,
                                    const double* noise) {
    if (!h || !X || !lens || !nfact || !leaf_kinds || !leaf_params || !scaled || !scales ||
        !active_cols || !B || !noise)
        return fail(RL_EINVAL, "rl_exact_set_factors: NULL argument");
    if (D < 1 || Q < 1) return fail(RL_EINVAL, "rl_exact_set_factors: D and Q must be >= 1");
    auto describe = [&](int q, int* desc, double* p0, double* p1) -> int {
        const int nf = nfact[q];
        if (nf < 1 || nf > EX_MAX_FACT)
            return fail(RL_EINVAL, "rl_exact_set_factors: kernel " + std::to_string(q) + " has " +
                                       std::to_string(nf) + " factors (1 .. 3)");
        const int* leaf = leaf_kinds + (size_t)q * EX_MAX_FACT;
        for (int f = 0; f < nf; ++f) {
            if (leaf[f] != EX_RBF && leaf[f] != EX_MATERN32 && leaf[f] != EX_STDPERIODIC &&
                leaf[f] != EX_MATERN52 && leaf[f] != EX_COSINE)
                return fail(RL_EINVAL, "rl_exact_set_factors: unknown kernel kind " + std::to_string(leaf[f]));
            double* pf = f == 0 ? p0 : p1 + 2 * (f - 1);
            pf[0] = leaf_params[((size_t)q * EX_MAX_FACT + f) * 2];
            pf[1] = leaf_params[((size_t)q * EX_MAX_FACT + f) * 2 + 1];
        }
        p0[2] = scaled[q] ? scales[q] : 0.0;
        *desc = ex_desc(leaf, nf, scaled[q] != 0);
        return RL_OK;
    };
    return ex_set(h, "rl_exact_set_factors", X, lens, D, Q, describe, active_cols, B, noise);
}

extern "C" int rl_exact_set_separable(rl_exact* h, const double* X, const int* lens, int D, int Q,
                                      const int* nfact, const int* leaf_kinds,
                                      const double* leaf_params, const int* leaf_cols,
                                      const int* scaled, const double* scales, const double* B,
                                      const double* noise) {
    if (!h || !X || !lens || !nfact || !leaf_kinds || !leaf_params || !leaf_cols || !scaled ||
        !scales || !B || !noise)
        return fail(RL_EINVAL, "rl_exact_set_separable: NULL argument");
    if (D < 1 || Q < 1) return fail(RL_EINVAL, "rl_exact_set_separable: D and Q must be >= 1");
    auto describe = [&](int q, int* desc, double* p0, double* p1) -> int {
        const int nf = nfact[q];
        if (nf < 1 || nf > EX_MAX_FACT)
            return fail(RL_EINVAL, "rl_exact_set_separable: kernel " + std::to_string(q) + " has " +
                                       std::to_string(nf) + " factors (1 .. 3)");
        const int* leaf = leaf_kinds + (size_t)q * EX_MAX_FACT;
        for (int f = 0; f < nf; ++f) {
            if (leaf[f] != EX_RBF && leaf[f] != EX_MATERN32 && leaf[f] != EX_STDPERIODIC &&
                leaf[f] != EX_MATERN52 && leaf[f] != EX_COSINE)
                return fail(RL_EINVAL, "rl_exact_set_separable: unknown kernel kind " + std::to_string(leaf[f]));
            double* pf = f == 0 ? p0 : p1 + 2 * (f - 1);
            pf[0] = leaf_params[((size_t)q * EX_MAX_FACT + f) * 2];
            pf[1] = leaf_params[((size_t)q * EX_MAX_FACT + f) * 2 + 1];
        }
        p0[2] = scaled[q] ? scales[q] : 0.0;
        *desc = ex_desc(leaf, nf, scaled[q] != 0);
        return RL_OK;
    };
    return ex_set(h, "rl_exact_set_separable", X, lens, D, Q, describe, leaf_cols, B, noise, true);
}

extern "C" int rl_exact_assemble(rl_exact* h) {
    if (!h) return fail(RL_EINVAL, "rl_exact_assemble: NULL handle");
    if (h->state < EX_SET) return fail(RL_EINVAL, "rl_exact_assemble: no parameters (rl_exact_set)");
    RL_HIP(hipSetDevice(h->device));
    const int n = h->n;
    if (!h->A) {
        const size_t bytes = (size_t)n * n * sizeof(double);
        size_t fr = 0, tot = 0;
        RL_HIP(hipMemGetInfo(&fr, &tot));
        if (bytes + ((size_t)64 << 20) > fr)
            return fail(RL_ENOMEM, "rl_exact: the " + std::to_string(n) + " x " + std::to_string(n) +
                                       " matrix needs " + std::to_string(bytes >> 20) + " MB, " +
                                       std::to_string(fr >> 20) + " MB free");
        if (h->A.reserve((size_t)n * n) != RL_OK) {
            (void)hipGetLastError();
            return fail(RL_ENOMEM, "rl_exact: hipMalloc of the n x n matrix failed");
        }
    }
    const int nb = ex_tiles(n);
    EX_LAUNCH_FACT(h, k_ex_assemble, dim3(nb, nb), dim3(256), 0, (hipStream_t)0, h->A, (long long)n, n, n,
              (const double*)h->X, (const int*)h->out_of, (const double*)h->X,
              (const int*)h->out_of, h->P, h->Q, (const int*)h->kinds, (const double*)h->prm,
              (const int*)h->cols, (const double*)h->Bm, h->D, (const double*)h->noise, 0, 1);
    RL_HIP(hipGetLastError());
    if (h->has_row_noise) {
        RL_LAUNCH(k_rn_add_diag, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)0, h->A.get(), (long long)n,
                  n, n, (const double*)h->row_noise, 0);
        RL_HIP(hipGetLastError());
    }
    RL_HIP(hipStreamSynchronize(0));
    h->state = EX_ASSEMBLED;
    return RL_OK;
}

// Known per-observation variances (host [n], the rows' order of rl_exact_set; NULL clears them):
// added to the diagonal wherever the per-output noise is -- rl_exact_assemble, rl_exact_dense_host.
// A matrix assembled or factored before the call is stale: the handle returns to its set state.
extern "C" int rl_exact_set_row_noise(rl_exact* h, const double* extra) {
    if (!h) return fail(RL_EINVAL, "rl_exact_set_row_noise: NULL handle");
    if (extra) {
        for (int i = 0; i < h->n; ++i)
            if (!(extra[i] >= 0.0) || !std::isfinite(extra[i]))
                return fail(RL_EINVAL, "rl_exact_set_row_noise: extra[" + std::to_string(i) +
                                           "] is negative or not finite");
        RL_HIP(hipSetDevice(h->device));
        RL_TRY(h->row_noise.reserve((size_t)h->n));
        RL_HIP(hipMemcpy(h->row_noise, extra, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice));
    }
    h->has_row_noise = extra != nullptr;
    if (h->state > EX_SET) h->state = EX_SET;
    return RL_OK;
}

extern "C" int rl_exact_factor(rl_exact* h, double* logdet, int* bad_col) {
    if (!h) return fail(RL_EINVAL, "rl_exact_factor: NULL handle");
    if (bad_col) *bad_col = -1;
    if (h->state != EX_ASSEMBLED) RL_TRY(rl_exact_assemble(h));
    RL_HIP(hipSetDevice(h->device));
    const int n = h->n, nb = ex_tiles(n);
    const hipStream_t st = 0;
    RL_HIP(hipMemsetAsync(h->flag, 0x7f, sizeof(int), st));
    for (int k = 0; k < nb; ++k) {
        const int k0 = k * EX_T, nk = std::min(EX_T, n - k0), r0 = k0 + nk, rest = n - r0;
        RL_LAUNCH(k_ex_potrf_diag, dim3(1), dim3(256), EX_T * EX_LDT * sizeof(double), st, h->A,
                  (long long)n, k0, nk, h->logd, h->flag);
        RL_HIP(hipGetLastError());
        if (rest == 0) break;
        RL_LAUNCH(k_ex_trsm_panel, dim3(ex_tiles(rest)), dim3(64), kTileLds, st, h->A, (long long)n,
                  k0, nk, r0, rest);
        RL_HIP(hipGetLastError());
        double* L21 = h->A + (long long)r0 * n + k0;
        RL_TRY(ex_gemm(h, st, h->A + (long long)r0 * n + r0, n, L21, n, 1, L21, n, 1, rest, rest, nk,
                       -1.0, 1, 1, 0, false));
    }
    RL_LAUNCH(k_ex_sum2, dim3(1), dim3(256), 256 * sizeof(double), st, (const double*)h->logd, n,
              h->scal);
    RL_HIP(hipGetLastError());
    int flag = 0;
    double ld = 0.0;
    RL_HIP(hipMemcpy(&flag, h->flag, sizeof(int), hipMemcpyDeviceToHost));
    RL_HIP(hipMemcpy(&ld, h->scal, sizeof(double), hipMemcpyDeviceToHost));
    if (flag >= 0 && flag < n) {
        // the handle keeps its parameters: set new ones (or the same) and factor again
        h->state = EX_SET;
        if (bad_col) *bad_col = flag;
        return fail(RL_ENOTPD, "rl_exact_factor: the matrix is not positive definite: pivot of column " +
                                   std::to_string(flag) + " is not a positive finite number");
    }
    if (logdet) *logdet = ld;
    h->state = EX_FACTORED;
    return RL_OK;
}

extern "C" int rl_exact_solve(rl_exact* h, const double* B, double* X, int nrhs, void* stream) {
    if (!h || !B || !X) return fail(RL_EINVAL, "rl_exact_solve: NULL argument");
    if (nrhs < 0) return fail(RL_EINVAL, "rl_exact_solve: nrhs < 0");
    if (h->state != EX_FACTORED)
        return fail(RL_EINVAL, "rl_exact_solve: the handle holds no Cholesky factor (rl_exact_factor)");
    if (nrhs == 0) return RL_OK;
    RL_HIP(hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)stream;
    if (X != B)
        RL_HIP(hipMemcpyAsync(X, B, (size_t)nrhs * h->n * sizeof(double), hipMemcpyDeviceToDevice, st));
    return ex_trsv(h, st, X, nrhs, true, true);
}

// test rows on the device: X (nt x P) and their outputs
static int ex_upload_test(rl_exact* h, const double* Xt, const int* tlens, DevBuf<double>* dX,
                          DevBuf<int>* dO, int* nt) {
    long long total = 0;
    for (int d = 0; d < h->D; ++d) {
        if (tlens[d] < 0) return fail(RL_EINVAL, "rl_exact: negative test length");
        total += tlens[d];
    }
    if (total > (1LL << 30)) return fail(RL_ELIMIT, "rl_exact: too many test points");
    *nt = (int)total;
    std::vector<int> o((size_t)total);
    for (int d = 0, i = 0; d < h->D; ++d)
        for (int k = 0; k < tlens[d]; ++k) o[i++] = d;
    RL_TRY(dX->reserve(std::max<size_t>(1, (size_t)total * h->P)));
    RL_TRY(dO->reserve(std::max<size_t>(1, (size_t)total)));
    if (total) {
        RL_HIP(hipMemcpy(*dX, Xt, (size_t)total * h->P * sizeof(double), hipMemcpyHostToDevice));
        RL_HIP(hipMemcpy(*dO, o.data(), (size_t)total * sizeof(int), hipMemcpyHostToDevice));
    }
    return RL_OK;
}

// rows of the cross-covariance per chunk: at most 256 MB of them on the device at once
static int ex_chunk_rows(const rl_exact* h) {
    const long long r = ((long long)256 << 20) / (8LL * h->n);
    return (int)std::max(1LL, std::min(r, (long long)1 << 20));
}

static int ex_cross_rows(rl_exact* h, const double* Xt, const int* tlens, const double* noise,
                         double* out_host, double* var_out) {
    if (h->state < EX_SET) return fail(RL_EINVAL, "rl_exact: no parameters (rl_exact_set)");
    RL_HIP(hipSetDevice(h->device));
    DevBuf<double> tX, tV;          // temporaries of this call
    DevBuf<int> tO;
    int nt = 0;
    if (Xt) {
        RL_TRY(ex_upload_test(h, Xt, tlens, &tX, &tO, &nt));
    } else {
        nt = h->n;
    }
    if (nt == 0) return RL_OK;
    const int rows = std::min(nt, ex_chunk_rows(h));
    if (tV.reserve((size_t)rows * h->n) != RL_OK) {
        (void)hipGetLastError();
        return fail(RL_ENOMEM, "rl_exact: no device memory for the cross-covariance");
    }
    double* V = tV;
    double* norms = nullptr;
    if (var_out) RL_TRY(ex_ws(h, (size_t)rows));
    for (int r0 = 0; r0 < nt; r0 += rows) {
        const int nr = std::min(rows, nt - r0);
        const double* xa = Xt ? tX + (long long)r0 * h->P : h->X + (long long)r0 * h->P;
        const int* oa = Xt ? tO + r0 : h->out_of + r0;
        RL_TRY(ex_cross(h, 0, V, xa, oa, nr, noise, r0));
        if (var_out) {
            RL_TRY(ex_trsv(h, 0, V, nr, true, false));
            norms = h->ws;      // (ex_trsv's updates have K <= 64: one chunk, no partials)
            RL_LAUNCH(k_ex_rownorm2, dim3(nr), dim3(256), 256 * sizeof(double), (hipStream_t)0,
                      (const double*)V, (long long)h->n, norms);
            RL_HIP(hipGetLastError());
            RL_HIP(hipMemcpy(var_out + r0, norms, (size_t)nr * sizeof(double), hipMemcpyDeviceToHost));
        } else {
            RL_HIP(hipMemcpy(out_host + (long long)r0 * h->n, V, (size_t)nr * h->n * sizeof(double),
                             hipMemcpyDeviceToHost));
        }
    }
    return RL_OK;
}

extern "C" int rl_exact_cross_host(rl_exact* h, const double* Xtest, const int* test_lens,
                                   double* out) {
    if (!h || !Xtest || !test_lens || !out) return fail(RL_EINVAL, "rl_exact_cross_host: NULL argument");
    return ex_cross_rows(h, Xtest, test_lens, nullptr, out, nullptr);
}

extern "C" int rl_exact_dense_host(rl_exact* h, double* out) {
    if (!h || !out) return fail(RL_EINVAL, "rl_exact_dense_host: NULL argument");
    return ex_cross_rows(h, nullptr, nullptr, h->noise, out, nullptr);
}

extern "C" int rl_exact_explained_variance(rl_exact* h, const double* Xtest, const int* test_lens,
                                           double* out) {
    if (!h || !Xtest || !test_lens || !out)
        return fail(RL_EINVAL, "rl_exact_explained_variance: NULL argument");
    if (h->state != EX_FACTORED)
        return fail(RL_EINVAL, "rl_exact_explained_variance: the handle holds no Cholesky factor");
    return ex_cross_rows(h, Xtest, test_lens, nullptr, nullptr, out);
}

// LDS of k_ex_cross_rows: the staged test rows may take kCrossRowLds bytes, the staged training
// columns kCrossColLds more (beyond that a thread reads its column from global memory).
static const size_t kCrossRowLds = 32 << 10, kCrossColLds = 16 << 10;

extern "C" int rl_exact_cross_dev(rl_exact* h, const double* Xtest, const int* test_lens, int row0,
                                  int nrows, double* out, void* stream) {
    if (!h || !Xtest || !test_lens || !out) return fail(RL_EINVAL, "rl_exact_cross_dev: NULL argument");
    if (h->state < EX_SET) return fail(RL_EINVAL, "rl_exact_cross_dev: no parameters (rl_exact_set)");
    long long nt = 0;
    for (int d = 0; d < h->D; ++d) {
        if (test_lens[d] < 0) return fail(RL_EINVAL, "rl_exact_cross_dev: negative test length");
        nt += test_lens[d];
    }
    if (nt > (1LL << 30)) return fail(RL_ELIMIT, "rl_exact_cross_dev: too many test points");
    if (row0 < 0 || nrows < 0 || (long long)row0 + nrows > nt)
        return fail(RL_EINVAL, "rl_exact_cross_dev: rows " + std::to_string(row0) + " .. " +
                                   std::to_string((long long)row0 + nrows) + " of " +
                                   std::to_string(nt) + " test points");
    if (nrows == 0) return RL_OK;
    const int P = h->P, Q = h->Q, D = h->D;
    const size_t row_bytes = ((size_t)P + (size_t)Q * D) * sizeof(double);
    if (row_bytes > kCrossRowLds)
        return fail(RL_ELIMIT, "rl_exact_cross_dev: one test row (P + Q D = " +
                                   std::to_string(row_bytes / 8) + " values) exceeds the kernel's LDS");
    RL_HIP(hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)stream;
    // outputs of the window's rows, from the lengths
    std::vector<int> o((size_t)nrows);
    {
        long long begin = 0;
        for (int d = 0; d < D; ++d) {
            const long long end = begin + test_lens[d];
            const long long a = std::max<long long>(begin, row0), b = std::min<long long>(end, (long long)row0 + nrows);
            for (long long i = a; i < b; ++i) o[(size_t)(i - row0)] = d;
            begin = end;
        }
    }
    RL_TRY(h->xt.reserve((size_t)nrows * P));
    RL_TRY(h->ot.reserve((size_t)nrows));
    // the host rows are consumed before the call returns; the kernel stays queued
    RL_HIP(hipMemcpyAsync(h->xt, Xtest + (long long)row0 * P, (size_t)nrows * P * sizeof(double),
                          hipMemcpyHostToDevice, st));
    RL_HIP(hipMemcpyAsync(h->ot, o.data(), (size_t)nrows * sizeof(int), hipMemcpyHostToDevice, st));
    RL_HIP(hipStreamSynchronize(st));
    const int ldx = P | 1;
    const int stage_cols = (size_t)EX_CR_COLS * ldx * sizeof(double) <= kCrossColLds ? 1 : 0;
    const int rg = (int)std::min<size_t>({(size_t)nrows, (size_t)EX_T, kCrossRowLds / row_bytes});
    const size_t lds = (size_t)rg * row_bytes + (stage_cols ? (size_t)EX_CR_COLS * ldx * sizeof(double) : 0);
    const long long gx = ((long long)h->n + EX_CR_COLS - 1) / EX_CR_COLS;
    const int gy = (nrows + rg - 1) / rg;
    if (gy > 65535) return fail(RL_ELIMIT, "rl_exact_cross_dev: too many row groups in one call");
    EX_LAUNCH_FACT(h, k_ex_cross_rows, dim3((unsigned)gx, (unsigned)gy), dim3(EX_CR_COLS), lds, st, out,
              (long long)h->n, nrows, h->n, rg, (const double*)h->xt, (const int*)h->ot,
              (const double*)h->X, (const int*)h->out_of, P, Q, (const int*)h->kinds,
              (const double*)h->prm, (const int*)h->cols, (const double*)h->Bm, D, stage_cols, ldx);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

extern "C" int rl_row_dots(const double* B, const double* X, int nvec, long long n, double* dots,
                           double* sqnorms, double* ws, void* stream) {
    if (!B || !X || !dots || !sqnorms || !ws) return fail(RL_EINVAL, "rl_row_dots: NULL argument");
    if (nvec < 0 || n < 1) return fail(RL_EINVAL, "rl_row_dots: bad sizes");
    if (nvec > 65535) return fail(RL_ELIMIT, "rl_row_dots: more than 65535 rows in one call");
    if (nvec == 0) return RL_OK;
    const hipStream_t st = (hipStream_t)stream;
    RL_LAUNCH(k_ex_rowdot_part, dim3(EX_RD_CHUNKS, nvec), dim3(256), 512 * sizeof(double), st, B, X,
              n, ws);
    RL_HIP(hipGetLastError());
    RL_LAUNCH(k_ex_rowdot_sum, dim3((nvec + 63) / 64), dim3(64), 0, st, (const double*)ws, nvec,
              dots, sqnorms);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

extern "C" int rl_exact_invert(rl_exact* h) {
    if (!h) return fail(RL_EINVAL, "rl_exact_invert: NULL handle");
    if (h->state == EX_INVERTED) return RL_OK;
    if (h->state != EX_FACTORED)
        return fail(RL_EINVAL, "rl_exact_invert: the handle holds no Cholesky factor (rl_exact_factor)");
    RL_HIP(hipSetDevice(h->device));
    const int n = h->n, nb = ex_tiles(n);
    const long long ld = n;
    double* A = h->A;
    const hipStream_t st = 0;
    // L^-1 in place, last block column first (LAPACK dtrtri, lower):  W_jj = L_jj^-1,
    // W21 = -(W22 L21) W_jj  (W22 already inverted; tmp = n x 64 beside the matrix)
    DevBuf<double> panel;
    if (panel.reserve((size_t)n * EX_T) != RL_OK) {
        (void)hipGetLastError();
        return fail(RL_ENOMEM, "rl_exact_invert: no device memory for an n x 64 panel");
    }
    double* tmp = panel;
    for (int j = nb - 1; j >= 0; --j) {
        const int j0 = j * EX_T, nj = std::min(EX_T, n - j0), r0 = j0 + nj, rest = n - r0;
        RL_LAUNCH(k_ex_trtri_diag, dim3(1), dim3(64), kTileLds, st, A, ld, j0, nj);
        RL_HIP(hipGetLastError());
        if (rest == 0) continue;
        RL_TRY(ex_gemm(h, st, tmp, EX_T, A + (long long)r0 * n + r0, n, 1, A + (long long)r0 * n + j0, 1, n,
                       rest, nj, rest, 1.0, 0, 0, 1, false));
        RL_TRY(ex_gemm(h, st, A + (long long)r0 * n + j0, n, tmp, EX_T, 1, A + (long long)j0 * n + j0, 1, n,
                       rest, nj, nj, -1.0, 0, 0, 0, false));
    }
    // K^-1 = W^T W, lower, in place by block rows (LAPACK dlauum):
    //   row block i  <-  sum_{t >= i0} W[t][i-block]^T W[t][0 .. i0 + ni)   (through the partials:
    //   the result overwrites rows the sum reads)
    for (int i = 0; i < nb; ++i) {
        const int i0 = i * EX_T, ni = std::min(EX_T, n - i0);
        RL_TRY(ex_gemm(h, st, A + (long long)i0 * n, n, A + (long long)i0 * n + i0, 1, n,
                       A + (long long)i0 * n, 1, n, ni, i0 + ni, n - i0, 1.0, 0, 0, 0, true));
    }
    RL_HIP(hipStreamSynchronize(st));
    h->state = EX_INVERTED;
    return RL_OK;
}

extern "C" int rl_exact_grad_sums(rl_exact* h, const double* alpha, double* out) {
    if (!h || !alpha || !out) return fail(RL_EINVAL, "rl_exact_grad_sums: NULL argument");
    if (h->state != EX_INVERTED) RL_TRY(rl_exact_invert(h));
    RL_HIP(hipSetDevice(h->device));
    const int D = h->D, ns = h->nslot;
    const hipStream_t st = 0;
    const size_t nout = (size_t)ns * D * D + D;
    RL_HIP(hipMemsetAsync(h->gout, 0, nout * sizeof(double), st));
    if (h->ntiles > 0) {
        RL_TRY(ex_ws(h, (size_t)h->ntiles * (ns + 1)));
        EX_LAUNCH_FACT(h, k_ex_grad_tiles, dim3(h->ntiles), dim3(256), (size_t)(ns + 1) * 256 * sizeof(double),
                  st, (const double*)h->A, (long long)h->n, alpha, (const int*)h->tiles,
                  (const int*)h->bounds, (const double*)h->X, h->P, h->Q, (const int*)h->kinds,
                  (const double*)h->prm, (const int*)h->cols, (const int*)h->dslot, ns, h->ws);
        RL_HIP(hipGetLastError());
    }
    RL_LAUNCH(k_ex_grad_reduce, dim3(D * (D + 1) / 2), dim3(64), 0, st, (const double*)h->ws,
              (const int*)h->pair_start, D, ns, h->gout);
    RL_HIP(hipGetLastError());
    RL_HIP(hipMemcpy(out, h->gout, nout * sizeof(double), hipMemcpyDeviceToHost));
    return RL_OK;
}
