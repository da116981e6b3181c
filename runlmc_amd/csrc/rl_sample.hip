// Function draws: the handle rl_sampler of include/runlmc_hip.h (prior draws of the grid
// operator's Gaussian by circulant embedding of the extended kernel rows and through the
// polynomial form), the counter-based normal generator and the residual of Matheron's rule.
// Kernels: rl_sample.h.
#include "rl_host.h"
#include "rl_sample.h"

#include <complex>

typedef std::complex<double> cd;

static const int kSmpTile = 4096;            // complex values of one LDS tile (64 KiB)
static const int kSmpAxis2d = 2048;          // longest axis of a 2-D embedding
static const long long kSmpMaxLen = 1ll << 22;

struct rl_sampler {
    rl_gridop* g = nullptr;      // not owned
    int device = 0, D = 0, m = 0, m1 = 0, m2 = 0;   // m1 == 0: 1-D grid
    bool set = false;
    int Q = 0, nemb = 0, npoly = 0, poly_rank = 0;
    long long zlen = 0;
    // embedding
    int N1 = 0, N2 = 0;          // one-launch path: N1 = Ls, N2 = 1; else Ls = N1 * N2 (2-D: N1s x N2s)
    bool one_launch = false;
    int cols = 1, rows = 1, K1 = 0;
    FftPlan plan1, plan2;
    DevBuf<cplx> tw1, tw2, twlo;
    DevBuf<int> freq1, pos1, freq2;
    DevBuf<int> eC;           // [nemb]
    DevBuf<int> efoff;
    DevBuf<long long> ezoff;
    DevBuf<double> F;         // all blocks
    DevBuf<double> slam;      // [nemb][Ltot]
    std::vector<double> h_lam;   // host [nemb][Ltot]: the clipped spectra (rl_sampler_spectrum_host)
    std::vector<int> emb_of;     // per row: its place among the embedding rows, or -1
    DevBuf<cplx> T;           // [pairs][D][Ltot]
    size_t T_pairs = 0;
    // polynomial rows
    DevBuf<int> pC;
    DevBuf<int> pfoff;
    DevBuf<long long> pzoff;
    DevBuf<double> G;         // [npoly][r][r]
    DevBuf<double> zhat;      // [nsamp][D][r]
};

static void smp_free_params(rl_sampler* h) {
    for (DevBuf<cplx>* b : {&h->tw1, &h->tw2, &h->twlo}) b->reset();
    for (DevBuf<int>* b : {&h->freq1, &h->pos1, &h->freq2, &h->eC, &h->efoff, &h->pC, &h->pfoff}) b->reset();
    for (DevBuf<long long>* b : {&h->ezoff, &h->pzoff}) b->reset();
    for (DevBuf<double>* b : {&h->F, &h->slam, &h->G}) b->reset();
    h->set = false;
}

// ---------------------------------------------------------------------------
// lengths and plans (the schedule rules of rl_gridop.hip's make_plan: odd passes first)
// ---------------------------------------------------------------------------
static bool smp_length_ok(long long n, int* odd_out) {
    if (n < 2 || n > kSmpMaxLen || (n & 1)) return false;
    long long p = n;
    while ((p & 1) == 0) p >>= 1;
    for (int odd : {1, 3, 5, 9, 15, 25})
        if (p == odd) {
            if (odd_out) *odd_out = odd;
            return true;
        }
    return false;
}

extern "C" int rl_sampler_length(long long want, int* length) {
    if (!length) return fail(RL_EINVAL, "rl_sampler_length: length is NULL");
    if (want > kSmpMaxLen)
        return fail(RL_ELIMIT, "rl_sampler_length: embeddings are at most 2^22 points long");
    long long best = 0;
    for (int odd : {1, 3, 5, 9, 15, 25}) {
        long long L = 2ll * odd;
        while (L < want) L *= 2;
        if (L <= kSmpMaxLen && (best == 0 || L < best)) best = L;
    }
    *length = (int)best;
    return RL_OK;
}

static FftPlan smp_plan(int n) {
    FftPlan p;
    p.n = n;
    p.npass = 0;
    for (int i = 0; i < RL_MAX_PASSES; ++i) p.radix[i] = 1;
    int rem = n;
    for (int odd : {3, 5})
        while (rem % odd == 0 && p.npass < 2) {
            p.radix[p.npass++] = odd;
            rem /= odd;
        }
    while (rem > 1) {
        int r = 8;
        while (rem % r) r /= 2;
        p.radix[p.npass++] = r;
        rem /= r;
    }
    return p;
}

// position -> frequency of the in-place forward graph (tests/flow_model.py)
static std::vector<int> smp_pos_to_freq(const FftPlan& p) {
    std::vector<int> f(p.n);
    for (int pos = 0; pos < p.n; ++pos) {
        int rem = pos, ns = p.n, mult = 1, k = 0;
        for (int s = 0; s < p.npass; ++s) {
            const int sub = ns / p.radix[s];
            const int d = rem / sub;
            rem -= d * sub;
            k += d * mult;
            mult *= p.radix[s];
            ns = sub;
        }
        f[pos] = k;
    }
    return f;
}

static std::vector<int> smp_invert(const std::vector<int>& f) {
    std::vector<int> inv(f.size());
    for (size_t i = 0; i < f.size(); ++i) inv[f[i]] = (int)i;
    return inv;
}

// exp(-2 pi i k stride / n), k < count, in long double
static std::vector<cplx> smp_unity(long long count, long long stride, long long n) {
    std::vector<cplx> t(count);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (long long i = 0; i < count; ++i) {
        const long double ang = two_pi * (long double)((i * stride) % n) / (long double)n;
        t[i].x = (double)cosl(ang);
        t[i].y = (double)(-sinl(ang));
    }
    return t;
}

// ---------------------------------------------------------------------------
// host transform of the mirrored rows (set time): recursive decimation in time over the
// smallest prime factor; tw = exp(-2 pi i k / N) of the top-level length
// ---------------------------------------------------------------------------
static void smp_host_fft(const cd* in, size_t stride, cd* out, size_t n, const std::vector<cd>& tw,
                         size_t twstride) {
    if (n == 1) {
        out[0] = in[0];
        return;
    }
    size_t p = 2;
    while (n % p) ++p;
    const size_t sub = n / p, N = tw.size();
    for (size_t r = 0; r < p; ++r) smp_host_fft(in + r * stride, stride * p, out + r * sub, sub, tw, twstride * p);
    cd y[32];
    for (size_t k = 0; k < sub; ++k) {
        for (size_t r = 0; r < p; ++r) y[r] = out[r * sub + k] * tw[(r * k * twstride) % N];
        for (size_t t = 0; t < p; ++t) {
            cd acc = y[0];
            for (size_t r = 1; r < p; ++r) acc += y[r] * tw[(r * t * sub * twstride) % N];
            out[k + sub * t] = acc;
        }
    }
}

static std::vector<cd> smp_host_table(size_t n) {
    std::vector<cd> tw(n);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (size_t k = 0; k < n; ++k) {
        const long double ang = two_pi * (long double)k / (long double)n;
        tw[k] = cd((double)cosl(ang), (double)(-sinl(ang)));
    }
    return tw;
}

// real spectrum of the circulant whose first row is the mirrored lattice ext [(n1/2+1)][(n2/2+1)]
// (n2 == 1: a 1-D row of n1/2 + 1 values), natural order [n1][n2]
static std::vector<double> smp_spectrum(const double* ext, int n1, int n2) {
    const int h1 = n1 / 2 + 1, h2 = n2 > 1 ? n2 / 2 + 1 : 1;
    std::vector<cd> a((size_t)n1 * n2), b((size_t)n1 * n2);
    for (int i = 0; i < n1; ++i) {
        const int li = i < h1 ? i : n1 - i;
        for (int j = 0; j < n2; ++j) {
            const int lj = j < h2 ? j : n2 - j;
            a[(size_t)i * n2 + j] = cd(ext[(size_t)li * h2 + lj], 0.0);
        }
    }
    if (n2 > 1) {
        const std::vector<cd> t2 = smp_host_table(n2);
        for (int i = 0; i < n1; ++i) smp_host_fft(&a[(size_t)i * n2], 1, &b[(size_t)i * n2], n2, t2, 1);
        a.swap(b);
    }
    const std::vector<cd> t1 = smp_host_table(n1);
    std::vector<cd> col(n1);
    std::vector<double> lam((size_t)n1 * n2);
    for (int j = 0; j < n2; ++j) {
        smp_host_fft(&a[j], (size_t)n2, col.data(), n1, t1, 1);
        for (int i = 0; i < n1; ++i) lam[(size_t)i * n2 + j] = col[i].real();
    }
    return lam;
}

// ---------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------
extern "C" int rl_sampler_destroy(rl_sampler* h) {
    if (!h) return RL_OK;
    (void)hipSetDevice(h->device);
    delete h;
    return RL_OK;
}

extern "C" int rl_sampler_create(rl_gridop* g, rl_sampler** out) {
    if (!g || !out) return fail(RL_EINVAL, "rl_sampler_create: NULL argument");
    if (g->lead) {
        *out = nullptr;
        return fail(RL_ELIMIT, "rl_sampler_create: no function draws on a 3-D grid (one- and "
                               "two-dimensional grids only)");
    }
    rl_sampler* h = new rl_sampler();
    h->g = g;
    h->device = g->device;
    h->D = g->D;
    h->m = g->m;
    h->m1 = g->geo.m1;
    h->m2 = g->geo.m1 ? g->geo.m2 : 0;
    *out = h;
    return RL_OK;
}

extern "C" int rl_sampler_set(rl_sampler* h, int Q, const int* nchan, const double* F,
                              const int* forms, int N1s, int N2s, const double* ext_rows,
                              int poly_rank, const double* poly_sqrt, double* clipped,
                              long long* zlen) {
    if (!h || !nchan || !F || !forms || !zlen) return fail(RL_EINVAL, "rl_sampler_set: NULL argument");
    if (Q < 1) return fail(RL_EINVAL, "rl_sampler_set: Q must be >= 1");
    const int D = h->D;
    const bool twod = h->m1 != 0;
    int nemb = 0, npoly = 0;
    for (int q = 0; q < Q; ++q) {
        if (nchan[q] < 1) return fail(RL_EINVAL, "rl_sampler_set: every row needs at least one channel");
        if (forms[q] == 0)
            ++nemb;
        else if (forms[q] == 1)
            ++npoly;
        else
            return fail(RL_EINVAL, "rl_sampler_set: forms are 0 (embedding) or 1 (polynomial)");
    }
    long long Ltot = 0;
    if (nemb) {
        if (!ext_rows) return fail(RL_EINVAL, "rl_sampler_set: embedding rows need ext_rows");
        if (!smp_length_ok(N1s, nullptr) || (twod && !smp_length_ok(N2s, nullptr)))
            return fail(RL_EINVAL, "rl_sampler_set: embedding lengths must be odd * 2^k, odd in "
                                   "{1, 3, 5, 9, 15, 25}, k >= 1 (rl_sampler_length)");
        if (!twod && N2s != 0) return fail(RL_EINVAL, "rl_sampler_set: N2s must be 0 on a 1-D grid");
        const int need1 = twod ? h->m1 : h->m, need2 = twod ? h->m2 : 1;
        if (N1s / 2 < need1 - 1 || (twod && N2s / 2 < need2 - 1))
            return fail(RL_EINVAL, "rl_sampler_set: the embedding must hold every lag of the grid (N / 2 >= m - 1)");
        Ltot = twod ? (long long)N1s * N2s : (long long)N1s;
        if (Ltot > kSmpMaxLen) return fail(RL_ELIMIT, "rl_sampler_set: embeddings are at most 2^22 points");
        if (twod && (N1s > kSmpAxis2d || N2s > kSmpAxis2d))
            return fail(RL_ELIMIT, "rl_sampler_set: at most 2048 points per axis of a 2-D embedding");
    }
    if (npoly) {
        if (twod) return fail(RL_EINVAL, "rl_sampler_set: the polynomial form exists on 1-D grids only");
        if (!poly_sqrt) return fail(RL_EINVAL, "rl_sampler_set: polynomial rows need poly_sqrt");
        if (!h->g->lr_beta || !h->g->lr_nu || h->g->lr_r != poly_rank ||
            (poly_rank != 24 && poly_rank != 32 && poly_rank != 36 && poly_rank != 40 && poly_rank != 48))
            return fail(RL_EINVAL, "rl_sampler_set: poly_rank is not the rank of the grid operator's "
                                   "polynomial form (rl_gridop_poly_coeffs)");
    }
    RL_HIP(hipSetDevice(h->device));
    smp_free_params(h);
    h->Q = Q;
    h->nemb = nemb;
    h->npoly = npoly;
    h->poly_rank = npoly ? poly_rank : 0;
    // per-row tables
    std::vector<int> eC, efoff, pC, pfoff;
    std::vector<long long> ezoff, pzoff;
    long long zo = 0;
    int fo = 0;
    for (int q = 0; q < Q; ++q) {
        const long long len = forms[q] == 0 ? Ltot : (long long)poly_rank;
        (forms[q] == 0 ? eC : pC).push_back(nchan[q]);
        (forms[q] == 0 ? efoff : pfoff).push_back(fo);
        (forms[q] == 0 ? ezoff : pzoff).push_back(zo);
        zo += (long long)nchan[q] * len;
        fo += D * nchan[q];
    }
    h->zlen = zo;
    h->emb_of.assign(Q, -1);
    for (int q = 0, e = 0; q < Q; ++q)
        if (forms[q] == 0) h->emb_of[q] = e++;
    std::vector<double> hF(F, F + fo);
    RL_TRY(h->F.upload(hF));
    if (nemb) {
        RL_TRY(h->eC.upload(eC));
        RL_TRY(h->efoff.upload(efoff));
        RL_TRY(h->ezoff.upload(ezoff));
        // spectra
        const int n1 = N1s, n2 = twod ? N2s : 1;
        const size_t ext_len = (size_t)(n1 / 2 + 1) * (twod ? n2 / 2 + 1 : 1);
        std::vector<double> slam((size_t)nemb * Ltot);
        h->h_lam.assign((size_t)nemb * Ltot, 0.0);
        int e = 0;
        for (int q = 0; q < Q; ++q) {
            if (forms[q] != 0) {
                if (clipped) clipped[q] = 0.0;
                continue;
            }
            const std::vector<double> lam = smp_spectrum(ext_rows + (size_t)e * ext_len, n1, n2);
            long double neg = 0.0L, tot = 0.0L;
            for (long long w = 0; w < Ltot; ++w) {
                const double v = lam[w];
                tot += std::fabs(v);
                if (v < 0.0) neg += -v;
                slam[(size_t)e * Ltot + w] = v > 0.0 ? std::sqrt(v / (double)Ltot) : 0.0;
                h->h_lam[(size_t)e * Ltot + w] = v > 0.0 ? v : 0.0;
            }
            if (clipped) clipped[q] = tot > 0.0L ? (double)(neg / tot) : 0.0;
            ++e;
        }
        RL_TRY(h->slam.upload(slam));
        // transform layout
        h->one_launch = !twod && Ltot <= RL_SAMPLER_LDS_MAX;
        if (h->one_launch) {
            h->N1 = (int)Ltot;
            h->N2 = 1;
        } else if (twod) {
            h->N1 = N1s;
            h->N2 = N2s;
        } else {
            // Ls = N1 N2 with N2 a power of two and the odd factor in N1.  N1 as short as 16 allows
            // (N2 up to kSmpTile): a column tile of k_smp_cols is then 16 columns wide, so that its
            // reads of the noise -- the traffic that matters -- are 128 contiguous bytes per row
            int odd = 1;
            (void)smp_length_ok(Ltot, &odd);
            const long long P = Ltot / odd;
            int n2p = 1;
            while (2 * n2p <= kSmpTile && P % (2 * n2p) == 0 && Ltot / (2 * n2p) >= 16) n2p *= 2;
            h->N2 = n2p;
            h->N1 = (int)(Ltot / n2p);
            if (h->N1 > kSmpTile || h->N2 > kSmpTile || h->N1 < 1)
                return fail(RL_ELIMIT, "rl_sampler_set: embedding length has no two-pass split");
        }
        h->plan1 = smp_plan(h->N1);
        const std::vector<int> f1 = smp_pos_to_freq(h->plan1);
        RL_TRY(h->freq1.upload(f1));
        RL_TRY(h->pos1.upload(smp_invert(f1)));
        RL_TRY(h->tw1.upload(smp_unity(h->N1, 1, h->N1)));
        if (!h->one_launch) {
            h->plan2 = smp_plan(h->N2);
            RL_TRY(h->freq2.upload(smp_pos_to_freq(h->plan2)));
            RL_TRY(h->tw2.upload(smp_unity(h->N2, 1, h->N2)));
            RL_TRY(h->twlo.upload(smp_unity(h->N2, 1, Ltot)));
            h->cols = std::max(1, std::min(16, kSmpTile / h->N1));
            h->rows = std::max(1, std::min(16, kSmpTile / h->N2));
            while (h->rows > 1 && (long long)h->N2 * (h->rows | 1) > kSmpTile) --h->rows;
            h->K1 = twod ? h->m1 : std::min(h->N1, h->m);
        }
    }
    if (npoly) {
        RL_TRY(h->pC.upload(pC));
        RL_TRY(h->pfoff.upload(pfoff));
        RL_TRY(h->pzoff.upload(pzoff));
        std::vector<double> hG(poly_sqrt, poly_sqrt + (size_t)npoly * poly_rank * poly_rank);
        RL_TRY(h->G.upload(hG));
    }
    *zlen = h->zlen;
    h->set = true;
    return RL_OK;
}

extern "C" int rl_sampler_spectrum_host(const rl_sampler* h, int q, double* out) {
    if (!h || !out) return fail(RL_EINVAL, "rl_sampler_spectrum_host: NULL argument");
    if (!h->set || q < 0 || q >= h->Q || h->emb_of[q] < 0)
        return fail(RL_EINVAL, "rl_sampler_spectrum_host: not a row in the embedding form");
    const size_t Ltot = (size_t)h->N1 * h->N2;
    memcpy(out, h->h_lam.data() + (size_t)h->emb_of[q] * Ltot, Ltot * sizeof(double));
    return RL_OK;
}

template <int R>
static void smp_expand(rl_sampler* h, double* U, int nrows, bool accumulate, hipStream_t st) {
    // (one round of four workgroups per compute unit, whatever the number of rows)
    // (a store policy from the knob only: the library's choice was measured on the product)
    const int policy = h->g->kn.lr_policy < 0 ? 0 : h->g->kn.lr_policy;
    lr_expand_launch<R>((const double*)h->zhat, nrows, h->m, (const double*)h->g->lr_beta, U, accumulate,
                        0, 4 * RL_LR_CUS, h->g->kn.lr_expand_plain, policy, st);
}

extern "C" int rl_sampler_draw(rl_sampler* h, const double* Z, double* U, int nsamp, void* stream) {
    if (!h || !Z || !U) return fail(RL_EINVAL, "rl_sampler_draw: NULL argument");
    if (!h->set) return fail(RL_EINVAL, "rl_sampler_draw: no parameters (rl_sampler_set)");
    if (nsamp < 0) return fail(RL_EINVAL, "rl_sampler_draw: nsamp < 0");
    if (nsamp == 0) return RL_OK;
    const int npairs = (nsamp + 1) / 2;
    if (npairs > 65535) return fail(RL_ELIMIT, "rl_sampler_draw: at most 131070 draws per call");
    RL_HIP(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int D = h->D;
    if (h->nemb) {
        SmpRows R{h->nemb, h->eC, h->efoff, h->ezoff, h->F, h->slam};
        if (h->one_launch) {
            trace_once("function draws: embedding, one launch (k_smp_embed1)");
            RL_LAUNCH(k_smp_embed1, dim3(D, npairs), dim3(RL_SMP_THREADS), (size_t)h->N1 * sizeof(cplx), st,
                      Z, h->zlen, R, D, h->m, h->plan1, (const cplx*)h->tw1, (const int*)h->pos1, U, nsamp);
        } else {
            trace_once("function draws: embedding, two passes (k_smp_cols / k_smp_rows)");
            const size_t Ltot = (size_t)h->N1 * h->N2;
            if ((size_t)npairs > h->T_pairs) {
                h->T_pairs = 0;
                if (h->T.renew((size_t)npairs * D * Ltot) != RL_OK) {
                    (void)hipGetLastError();
                    return fail(RL_ENOMEM, "rl_sampler_draw: no device memory for the intermediates of " +
                                               std::to_string(npairs) + " pairs");
                }
                h->T_pairs = npairs;
            }
            const int twod = h->m1 != 0;
            RL_LAUNCH(k_smp_cols, dim3(D, (h->N2 + h->cols - 1) / h->cols, npairs), dim3(RL_SMP_THREADS),
                      (size_t)h->N1 * h->cols * sizeof(cplx), st, Z, h->zlen, R, D, h->plan1, h->N2, h->cols,
                      (const cplx*)h->tw1, (const cplx*)h->twlo, (const int*)h->freq1, twod ? 0 : 1, h->T);
            const int ld = h->rows | 1;
            RL_LAUNCH(k_smp_rows, dim3(D, (h->K1 + h->rows - 1) / h->rows, npairs), dim3(RL_SMP_THREADS),
                      (size_t)h->N2 * ld * sizeof(cplx), st, (const cplx*)h->T, D, h->N1, h->plan2, h->rows, ld,
                      h->K1, (const cplx*)h->tw2, (const int*)h->pos1, (const int*)h->freq2, h->m,
                      twod ? h->m2 : 0, U, nsamp);
        }
    }
    if (h->npoly) {
        const int r = h->poly_rank;
        if (!h->g->lr_beta || h->g->lr_r != r)
            return fail(RL_EINVAL, "rl_sampler_draw: the grid operator's polynomial form changed since rl_sampler_set");
        const size_t need = (size_t)nsamp * D * r;
        RL_TRY(h->zhat.reserve(need));
        trace_once("function draws: polynomial rows (k_smp_poly_coef + k_lr_expand)");
        RL_LAUNCH(k_smp_poly_coef, dim3((unsigned)((need + 255) / 256)), dim3(RL_SMP_THREADS), 0, st, Z, h->zlen,
                  h->npoly, (const int*)h->pC, (const int*)h->pfoff, (const long long*)h->pzoff,
                  (const double*)h->F, (const double*)h->G, (const double*)h->g->lr_nu, D, r, nsamp, h->zhat);
        const bool acc = h->nemb > 0;
        switch (r) {
            case 24: smp_expand<24>(h, U, nsamp * D, acc, st); break;
            case 32: smp_expand<32>(h, U, nsamp * D, acc, st); break;
            case 36: smp_expand<36>(h, U, nsamp * D, acc, st); break;
            case 40: smp_expand<40>(h, U, nsamp * D, acc, st); break;
            default: smp_expand<48>(h, U, nsamp * D, acc, st); break;
        }
    }
    RL_HIP(hipGetLastError());
    return RL_OK;
}

extern "C" int rl_normal_fill(unsigned long long seed, long long draw0, int ndraws, long long zlen,
                              double* Z, void* stream) {
    if (ndraws < 0 || zlen < 0 || draw0 < 0) return fail(RL_EINVAL, "rl_normal_fill: negative size");
    if (ndraws == 0 || zlen == 0) return RL_OK;
    if (!Z) return fail(RL_EINVAL, "rl_normal_fill: Z is NULL");
    if (ndraws > 65535) return fail(RL_ELIMIT, "rl_normal_fill: at most 65535 rows per call");
    const long long blocks = std::min<long long>((zlen + RL_SMP_THREADS - 1) / RL_SMP_THREADS, 4096);
    RL_LAUNCH(k_smp_normal, dim3((unsigned)blocks, ndraws), dim3(RL_SMP_THREADS), 0, (hipStream_t)stream, seed,
              draw0, zlen, Z);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

extern "C" int rl_pathwise_residual(const double* y, const double* WU, const double* E,
                                    const double* sqrt_eps_rows, double* R, int nsamp, long long n,
                                    void* stream) {
    if (nsamp < 0 || n < 0) return fail(RL_EINVAL, "rl_pathwise_residual: negative size");
    if (nsamp == 0 || n == 0) return RL_OK;
    if (!y || !WU || !E || !sqrt_eps_rows || !R) return fail(RL_EINVAL, "rl_pathwise_residual: NULL argument");
    if (nsamp > 65535) return fail(RL_ELIMIT, "rl_pathwise_residual: at most 65535 rows per call");
    const long long blocks = std::min<long long>((n + RL_SMP_THREADS - 1) / RL_SMP_THREADS, 4096);
    RL_LAUNCH(k_smp_residual, dim3((unsigned)blocks, nsamp), dim3(RL_SMP_THREADS), 0, (hipStream_t)stream, y, WU, E,
              sqrt_eps_rows, R, n);
    RL_HIP(hipGetLastError());
    return RL_OK;
}
