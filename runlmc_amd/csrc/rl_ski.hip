// SKI operator K~ = sum_t W_t K_t W_t^T + diag(eps): handles, interpolation products, the
// row-polynomial form of a polynomial-form operator, products in the caller's and in the
// internal row order (one of the three translation units of librunlmc_hip.so, rl_host.h).
#include "rl_host.h"


// Small batches want every (row, vector) on its own thread (latency-bound);
// large ones want the CSR entries reused across a block of vectors
// (bandwidth-bound: the structure is 12 bytes per non-zero per pass).
static void launch_spmv(const int* indptr, const int* indices, const double* vals, int nrows,
                        int ncols, int nvec, const double* X, double* Y, const double* diag,
                        const double* X2, hipStream_t st, int accumulate = 0,
                        int* bump = nullptr, int avg_nnz = 0) {
    const unsigned gx = (nrows + RL_THREADS - 1) / RL_THREADS;
    const bool blocked = (size_t)nrows * nvec >= ((size_t)1 << 22);
    // long rows of a small product: eight lanes per row (k_spmv_wide)
    if (!blocked && avg_nnz > 12 && diag == nullptr && !accumulate) {
        const unsigned gw = (unsigned)(((size_t)nrows * 8 + RL_THREADS - 1) / RL_THREADS);
        RL_LAUNCH(k_spmv_wide<8>, dim3(gw, nvec), dim3(RL_THREADS), RL_THREADS * sizeof(double), st,
                  indptr, indices, vals, nrows, ncols, X, Y, bump);
        return;
    }
    if (blocked) {
        RL_LAUNCH(k_spmv<8>, dim3(gx, (nvec + 7) / 8), dim3(RL_THREADS), 0, st, indptr, indices,
                  vals, nrows, ncols, nvec, X, Y, diag, X2, accumulate, bump);
    } else {
        RL_LAUNCH(k_spmv<1>, dim3(gx, nvec), dim3(RL_THREADS), 0, st, indptr, indices, vals,
                  nrows, ncols, nvec, X, Y, diag, X2, accumulate, bump);
    }
}

static int check_csr(const int* indptr, const int* indices, int nrows, int ncols,
                     const char* what) {
    if (!indptr || indptr[0] != 0) return fail(RL_EINVAL, std::string(what) + ": bad indptr[0]");
    for (int i = 0; i < nrows; ++i)
        if (indptr[i + 1] < indptr[i])
            return fail(RL_EINVAL, std::string(what) + ": indptr not monotone");
    const int nnz = indptr[nrows];
    if (nnz > 0 && !indices) return fail(RL_EINVAL, std::string(what) + ": indices is NULL");
    for (int k = 0; k < nnz; ++k)
        if (indices[k] < 0 || indices[k] >= ncols)
            return fail(RL_EINVAL, std::string(what) + ": column index out of range");
    return RL_OK;
}

// Upload one term's CSR pair, rows of W (and column indices of WT) renumbered
// by `perm` (perm[i] = caller's row of internal row i) when given.
static int upload_term(SkiTerm* t, int n, int ngrid, const int* W_indptr, const int* W_indices,
                       const double* W_data, const int* WT_indptr, const int* WT_indices,
                       const double* WT_data, const std::vector<int>* perm) {
    const size_t nnz = W_indptr[n];
    std::vector<int> wp_ptr, wp_idx, wtp_idx;
    std::vector<double> wp_val, wtp_val;
    if (perm) {
        std::vector<int> inv(n);
        for (int i = 0; i < n; ++i) inv[(*perm)[i]] = i;
        wp_ptr.assign(n + 1, 0);
        wp_idx.reserve(nnz);
        wp_val.reserve(nnz);
        for (int i = 0; i < n; ++i) {
            const int r = (*perm)[i];
            for (int k = W_indptr[r]; k < W_indptr[r + 1]; ++k) {
                wp_idx.push_back(W_indices[k]);
                wp_val.push_back(W_data[k]);
            }
            wp_ptr[i + 1] = (int)wp_idx.size();
        }
        wtp_idx.resize(nnz);
        wtp_val.resize(nnz);
        std::vector<std::pair<int, double>> row;
        for (int r = 0; r < ngrid; ++r) {
            row.clear();
            for (int k = WT_indptr[r]; k < WT_indptr[r + 1]; ++k)
                row.emplace_back(inv[WT_indices[k]], WT_data[k]);
            std::sort(row.begin(), row.end());
            for (size_t j = 0; j < row.size(); ++j) {
                wtp_idx[WT_indptr[r] + j] = row[j].first;
                wtp_val[WT_indptr[r] + j] = row[j].second;
            }
        }
        W_indptr = wp_ptr.data(); W_indices = wp_idx.data(); W_data = wp_val.data();
        WT_indices = wtp_idx.data(); WT_data = wtp_val.data();
    }
    t->ngrid = ngrid;
    // interpolation structure (see SkiTerm)
    std::vector<int> base, lo, sp_ptr, sp_idx;
    std::vector<double> w4, sp_val;
    {
        bool ok = ngrid >= 4;
        base.resize(n);
        w4.assign((size_t)4 * n, 0.0);
        int prev = 0;
        for (int i = 0; i < n && ok; ++i) {
            const int k0 = W_indptr[i], cnt = W_indptr[i + 1] - k0;
            if (cnt > 4) { ok = false; break; }
            for (int j = 1; j < cnt; ++j)
                if (W_indices[k0 + j] != W_indices[k0] + j) ok = false;
            int b = cnt ? W_indices[k0] : prev, shift = 0;
            if (b > ngrid - 4) { shift = b - (ngrid - 4); b = ngrid - 4; }
            if (shift + cnt > 4 || b < prev) { ok = false; break; }
            prev = b;
            base[i] = b;
            for (int j = 0; j < cnt; ++j) w4[(size_t)4 * i + shift + j] = W_data[k0 + j];
        }
        if (ok) {
            // W^T: grid row r is touched by the rows with base in [r - 3, r]
            lo.resize(ngrid);
            sp_ptr.assign(ngrid + 1, 0);
            int a = 0, e = 0;
            for (int r = 0; r < ngrid; ++r) {
                while (a < n && base[a] < r - 3) ++a;
                while (e < n && base[e] <= r) ++e;
                lo[r] = a;
                sp_ptr[r + 1] = sp_ptr[r] + (e - a);
                for (int i = a; i < e; ++i) {
                    sp_idx.push_back(i);
                    sp_val.push_back(w4[(size_t)4 * i + (r - base[i])]);
                }
            }
            t->h_base = base;
            RL_TRY(t->W4_base.upload(base.data(), (size_t)n));
            RL_TRY(t->W4_w.upload(w4.data(), (size_t)4 * n));
            RL_TRY(t->WT_lo.upload(lo.data(), (size_t)ngrid));
            WT_indptr = sp_ptr.data(); WT_indices = sp_idx.data(); WT_data = sp_val.data();
            for (int r0 = 0; r0 < n; r0 += RL_THREADS)
                t->w_xmax = std::max(t->w_xmax,
                                     base[std::min(n, r0 + RL_THREADS) - 1] + 4 - base[r0]);
            for (int r0 = 0; r0 < ngrid; r0 += RL_THREADS) {
                const int rl = std::min(ngrid, r0 + RL_THREADS) - 1;
                const int c1 = lo[rl] + (sp_ptr[rl + 1] - sp_ptr[rl]);
                t->wt_xmax = std::max(t->wt_xmax, c1 - lo[r0]);
                t->wt_emax = std::max(t->wt_emax, sp_ptr[rl + 1] - sp_ptr[r0]);
            }
        }
    }
    const size_t nnzT = WT_indptr[ngrid];
    t->nnzWT = (int)nnzT;
    RL_TRY(t->W_indptr.upload(W_indptr, (size_t)n + 1));
    RL_TRY(t->W_indices.upload(W_indices, nnz));
    RL_TRY(t->W_data.upload(W_data, nnz));
    RL_TRY(t->WT_indptr.upload(WT_indptr, (size_t)ngrid + 1));
    RL_TRY(t->WT_indices.upload(WT_indices, nnzT));
    RL_TRY(t->WT_data.upload(WT_data, nnzT));
    return RL_OK;
}

extern "C" int rl_ski_create(rl_gridop* g, int n, const int* W_indptr, const int* W_indices,
                             const double* W_data, const int* WT_indptr, const int* WT_indices,
                             const double* WT_data, rl_ski** out) {
    if (!out) return fail(RL_EINVAL, "out is NULL");
    *out = nullptr;
    if (!g) return fail(RL_EINVAL, "gridop is NULL");
    if (n < 1) return fail(RL_EINVAL, "rl_ski_create: n < 1");
    const int ngrid = g->D * g->m;
    RL_TRY(check_csr(W_indptr, W_indices, n, ngrid, "W"));
    RL_TRY(check_csr(WT_indptr, WT_indices, ngrid, n, "WT"));
    if (W_indptr[n] != WT_indptr[ngrid])
        return fail(RL_EINVAL, "rl_ski_create: W and WT have different nnz");
    RL_HIP(hipSetDevice(g->device));
    rl_ski* s = new rl_ski;
    HandleGuard<rl_ski, rl_ski_destroy> guard(s);
    s->kn = read_knobs();
    s->g = g;
    s->device = g->device;
    s->n = n;
    s->ngrid = ngrid;
    // sort the data points by the first grid point they touch
    std::vector<int> perm(n);
    for (int i = 0; i < n; ++i) perm[i] = i;
    auto key = [&](int i) {
        return W_indptr[i + 1] > W_indptr[i] ? W_indices[W_indptr[i]] : 0x7fffffff;
    };
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return key(a) < key(b); });
    bool identity = true;
    for (int i = 0; i < n && identity; ++i) identity = perm[i] == i;
    if (s->kn.no_sort) identity = true;
    if (!identity) {
        s->permuted = true;
        s->h_perm = perm;
        RL_TRY(s->perm.upload(perm.data(), (size_t)n));
    }
    SkiTerm t0;
    t0.g = g;
    RL_TRY(upload_term(&t0, n, ngrid, W_indptr, W_indices, W_data, WT_indptr, WT_indices,
                       WT_data, s->permuted ? &s->h_perm : nullptr));
    s->terms.push_back(std::move(t0));
    s->max_ngrid = ngrid;
    s->nnz = W_indptr[n];
    RL_TRY(s->noise_diag.reserve((size_t)n));
    RL_HIP(hipMemset(s->noise_diag, 0, (size_t)n * sizeof(double)));
    *out = guard.release();
    return RL_OK;
}

extern "C" int rl_ski_add_term(rl_ski* s, rl_gridop* g, const int* W_indptr,
                               const int* W_indices, const double* W_data,
                               const int* WT_indptr, const int* WT_indices,
                               const double* WT_data) {
    if (!s || !g) return fail(RL_EINVAL, "rl_ski_add_term: NULL handle");
    if (g->D != s->g->D || g->device != s->g->device)
        return fail(RL_EINVAL, "rl_ski_add_term: grid operator has another D or device");
    const int ngrid = g->D * g->m;
    RL_TRY(check_csr(W_indptr, W_indices, s->n, ngrid, "W"));
    RL_TRY(check_csr(WT_indptr, WT_indices, ngrid, s->n, "WT"));
    if (W_indptr[s->n] != WT_indptr[ngrid])
        return fail(RL_EINVAL, "rl_ski_add_term: W and WT have different nnz");
    RL_HIP(hipSetDevice(g->device));
    SkiTerm t;
    t.g = g;
    // the handle's row order was fixed by its first term
    RL_TRY(upload_term(&t, s->n, ngrid, W_indptr, W_indices, W_data, WT_indptr, WT_indices,
                       WT_data, s->permuted ? &s->h_perm : nullptr));
    s->terms.push_back(std::move(t));
    if (ngrid > s->max_ngrid) {
        s->max_ngrid = ngrid;
        s->cap = 0;            // grid-side temporaries must grow
    }
    return RL_OK;
}


extern "C" int rl_ski_destroy(rl_ski* s) {
    if (!s) return RL_OK;
    (void)hipSetDevice(s->device);
    if (s->solver_stream) (void)hipStreamDestroy(s->solver_stream);
    if (s->pin_count) (void)hipHostFree(s->pin_count);
    for (hipEvent_t e : s->count_ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
    return RL_OK;
}

// the diagonal repeat(noise, lens) in the caller's row order, checked against the handle
static int ski_noise_diag(const rl_ski* s, const char* who, const double* noise, const int* lens,
                          std::vector<double>* diag) {
    diag->clear();
    diag->reserve(s->n);
    for (int d = 0; d < s->g->D; ++d) {
        if (lens[d] < 0) return fail(RL_EINVAL, std::string(who) + ": negative length");
        diag->insert(diag->end(), (size_t)lens[d], noise[d]);
    }
    if ((int)diag->size() != s->n)
        return fail(RL_EINVAL, std::string(who) + ": sum(lens) != n");
    return RL_OK;
}

// what rl_ski_set_noise and rl_ski_set_noise_rows share: a diagonal in the caller's row order
// becomes the handle's (permuted, its runs, the device array, a new noise version)
static int ski_install_noise(rl_ski* s, std::vector<double>& diag) {
    s->caller_noise_same = true;
    if (s->permuted) {
        std::vector<double> sorted(diag.size());
        for (int i = 0; i < s->n; ++i) sorted[i] = diag[s->h_perm[i]];
        for (int i = 0; i < s->n && s->caller_noise_same; ++i)
            s->caller_noise_same = sorted[i] == diag[i];
        diag.swap(sorted);
    }
    // runs of equal values in internal order (one per output when every output's
    // rows are contiguous): what the solver's vector kernel takes instead of the array
    s->eps_end.clear();
    s->eps_val.clear();
    for (int i = 0; i < s->n; ++i) {
        if (i == 0 || diag[i] != diag[i - 1]) {
            if ((int)s->eps_val.size() == RL_MAX_D) {       // not per-output after all
                s->eps_end.clear();
                s->eps_val.clear();
                break;
            }
            if (i > 0) s->eps_end.push_back(i);
            s->eps_val.push_back(diag[i]);
        }
    }
    if (!s->eps_val.empty()) s->eps_end.push_back(s->n);
    RL_HIP(hipSetDevice(s->g->device));
    RL_HIP(hipMemcpy(s->noise_diag, diag.data(), diag.size() * sizeof(double),
                     hipMemcpyHostToDevice));
    s->has_noise = true;
    s->h_noise.swap(diag);
    ++s->noise_ver;
    return RL_OK;
}

extern "C" int rl_ski_set_noise(rl_ski* s, const double* noise, const int* lens) {
    if (!s || !noise || !lens) return fail(RL_EINVAL, "rl_ski_set_noise: NULL argument");
    std::vector<double> diag;
    RL_TRY(ski_noise_diag(s, "rl_ski_set_noise", noise, lens, &diag));
    RL_TRY(ski_install_noise(s, diag));
    s->row_noise = false;
    return RL_OK;
}

// e = repeat(noise, lens) + extra, extra >= 0 per observation in the caller's row order (known
// variances: never a parameter).  Marks the handle: its factorisation takes the scaled form of
// rl_rownoise.h, where a diagonal set through rl_ski_set_noise must be constant per output.
extern "C" int rl_ski_set_noise_rows(rl_ski* s, const double* noise, const int* lens, const double* extra) {
    if (!s || !noise || !lens || !extra) return fail(RL_EINVAL, "rl_ski_set_noise_rows: NULL argument");
    std::vector<double> diag;
    RL_TRY(ski_noise_diag(s, "rl_ski_set_noise_rows", noise, lens, &diag));
    for (int i = 0; i < s->n; ++i) {
        if (!(extra[i] >= 0.0) || !std::isfinite(extra[i]))
            return fail(RL_EINVAL, "rl_ski_set_noise_rows: extra[" + std::to_string(i) +
                                       "] is negative or not finite");
        diag[i] += extra[i];
    }
    RL_TRY(ski_install_noise(s, diag));
    s->row_noise = true;
    return RL_OK;
}

int ski_reserve(rl_ski* s, int nvec) {
    if (nvec <= s->cap && s->G1) return RL_OK;
    s->G1.reset();
    s->G2.reset();
    s->cap = 0;
    RL_TRY(s->G1.reserve((size_t)nvec * s->max_ngrid));
    RL_TRY(s->G2.reserve((size_t)nvec * s->max_ngrid));
    s->cap = nvec;
    return RL_OK;
}

int ski_reserve_perm(rl_ski* s, int nvec) {
    if (!s->permuted || nvec <= s->pcap) return RL_OK;
    s->P1.reset();
    s->P2.reset();
    s->pcap = 0;
    RL_TRY(s->P1.reserve((size_t)nvec * s->n));
    RL_TRY(s->P2.reserve((size_t)nvec * s->n));
    s->pcap = nvec;
    return RL_OK;
}

// caller order <-> internal (sorted) order
void permute_rows(rl_ski* s, const double* X, double* Y, int nvec, int scatter,
                         hipStream_t st) {
    // (row-block count padded to a multiple of 8 for the XCD-aware order; the
    // kernel masks rows past n)
    dim3 grid((((s->n + RL_THREADS - 1) / RL_THREADS) + 7) / 8 * 8, nvec);
    RL_LAUNCH(k_permute_rows, grid, dim3(RL_THREADS), 0, st, X, Y, (const int*)s->perm, s->n,
              scatter);
}

// groups of 8 vectors a staged-SpMV workgroup walks with the same rows
// (measured at C5: DESIGN.md)
static int staged_vgroups() { return 4; }

// the 64 KiB dynamic-LDS opt-in of a staged kernel's three instantiations, once per device
template <class K>
static void staged_lds_optin(unsigned long long* seen, K k1, K k2, K k4) {
    if (!first_on_device(seen)) return;
    for (K k : {k1, k2, k4})
        (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
}
// the three stages in INTERNAL row order
int ski_wt_int(rl_ski* s, const SkiRoute& route, const double* Xp, double* G, int nvec, hipStream_t st,
               int* bump) {
    constexpr int VB = 8;
    const size_t lds = ((size_t)VB * s->terms[0].wt_xmax + s->terms[0].wt_emax) * sizeof(double);
    if (route.wt_staged) {
        trace_once("W^T product: k_spmv_wt_staged");
        static unsigned long long seen = 0;
        staged_lds_optin(&seen, k_spmv_wt_staged<VB, 1>, k_spmv_wt_staged<VB, 2>, k_spmv_wt_staged<VB, 4>);
        const unsigned gx = (s->ngrid + RL_THREADS - 1) / RL_THREADS;
        const int vg = staged_vgroups();
        const dim3 grid(gx, ((nvec + VB - 1) / VB + vg - 1) / vg);
#define RL_WT_STAGED(XPT)                                                                       \
    RL_LAUNCH((k_spmv_wt_staged<VB, XPT>), grid, dim3(RL_THREADS), lds, st,                     \
              (const int*)s->terms[0].WT_indptr, (const int*)s->terms[0].WT_lo,                 \
              (const double*)s->terms[0].WT_data, s->ngrid, s->n, nvec, Xp, G, s->terms[0].wt_xmax, vg, bump)
        if (s->terms[0].wt_xmax <= RL_THREADS) RL_WT_STAGED(1);
        else if (s->terms[0].wt_xmax <= 2 * RL_THREADS) RL_WT_STAGED(2);
        else RL_WT_STAGED(4);
#undef RL_WT_STAGED
        RL_HIP(hipGetLastError());
        return RL_OK;
    }
    launch_spmv(s->terms[0].WT_indptr, s->terms[0].WT_indices, s->terms[0].WT_data, s->ngrid, s->n,
                nvec, Xp, G, nullptr, nullptr, st, 0, bump, s->ngrid > 0 ? s->terms[0].nnzWT / s->ngrid : 0);
    RL_HIP(hipGetLastError());
    return RL_OK;
}
// ... and with MINRES's P inside (k_spmv_w_staged_p: the partial sums' words next to the tile,
// row accesses by 32-bit byte offsets)
static size_t w_staged_p_lds(const rl_ski* s) {
    constexpr int VB = 8;
    size_t lds = ((size_t)VB * s->terms[0].w_xmax + (size_t)staged_vgroups() * VB * 8) * sizeof(double);
#if defined(RL_EMU)
    lds += 256 * sizeof(double);
#endif
    return lds;
}
// The route of a K~ product of nvec vectors (rl_host.h SkiRoute): the one place that knows.
// (The interpolation kernels of the first term; further terms always run CSR products.)
SkiRoute ski_route(const rl_ski* s, int nvec) {
    constexpr int VB = 8;
    const SkiTerm& t = s->terms[0];
    const rl_gridop* g = s->g;
    SkiRoute r;
    // large batch (or the test hook), structured W / W^T whose workgroup ranges fit LDS: staged
    // forms (measured at C5, 129 vectors: see DESIGN.md)
    const bool staged_on = !s->kn.no_staged_wt;
    const bool large_rows = (size_t)s->n * nvec >= ((size_t)1 << 22) || s->kn.staged_wt;
    const size_t wt_lds = ((size_t)VB * t.wt_xmax + t.wt_emax) * sizeof(double);
    r.wt_staged = t.WT_lo != nullptr && t.wt_xmax > 0 && wt_lds <= 64 * 1024 &&
                  t.wt_xmax <= 4 * RL_THREADS &&
                  ((size_t)s->ngrid * nvec >= ((size_t)1 << 22) || s->kn.staged_wt) && staged_on;
    const bool w4 = t.W4_base != nullptr && t.w_xmax > 0;
    r.w_staged = w4 && (size_t)VB * t.w_xmax * sizeof(double) <= 64 * 1024 &&
                 t.w_xmax <= 4 * RL_THREADS && large_rows && staged_on;
    r.w_staged_p = single_term(s) && r.w_staged && w_staged_p_lds(s) <= 64 * 1024 && s->n < (1 << 28);
    r.grid_poly = g->lr_ok && !g->lr_dirty;
    // the W product takes the grid values from the polynomial form's mixed coefficients
    // (k_spmv_w_poly): staged W on a 1-D grid the polynomial form is eligible for; whether the
    // operator IS in that form at a rank the kernel takes the grid handle decides when the
    // product runs (its verification may still be pending here): GridRoute::deferrable
    r.w_poly = w4 && t.w_xmax <= 2 * RL_THREADS &&
               ((size_t)VB * t.w_xmax + (size_t)VB * 2 * RL_LR_RMAX) * sizeof(double) <= 64 * 1024 &&
               large_rows && staged_on && (g->lr_try || g->lr_ok) && g->m >= 4 * RL_THREADS &&
               s->ngrid == g->D * g->m && !s->kn.no_w_poly;
    // the operator as F M F^T: single term, structured W on a 1-D grid, every top row in the
    // polynomial form, a large system
    r.rowpoly = single_term(s) && t.W4_base != nullptr && !t.h_base.empty() &&
           !g->wide && !g->lead &&
           g->lr_try && !g->lr_dirty && g->lr_ok && s->ngrid == g->D * g->m &&
           s->n < (1 << 28) &&          // (k_rp_expand's row accesses carry 32-bit byte offsets)
           // (the batch gate of the structured forms also gates this one: rl_gridop_set_form_gate
           // with a huge value puts the whole operator back on the transform kernels)
           (size_t)nvec * g->D * g->m >= g->lr_min && large_rows &&
           // (F is read twice per product whatever the batch: at ranks above 32 a batch of a
           // few dozen vectors is level with the interpolation products or behind them --
           // C5, 17 vectors, rank 36: 0.615 against 0.587 ms per round; rank 24: 0.49 against 0.53)
           // (... except batches of at most 17, which take the small-batch projection:
           // rank 36, 17 vectors: see profiles/r04/rp_ab.txt)
           (g->lr_r <= 32 || nvec >= 48 || nvec <= RL_RP_VG + 1 || s->kn.staged_wt) &&
           staged_on && !s->kn.no_rp;
    if (r.rowpoly) {
        r.rank = g->lr_r;
        r.rp_part_per_run = (size_t)nvec * r.rank;
        r.lr_zhat = (size_t)nvec * g->D * RL_LR_RMAX;
    }
    return r;
}
// F for the route's rank, the runs and the partial sums of the batch are there (rp_prepare)
bool ski_ready(const rl_ski* s, const SkiRoute& r) {
    return !r.rowpoly || (s->rp_F != nullptr && s->rp_R == r.rank && s->rp_runs != nullptr &&
                          s->rp_part.cap >= (size_t)s->rp_nruns * r.rp_part_per_run &&
                          s->g->lr_zhat.cap >= r.lr_zhat);
}
// (pf.pc != NULL: MINRES's P inside the product, no output vector -- ski_mvm_int checked that
// the route admits it)
static int ski_w_int(rl_ski* s, const SkiRoute& route, const double* G, double* Yp, int nvec,
                     const double* diag, const double* X2p, hipStream_t st, const RpPFuse& pf) {
    // large batch, structured W: staged form (see ski_wt_int)
    constexpr int VB = 8;
    const size_t lds = (size_t)VB * s->terms[0].w_xmax * sizeof(double);
    const int vg = staged_vgroups();
    const dim3 grid((s->n + RL_THREADS - 1) / RL_THREADS, ((nvec + VB - 1) / VB + vg - 1) / vg);
    if (pf.pc != nullptr) {
        trace_once("W product: k_spmv_w_staged_p (MINRES's P inside)");
        static unsigned long long seenp = 0;
        staged_lds_optin(&seenp, k_spmv_w_staged_p<VB, 1>, k_spmv_w_staged_p<VB, 2>, k_spmv_w_staged_p<VB, 4>);
        const size_t ldsp = w_staged_p_lds(s);
#define RL_W_STAGED_P(XPT)                                                                      \
    RL_LAUNCH((k_spmv_w_staged_p<VB, XPT>), grid, dim3(RL_THREADS), ldsp, st,                   \
              (const int*)s->terms[0].W4_base, (const double*)s->terms[0].W4_w, s->n, s->ngrid, \
              nvec, G, diag, X2p, s->terms[0].w_xmax, vg, pf)
        if (s->terms[0].w_xmax <= RL_THREADS) RL_W_STAGED_P(1);
        else if (s->terms[0].w_xmax <= 2 * RL_THREADS) RL_W_STAGED_P(2);
        else RL_W_STAGED_P(4);
#undef RL_W_STAGED_P
        RL_HIP(hipGetLastError());
        return RL_OK;
    }
    if (route.w_staged) {
        trace_once("W product: k_spmv_w_staged");
        static unsigned long long seen = 0;
        staged_lds_optin(&seen, k_spmv_w_staged<VB, 1>, k_spmv_w_staged<VB, 2>, k_spmv_w_staged<VB, 4>);
#define RL_W_STAGED(XPT)                                                                        \
    RL_LAUNCH((k_spmv_w_staged<VB, XPT>), grid, dim3(RL_THREADS), lds, st,                      \
              (const int*)s->terms[0].W4_base, (const double*)s->terms[0].W4_w, s->n, s->ngrid, \
              nvec, G, Yp, diag, X2p, s->terms[0].w_xmax, vg)
        if (s->terms[0].w_xmax <= RL_THREADS) RL_W_STAGED(1);
        else if (s->terms[0].w_xmax <= 2 * RL_THREADS) RL_W_STAGED(2);
        else RL_W_STAGED(4);
#undef RL_W_STAGED
        RL_HIP(hipGetLastError());
        return RL_OK;
    }
    launch_spmv(s->terms[0].W_indptr, s->terms[0].W_indices, s->terms[0].W_data, s->n, s->ngrid, nvec,
                G, Yp, diag, X2p, st);
    RL_HIP(hipGetLastError());
    return RL_OK;
}
static int ski_w_poly(rl_ski* s, double* Yp, int nvec, const double* diag, const double* X2p,
                      hipStream_t st) {
    constexpr int VB = 8;
    rl_gridop* g = s->g;
    const int R = g->lr_r;
    const size_t lds = ((size_t)VB * s->terms[0].w_xmax + (size_t)VB * 2 * R) * sizeof(double);
    trace_once("W product: k_spmv_w_poly (grid values from the mixed coefficients)");
    const unsigned gx = (s->n + RL_THREADS - 1) / RL_THREADS;
    const int vg = staged_vgroups();
    const dim3 grid(gx, ((nvec + VB - 1) / VB + vg - 1) / vg);
#define RL_W_POLY(XPT, R_)                                                                      \
    RL_LAUNCH((k_spmv_w_poly<VB, XPT, R_>), grid, dim3(RL_THREADS), lds, st,                    \
              (const int*)s->terms[0].W4_base, (const double*)s->terms[0].W4_w, s->n, s->ngrid, \
              nvec,                                                                             \
              (const double*)g->lr_zhat, (const double*)g->lr_beta, g->D, g->m, Yp, diag, X2p,  \
              s->terms[0].w_xmax, vg)
    if (R == 24) {
        if (s->terms[0].w_xmax <= RL_THREADS) RL_W_POLY(1, 24);
        else RL_W_POLY(2, 24);
    } else if (R == 32) {
        if (s->terms[0].w_xmax <= RL_THREADS) RL_W_POLY(1, 32);
        else RL_W_POLY(2, 32);
    } else if (R == 36) {
        if (s->terms[0].w_xmax <= RL_THREADS) RL_W_POLY(1, 36);
        else RL_W_POLY(2, 36);
    } else {
        return fail(RL_EINVAL, "k_spmv_w_poly: no instantiation for this rank");
    }
#undef RL_W_POLY
    RL_HIP(hipGetLastError());
    return RL_OK;
}
// ---------------------------------------------------------------------------
// Row-polynomial form of large solver rounds (rl_rowpoly.h)
// ---------------------------------------------------------------------------
// F for the operator's current rank, the runs of rows k_rp_project walks, the partial sums
// of nvec vectors.  Allocates: never inside a stream capture (the solver calls it before).
int rp_prepare(rl_ski* s, int nvec) {
    rl_gridop* g = s->g;
    const int R = g->lr_r, n = s->n, D = g->D, m = g->m;
    if (s->rp_R != R) {
        s->rp_R = 0;
        RL_TRY(s->rp_F.renew((size_t)R * n));
        RL_LAUNCH(k_rp_build, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t) nullptr,
                  (const int*)s->terms[0].W4_base, (const double*)s->terms[0].W4_w, n, m, R,
                  (const double*)g->lr_beta, s->rp_F);
        RL_HIP(hipGetLastError());
        RL_HIP(hipDeviceSynchronize());
        s->rp_R = R;
    }
    if (!s->rp_runs) {
        // rows of an output are contiguous in the sorted order; runs of whole tiles, about five
        // hundred of them (C5, rows per run 512 ... 2048: the projection 344-371 us at 129
        // vectors, 74-76 at 17; k_lr_mix, which sums the runs, 32 -> 18 us: the longest wins)
        std::vector<int> out_end(D, 0), run_ptr(D + 1, 0), runs;
        int len = ((n + 511) / 512 + RL_RP_TILE - 1) / RL_RP_TILE * RL_RP_TILE;
        len = std::max(RL_RP_TILE, std::min(len, 64 * RL_RP_TILE));
        if (s->kn.rp_runlen > 0) len = (s->kn.rp_runlen + RL_RP_TILE - 1) / RL_RP_TILE * RL_RP_TILE;
        int i = 0;
        for (int d = 0; d < D; ++d) {
            const int start = i;
            while (i < n && s->terms[0].h_base[i] < (d + 1) * m) ++i;
            out_end[d] = i;
            run_ptr[d] = (int)runs.size() / 3;
            for (int r0 = start; r0 < i; r0 += len) {
                runs.push_back(r0);
                runs.push_back(std::min(r0 + len, i));
                runs.push_back(d);
            }
        }
        run_ptr[D] = (int)runs.size() / 3;
        if (i != n) return fail(RL_EINVAL, "row-polynomial form: rows are not sorted by output");
        if (runs.empty()) return fail(RL_EINVAL, "row-polynomial form: no rows");
        RL_TRY(s->rp_runs.upload(runs.data(), runs.size()));
        RL_TRY(s->rp_run_ptr.upload(run_ptr.data(), run_ptr.size()));
        RL_TRY(s->rp_out_end.upload(out_end.data(), out_end.size()));
        s->rp_nruns = run_ptr[D];
        s->h_run_ptr = run_ptr;
        s->h_out_end = out_end;
    }
    const size_t need = (size_t)s->rp_nruns * nvec * R;
    RL_TRY(s->rp_part.reserve(need));
    RL_TRY(lr_reserve(g, nvec));             // (the mixed coefficients live on the grid handle)
    return RL_OK;
}
// (F: the table the projection reads; the expansion computes its rows of F from the
// interpolation entries base / w4 -- all three in the row order of the batch)
template <int R>
static void rp_launch(rl_ski* s, const double* F, const int* base, const double* w4,
                      const double* Xp, double* Yp, int nvec, const double* diag, hipStream_t st,
                      const SkiCall& call) {
    rl_gridop* g = s->g;
    constexpr int NT = (R + 15) / 16;
    const size_t lds = (((size_t)16 * NT + 2 * RL_RP_VG) * RL_RP_LD + RL_RP_TILE) * sizeof(double);
    const int vblk = RL_RP_NG(R) * RL_RP_VG;
    const RpFuse& fz = call.fuse;
    // at most one block of 16 vectors and a lone last one (a rank's share of an 8-way probe
    // split): the small-batch kernel, next tile's loads in flight during the current one
    if (nvec <= RL_RP_VG + 1 && (nvec <= RL_RP_VG || nvec % RL_RP_VG == 1) && !s->kn.no_rp_small) {
        const size_t lds1 = (((size_t)16 * NT + RL_RP_VG) * RL_RP_LD + RL_RP_TILE) * sizeof(double);
        if (fz.r2 != nullptr)
            RL_LAUNCH((k_rp_project1<R, true>), dim3(s->rp_nruns), dim3(256), lds1, st, Xp,
                      s->n, nvec, F, (const int*)s->rp_runs, s->rp_part, call.bump, fz);
        else
            RL_LAUNCH((k_rp_project1<R>), dim3(s->rp_nruns), dim3(256), lds1, st, Xp, s->n,
                      nvec, F, (const int*)s->rp_runs, s->rp_part, call.bump,
                      RpFuse{nullptr, nullptr, nullptr});
    } else if (fz.r2 != nullptr) {
        const int vb = RL_RP_NG_FB(R) * RL_RP_VG;
        RL_LAUNCH((k_rp_project<R, true>),
                  dim3(8 * ((s->rp_nruns + 7) / 8) * ((nvec + vb - 1) / vb)), dim3(256), lds, st,
                  Xp, s->n, nvec, F, (const int*)s->rp_runs, s->rp_nruns, s->rp_part, call.bump, fz);
    } else {
        RL_LAUNCH((k_rp_project<R>), dim3(8 * ((s->rp_nruns + 7) / 8) * ((nvec + vblk - 1) / vblk)),
                  dim3(256), lds, st, Xp, s->n, nvec, F, (const int*)s->rp_runs, s->rp_nruns, s->rp_part,
                  call.bump, RpFuse{nullptr, nullptr, nullptr});
    }
    int split3 = 0;
    const size_t mix_lds = lr_mix_lds(g->D, R, g->Q, &split3);
    RL_LAUNCH(k_lr_mix, dim3(nvec), dim3(RL_LR_MIXT), mix_lds, st,
              (const double*)s->rp_part, 0, nvec, g->D, R, g->Q, (const double*)g->lr_C,
              (const double*)g->lr_B, (const double*)g->lr_nu, g->lr_zhat,
              (const int*)s->rp_run_ptr, split3);
    if (call.head != nullptr) minres2_head(*call.head, call.head_par, st);
    const RpPFuse& pf = call.pfuse;
    if (pf.pc != nullptr) {
        // MINRES's P inside the expansion: no operator output is written
        size_t ldsp = (size_t)nvec * 8 * sizeof(double);
#if defined(RL_EMU)
        ldsp += 256 * sizeof(double);
#endif
        RL_LAUNCH((k_rp_expand<R, true, true>), dim3((s->n + 255) / 256), dim3(256), ldsp, st,
                  (const double*)g->lr_zhat, F, s->n, nvec, g->D,
                  (const int*)s->rp_out_end, Yp, diag, Xp, s->kn.rp_stagger, base, w4, g->m,
                  (const double*)g->lr_beta, pf);
        return;
    }
    const RpPFuse nopf{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (diag != nullptr)
        RL_LAUNCH((k_rp_expand<R, true, false, true>), dim3((s->n + 255) / 256), dim3(256), 0, st,
                  (const double*)g->lr_zhat, F, s->n, nvec, g->D,
                  (const int*)s->rp_out_end, Yp, diag, Xp, s->kn.rp_stagger, base, w4, g->m,
                  (const double*)g->lr_beta, nopf);
    else
        RL_LAUNCH((k_rp_expand<R, true, false, false>), dim3((s->n + 255) / 256), dim3(256), 0, st,
                  (const double*)g->lr_zhat, F, s->n, nvec, g->D,
                  (const int*)s->rp_out_end, Yp, diag, Xp, s->kn.rp_stagger, base, w4, g->m,
                  (const double*)g->lr_beta, nopf);
}
// Do the rows of every output occupy the SAME index range in the caller's order as in the
// sorted one?  (True for W built output by output, multi_interpolant's block-diagonal layout,
// runlmc/approx/interpolation.py:161-176; false when the caller interleaves outputs.)  Only
// then do the sorted order's runs, output borders and per-output noise serve a batch in the
// caller's order; otherwise rl_ski_mvm permutes the batch (correct for any row order).
static bool caller_order_same(rl_ski* s) {
    if (s->caller_ranges_same < 0) {
        const int n = s->n, m = s->g->m;
        bool same = (int)s->terms[0].h_base.size() == n && (int)s->h_perm.size() == n;
        for (int a = 0; a < n && same;) {
            const int d = s->terms[0].h_base[a] / m;
            int b = a;
            while (b < n && s->terms[0].h_base[b] / m == d) ++b;
            for (int i = a; i < b && same; ++i) same = s->h_perm[i] >= a && s->h_perm[i] < b;
            a = b;
        }
        s->caller_ranges_same = same ? 1 : 0;
    }
    return s->caller_ranges_same == 1 && s->caller_noise_same;
}
// caller_order: the batch is in the caller's row order (F / entries permuted accordingly)
static int ski_rp_mvm(rl_ski* s, bool caller_order, const double* Xp, double* Yp, int nvec,
                      const double* diag, hipStream_t st, const SkiCall& call) {
    trace_once("K~ product: row-polynomial form (k_rp_project / k_lr_mix / k_rp_expand)");
    const double* F = caller_order ? s->rp_Fc : s->rp_F;
    const int* base = caller_order ? s->rp_base_c : s->terms[0].W4_base;
    const double* w4 = caller_order ? s->rp_w4_c : s->terms[0].W4_w;
    switch (s->g->lr_r) {
        case 24: rp_launch<24>(s, F, base, w4, Xp, Yp, nvec, diag, st, call); break;
        case 32: rp_launch<32>(s, F, base, w4, Xp, Yp, nvec, diag, st, call); break;
        case 36: rp_launch<36>(s, F, base, w4, Xp, Yp, nvec, diag, st, call); break;
        case 40: rp_launch<40>(s, F, base, w4, Xp, Yp, nvec, diag, st, call); break;
        case 48: rp_launch<48>(s, F, base, w4, Xp, Yp, nvec, diag, st, call); break;
        default: return fail(RL_EINVAL, "row-polynomial form: bad basis size");
    }
    RL_HIP(hipGetLastError());
    return RL_OK;
}
// Yp = K~ Xp, both in internal row order (what the solver iterates on); `call`: what a solver
// round asks beyond the product.  The SKI level's entry: it alone asks whether st is being captured.
int ski_mvm_int(rl_ski* s, const double* Xp, double* Yp, int nvec, hipStream_t st, const SkiCall& call) {
    RL_TRY(ski_reserve(s, nvec));
    const double* diag = s->has_noise && call.noise ? s->noise_diag.get() : nullptr;
    // (only a single-term operator on a plain grid has routes that allocate or verify)
    const bool structured = single_term(s) && !s->g->wide && !s->g->lead;
    const bool capturing = structured && stream_capturing(st);
    // (a pending form decision is taken here, so that the path does not depend on whether an
    // earlier product happened to trigger it)
    if (structured && !capturing) RL_TRY(lr_prepare(s->g, nvec));
    const SkiRoute route = ski_route(s, nvec);
    // F M F^T, no interpolation products, no grid vector (rl_rowpoly.h): its buffers are prepared
    // here outside a capture; a captured product that finds them short takes the other route
    if (route.rowpoly && !ski_ready(s, route) && !capturing) RL_TRY(rp_prepare(s, nvec));
    const bool rowpoly = route.rowpoly && ski_ready(s, route);
    // the call's request against the route: B rides in the projection, P in the expansion or the staged W
    const bool want_b = call.fuse.r2 != nullptr, want_p = call.pfuse.pc != nullptr;
    if ((want_b && !rowpoly) || (want_p && !rowpoly && !route.w_staged_p))
        return fail(RL_EINVAL, "internal: MINRES update fused into a product whose route does not run it");
    if (rowpoly) return ski_rp_mvm(s, false, Xp, Yp, nvec, diag, st, call);
    RL_TRY(ski_wt_int(s, route, Xp, s->G1, nvec, st, call.bump));
    // a polynomial-form operator hands its mixed coefficients to the W kernel instead of writing the
    // grid vector (the grid handle says whether it did) -- not when P rides in W, which reads it
    bool expansion_deferred = false;
    RL_TRY(gridop_mvm_int(s->g, s->G1, s->G2, nvec, st, route.w_poly && !want_p, &expansion_deferred));
    if (expansion_deferred) {
        RL_TRY(ski_w_poly(s, Yp, nvec, diag, Xp, st));
    } else {
        if (want_p && call.head != nullptr) minres2_head(*call.head, call.head_par, st);
        RL_TRY(ski_w_int(s, route, s->G2, Yp, nvec, diag, Xp, st, call.pfuse));
    }
    for (size_t k = 1; k < s->terms.size(); ++k) {       // Yp += W_t K_t W_t^T Xp
        const SkiTerm& t = s->terms[k];
        launch_spmv(t.WT_indptr, t.WT_indices, t.WT_data, t.ngrid, s->n, nvec, Xp, s->G1,
                    nullptr, nullptr, st);
        RL_TRY(rl_gridop_mvm(t.g, s->G1, s->G2, nvec, st));
        launch_spmv(t.W_indptr, t.W_indices, t.W_data, s->n, t.ngrid, nvec, s->G2, Yp, nullptr,
                    nullptr, st, 1);
    }
    RL_HIP(hipGetLastError());
    return RL_OK;
}

// CSR pair of term `term` (0 = the handle's first term)
static int term_view(rl_ski* s, int term, const SkiTerm** out) {
    if (term < 0 || term >= (int)s->terms.size())
        return fail(RL_EINVAL, "SKI term index out of range");
    *out = &s->terms[term];
    return RL_OK;
}

extern "C" int rl_ski_apply_wt_term(rl_ski* s, int term, const double* X, double* G, int nvec,
                                    void* stream) {
    if (!s || !X || !G) return fail(RL_EINVAL, "rl_ski_apply_wt: NULL argument");
    if (nvec <= 0) return nvec == 0 ? RL_OK : fail(RL_EINVAL, "nvec < 0");
    const SkiTerm* tp = nullptr;
    RL_TRY(term_view(s, term, &tp));
    const SkiTerm& t = *tp;
    RL_HIP(hipSetDevice(s->g->device));
    hipStream_t st = (hipStream_t)stream;
    if (s->permuted) {
        RL_TRY(ski_reserve_perm(s, nvec));
        permute_rows(s, X, s->P1, nvec, 0, st);
        X = s->P1;
    }
    launch_spmv(t.WT_indptr, t.WT_indices, t.WT_data, t.ngrid, s->n, nvec, X, G, nullptr,
                nullptr, st);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

extern "C" int rl_ski_apply_w_term(rl_ski* s, int term, const double* G, double* Y, int nvec,
                                   void* stream) {
    if (!s || !G || !Y) return fail(RL_EINVAL, "rl_ski_apply_w: NULL argument");
    if (nvec <= 0) return nvec == 0 ? RL_OK : fail(RL_EINVAL, "nvec < 0");
    const SkiTerm* tp = nullptr;
    RL_TRY(term_view(s, term, &tp));
    const SkiTerm& t = *tp;
    RL_HIP(hipSetDevice(s->g->device));
    hipStream_t st = (hipStream_t)stream;
    double* dst = Y;
    if (s->permuted) {
        RL_TRY(ski_reserve_perm(s, nvec));
        dst = s->P2;
    }
    launch_spmv(t.W_indptr, t.W_indices, t.W_data, s->n, t.ngrid, nvec, G, dst, nullptr, nullptr,
                st);
    if (s->permuted) permute_rows(s, s->P2, Y, nvec, 1, st);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

extern "C" int rl_ski_apply_wt(rl_ski* s, const double* X, double* G, int nvec, void* stream) {
    return rl_ski_apply_wt_term(s, 0, X, G, nvec, stream);
}

extern "C" int rl_ski_apply_w(rl_ski* s, const double* G, double* Y, int nvec, void* stream) {
    return rl_ski_apply_w_term(s, 0, G, Y, nvec, stream);
}

extern "C" int rl_ski_mvm(rl_ski* s, const double* X, double* Y, int nvec, void* stream) {
    if (!s || !X || !Y) return fail(RL_EINVAL, "rl_ski_mvm: NULL argument");
    if (X == Y) return fail(RL_EINVAL, "rl_ski_mvm: X and Y may not alias");
    if (nvec <= 0) return nvec == 0 ? RL_OK : fail(RL_EINVAL, "nvec < 0");
    RL_HIP(hipSetDevice(s->g->device));
    hipStream_t st = (hipStream_t)stream;
    if (!s->permuted) return ski_mvm_int(s, X, Y, nvec, st);
    // Row-polynomial form in the CALLER's row order: F's columns permuted once per rank, no
    // row permutation of the batch (they were half of this product's time at C5).  The rows of
    // an output are contiguous in both orders, so runs, output borders and the noise array
    // (constant per output) serve both.
    if (single_term(s) && !s->g->wide && !s->g->lead && !stream_capturing(st) && caller_order_same(s)) {
        RL_TRY(lr_prepare(s->g, nvec));
        if (ski_route(s, nvec).rowpoly) {
            RL_TRY(rp_prepare(s, nvec));
            if (!s->rp_base_c || !s->rp_w4_c) {
                // (a failed second allocation must not leave the first behind as a sign that
                // both exist)
                RL_TRY(s->rp_base_c.reserve((size_t)s->n));
                if (s->rp_w4_c.reserve((size_t)4 * s->n) != RL_OK) {
                    s->rp_base_c.reset();
                    return RL_EHIP;
                }
                RL_LAUNCH(k_rp_permute_entries, dim3((s->n + 255) / 256), dim3(256), 0,
                          (hipStream_t) nullptr, (const int*)s->terms[0].W4_base, (const double*)s->terms[0].W4_w,
                          (const int*)s->perm, s->n, s->rp_base_c, s->rp_w4_c);
                RL_HIP(hipGetLastError());
                RL_HIP(hipDeviceSynchronize());
            }
            if (s->rp_Fc_R != s->rp_R) {
                s->rp_Fc_R = 0;
                RL_TRY(s->rp_Fc.renew((size_t)s->rp_R * s->n));
                permute_rows(s, s->rp_F, s->rp_Fc, s->rp_R, 1, (hipStream_t) nullptr);
                RL_HIP(hipGetLastError());
                RL_HIP(hipDeviceSynchronize());
                s->rp_Fc_R = s->rp_R;
            }
            return ski_rp_mvm(s, true, X, Y, nvec, s->has_noise ? s->noise_diag.get() : nullptr, st,
                              SkiCall());
        }
    }
    RL_TRY(ski_reserve_perm(s, nvec));
    permute_rows(s, X, s->P1, nvec, 0, st);
    RL_TRY(ski_mvm_int(s, s->P1, s->P2, nvec, st));
    permute_rows(s, s->P2, Y, nvec, 1, st);
    return RL_OK;
}

