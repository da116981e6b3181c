// Host-side internals shared by the translation units of the library (round 6 split of
// runlmc_hip.hip): rl_gridop.hip (grid operator, forms), rl_ski.hip (SKI operator products),
// rl_solve.hip (Krylov and direct solves, host helpers, gradient partial sums).  Kernels come
// from the rl_*.h headers; their non-template kernels have internal linkage, so that every
// translation unit instantiates only what it launches.  Device memory of every handle lives in
// DevBuf members (below): a destroy function ends its streams, events and child handles and
// deletes the handle, whose destructor frees the buffers.
#pragma once
#include "../../include/runlmc_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "rl_kernels.h"
#include "rl_kernels2.h"
#include "rl_kernels3.h"
#include "rl_lowrank.h"
#include "rl_rowpoly.h"
#include "rl_filter.h"

#define RL_MAX_D 16

// ---------------------------------------------------------------------------
// errors (rl_gridop.hip owns the thread-local message)
// ---------------------------------------------------------------------------
int fail(int code, const std::string& msg);
#define RL_HIP(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(RL_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

#define RL_TRY(expr)              \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != RL_OK) return rc_; \
    } while (0)


// RUNLMC_TRACE=1: one line on stderr the first time each kernel variant is chosen
void trace_once(const char* what);
// true the first time a call site (its own bit mask `seen`) sees the current device
bool first_on_device(unsigned long long* seen);

// ---------------------------------------------------------------------------
// Environment switches.  Read ONCE, when a handle is created, into the handle:
// nothing a product or a solve does afterwards depends on the environment.
// What is left are (a) switches that turn a form or a fused path off for A/B
// measurements, (b) hooks the tests use to reach, at small sizes, the code paths
// that sizes select in production (chunked products, staged SpMVs, long-system
// loops).  Kernel-tuning knobs of earlier rounds (tile sizes, thread counts,
// stream counts, the round-1 kernels) are gone with the measurements that settled
// them.
// ---------------------------------------------------------------------------
struct RlKnobs {
    bool pow2_only = false;      // RUNLMC_POW2_ONLY: the reference's embedding length
    int chunk_mb = 0;            // RUNLMC_CHUNK_MB: intermediates per chunk of a batched product
    int two_streams = -1;        // RUNLMC_TWO_STREAMS=0/1 (default: by size)
    int affine = -1;             // RUNLMC_AFFINE=0/1: pair-affine order of the transform kernels
    int affine_kb = 0;           // RUNLMC_AFFINE_KB: L2-sized chunks of that many KB per XCD (experiment)
    int affine_max_kb = 2048;    // RUNLMC_AFFINE_MAX_KB: largest pair (KB of intermediates) that takes the order
    bool no_v1p = false;         // RUNLMC_NO_V1P: never the single-tile product
    int v1p_min = 0;             // RUNLMC_V1P_MIN
    bool no_lowrank = false;     // RUNLMC_NO_LOWRANK: no polynomial-subspace form
    bool no_filter = false;      // RUNLMC_NO_FILTER: no recursive-filter form
    bool sf_scan2 = false;       // RUNLMC_SF_SCAN2: the chunk chain reading the chunk states twice (k_sf_scan) on short grids too
    bool sf_carries1 = false;    // RUNLMC_SF_CARRIES1: the chunk states without the parity trick (k_sf_carries<2>)
    bool no_lr_bound = false;    // RUNLMC_NO_LR_BOUND: the polynomial verification without its operator-norm
                                 // bound (tests: what rounds 2-4 accepted)
    bool poly_round = false;     // RUNLMC_POLY_ROUND: polynomial rounds also on grids of 96..2047 points
    bool no_poly_round = false;  // RUNLMC_NO_POLY_ROUND
    long long lr_min = -1;       // RUNLMC_LR_MIN: batch gate of the structured forms
    bool staged_wt = false;      // RUNLMC_STAGED_WT: LDS-staged SpMVs whatever the size
    bool no_staged_wt = false;   // RUNLMC_NO_STAGED_WT
    bool no_w_poly = false;      // RUNLMC_NO_W_POLY: the W product reads the expanded grid vector
    bool no_rp = false;          // RUNLMC_NO_RP: no row-polynomial form of large solver rounds (rl_rowpoly.h)
    int rp_stagger = 7;          // RUNLMC_RP_STAGGER: k_rp_expand's workgroup b starts at vector (stagger b) mod nvec
    int rp_runlen = 0;           // RUNLMC_RP_RUNLEN: rows per run of k_rp_project (default: about n / 1024)
    bool no_rp_small = false;    // RUNLMC_NO_RP_SMALL: batches of <= 17 vectors through the general k_rp_project
    bool rp_pfuse = true;        // RUNLMC_NO_RP_PFUSE turns off MINRES's P inside the row-polynomial expansion
                                 // (k_minres2_ph + k_rp_expand<.., true>; rl_rowpoly.h RpPFuse): C5 round 2.30 ms
                                 // against 2.62 with P as its own kernel (profiles/r05/rp_pfuse_ab.txt, run 3)
    bool w_pfuse = true;         // RUNLMC_NO_W_PFUSE turns off MINRES's P inside the staged W product of rounds whose
                                 // operator is not in the row-polynomial form (k_spmv_w_staged_p, k_minres2_bv):
                                 // C5 matern round 3.71 ms against 4.18, mix 3.98 against 4.41
    bool no_rp_fuse = false;     // RUNLMC_NO_RP_FUSE: MINRES's B as its own kernel in row-polynomial rounds
    bool no_lr_small = false;    // RUNLMC_NO_LR_SMALL: small batches never take k_lr_small_*
    int lr_expand_plain = 0;     // RUNLMC_LR_EXPAND_PLAIN: 1 k_lr_expand whatever the row length (never
                                 // k_lr_expand_lines: A/B runs, the bit-equality tests), 2 the same with
                                 // its row blocks padded to a multiple of 8 (what k_lr_expand_lines is held against)
                                 // 3 k_lr_expand_lines also where it is not the default (rank >= 36, accumulating)
    int lr_policy = -1;          // RUNLMC_LR_POLICY: cache policy of k_lr_project's loads and k_lr_expand(_lines)'
                                 // stores and the projection's depth (rl_lowrank.h LrPolicy): bit 0 nt loads,
                                 // bits 1-2 stores plain / nt / sc1, bit 3 two rows per wave and a ring of
                                 // four at rank 24.  0: none of it, whatever the size; unset: the library's
                                 // choice by instantiation and size (lr_policy_of)
    bool no_precond_approx = false;   // RUNLMC_NO_PRECOND_APPROX: no preconditioner for operators outside the polynomial form
    long long precond_hi_min = 100000;   // RUNLMC_PRECOND_HI_MIN: rows from which an operator without a polynomial row
                                      // gets the 96-function preconditioner
    int precond_hi_use = 0;           // RUNLMC_PRECOND_HI_USE: functions of it a factorisation uses (0: the library's rule)
    int precond_hi_rank = 192;         // RUNLMC_PRECOND_HI_RANK: its basis size (whole blocks of 48)
    bool no_precond_hi_mixed = false; // RUNLMC_NO_PRECOND_HI_MIXED: ... but not operators with SOME rows in the polynomial form
    bool precond_hi_passes = false;   // RUNLMC_PRECOND_HI_PASSES: its expansion block by block through the rank-48
                                      // kernel (as first built) instead of k_hz_expand_mm's one pass (A/B)
    bool no_precond_hi = false;       // RUNLMC_NO_PRECOND_HI: operators without a polynomial row keep the 48-function
                                      // preconditioner (not the 96-function one of rl_solve.hip: hz_*)
    int w_poly_rmax = 32;        // RUNLMC_W_POLY_RMAX: largest rank whose expansion the W kernel takes over
                                 // (36 measured: 791 us against 186 + 473 for expansion + staged W per C5 round)
    bool no_sort = false;        // RUNLMC_NO_SORT: caller's data order inside the SKI handle
    long long ws_cache_mb = -1;  // RUNLMC_WS_CACHE_MB
    int solver_maxblk = 0;       // RUNLMC_SOLVER_MAXBLK
    bool no_fuse_w = false;      // RUNLMC_NO_FUSE_W
    bool no_fuse_wt = false;     // RUNLMC_NO_FUSE_WT
    bool no_graph = false;       // RUNLMC_NO_GRAPH: solver rounds launched eagerly
    bool minres_v1 = false;      // RUNLMC_MINRES_V1 (emulator build only: the four-kernel
                                 // iteration the tests hold the two-kernel rounds against)
};
// Three switches are the user's: RUNLMC_POW2_ONLY (the reference's embedding length),
// RUNLMC_WS_CACHE_MB (memory the solver keeps between calls), RUNLMC_TRACE (prints which
// kernels ran).  Every other one is an A/B or test hook and is read ONLY under
// RUNLMC_DEBUG=1 -- without it the library runs its defaults whatever the environment says
// (and names every hook it ignored on stderr, each once).
RlKnobs read_knobs();

// ---------------------------------------------------------------------------
// Device memory.  Every device buffer of a handle is a DevBuf member: the handle's
// destructor frees it, so `delete h` in a destroy function is the whole of freeing.
// reserve() never over-allocates and keeps no contents; it knows nothing about streams,
// so a product's entry function reserves outside a capture only (ski_mvm_int, mvm_with_mix).
// ---------------------------------------------------------------------------
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;     // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p; cap = o.cap;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    T* get() const { return p; }
    operator T*() const { return p; }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // at least n elements: nothing when they are there, else free and allocate exactly n
    int reserve(size_t n) { return cap >= n ? RL_OK : alloc(n * sizeof(T), n); }
    // exactly n elements whatever was there (contents are not kept)
    int renew(size_t n) { return alloc(n * sizeof(T), n); }
    // a fresh allocation holding the host array (empty input: 16 bytes / one element)
    int upload(const T* host, size_t n) {
        RL_TRY(alloc(std::max<size_t>(n * sizeof(T), 16), n));
        if (n) RL_HIP(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
        return RL_OK;
    }
    int upload(const std::vector<T>& host) {
        RL_TRY(alloc(std::max<size_t>(host.size(), 1) * sizeof(T), host.size()));
        if (!host.empty())
            RL_HIP(hipMemcpy(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
        return RL_OK;
    }
private:
    int alloc(size_t bytes, size_t n) {
        reset();
        const hipError_t e = hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(RL_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
        cap = n;
        return RL_OK;
    }
};

static const size_t kLdsSoft = 76 * 1024;    // two workgroups per CU
static const size_t kLdsHard = 156 * 1024;   // one workgroup per CU (160 KiB LDS)

// ---------------------------------------------------------------------------
// grid operator
// ---------------------------------------------------------------------------
struct rl_gridop {
    RlKnobs kn;                 // environment switches as they were when the handle was created
    int device = 0;
    int D = 0, m = 0, L = 0, N1 = 0, N2 = 0;
    Geom geo{0, 0, 0};   // m1 == 0: 1-D grid; else an m1 x m2 grid (2-D BTTB)
    int colsA = 0;   // columns per k_cols_* workgroup
    int rowsB = 0;   // rows per k_rows_mix workgroup
    int rowsS = 0;   // rows per k_rows_spec workgroup
    int code1 = 0, code2 = 0;   // fused_code(N1), fused_code(N2); both != 0 -> v2 kernels
    bool v2 = false;
    bool rows3 = false;         // row kernel = k3_rows_mix (plan2 = {RA, RB, 2})
    // polynomial-subspace form for smooth kernels (rl_lowrank.h)
    bool lr_try = false;        // eligible: 1-D grid, long enough, not switched off
    bool lr_ok = false;         // verified against the FFT path for the current parameters
    bool lr_round_try = false;  // the solver's polynomial rounds may use this grid
    // D > RL_MAX_D outputs ("wide" operator, round 4): the D x D mix does not fit the row
    // kernels' registers, so the Toeplitz blocks run through a child handle with ONE output
    // on nvec * D rows (T_q applied to every row: rl_gridop_mvm_top of the child, in
    // whatever form that top takes) and k_wide_mix applies the dense couplings,
    //   Y[v][a] (+)= sum_b B_q[a][b] (T_q X)[v][b].
    // (reference kronecker.py:39-46 has no limit on D; Q products + Q mix passes)
    // A 2-D grid with D <= RL_MAX_D whose row tile of D outputs exceeds the LDS takes the
    // same route (gridop_create_impl: rows_too_long).
    bool wide = false;
    rl_gridop* child = nullptr;
    DevBuf<double> wide_B;   // [max_tops][D][D]
    DevBuf<double> wide_Z;   // T_q X of one top: nvec * D * m
    // 3-D grid m0 x m1 x m2 (rl_lead.h): a real transform along the leading axis (k_lead_fwd),
    // one 2-D product over (m1, m2) per leading frequency f < F = N0 / 2 + 1 -- kids[f], a
    // complete 2-D operator with D outputs holding the real rows sum_j c_q[j] cos(2 pi f j / N0)
    // and the caller's couplings, applied to the real and the imaginary slab as two vectors --
    // and the inverse transform (k_lead_inv).  One stream, in order.  No structured forms.
    bool lead = false;
    int m0 = 0, N0 = 0;
    std::vector<rl_gridop*> kids;
    DevBuf<double> lead_tw;  // dev [N0 / 2][2]: exp(-2 pi i k / N0)
    DevBuf<double> lead_x, lead_y;   // [F][2][nvec][D][m1 m2] each
    size_t lead_cap = 0;        // vectors they hold
    int lr_rejects = 0;         // consecutive parameter sets with a top the verification rejected
    int lr_skip = 0;            // parameter updates the verification still sits out (back-off:
                                // 0, 1, 3 ... 31 updates after 1, 2, 3 ... rejections in a row)
    DevBuf<double> lr_stat;  // dev verdict records of the verification; lr_C lives behind them
    bool lr_dirty = false;      // parameters changed since the last verification: the
                                // set-time work (lr_setup) runs when the first batch above
                                // the gate asks for it -- small-batch users never pay it
    std::vector<double> lr_A, lr_W, lr_kap;    // the parameters lr_setup will need
    std::vector<int> lr_Qi;
    bool lr_bypass = false;     // set while the FFT path is wanted (set-time verification)
    int lr_r = 0;               // basis size in use (24 / 32 / 48)
    int lr_rank_hint = 0;       // first rank the verification tries (rl_gridop_set_rank_hint)
    size_t lr_min = 0;          // batches below this many elements stay on the FFT path
    DevBuf<double> lr_beta;  // dev [RL_LR_RMAX] recurrence coefficients
    DevBuf<double> lr_nu;    // dev [RL_LR_RMAX] normalisation
    DevBuf<double> lr_phiJ;  // dev [RL_LR_RMAX][m]
    double* lr_C = nullptr;  // dev [max_tops][r][r] (inside lr_stat's allocation)
    DevBuf<double> lr_M;     // dev [D][24][D][24]: the whole coefficient map (polynomial rounds)
    std::vector<double> lr_hC;  // host copy of lr_C for it
    DevBuf<double> lr_spart; // dev [nvec][D][nseg][r]: partial sums of k_lr_small_project
    DevBuf<double> lr_Cx;    // dev [RMAX][RMAX]: scratch of lr_all_coeffs
    DevBuf<double> lr_Mf;    // dev [D][r][D][r]: the coefficient map for k_lr_small_expand (any rank)
    bool lr_Mf_ok = false;      // ... built for the current parameters
    std::vector<double> lr_hB;  // host [Q][D][D]: the couplings lr_B holds (direct solves, rl_direct.h)
    std::vector<double> lr_hnu; // host copy of lr_nu
    unsigned long long param_ver = 0;   // bumped by every parameter update (what a factorisation was built for)
    DevBuf<double> lr_B;     // dev [max_tops][D][D]
    DevBuf<double> lr_eye;   // dev [D][D]
    DevBuf<double> lr_part;  // projection partial sums
    DevBuf<double> lr_zhat;  // mixed coefficients [rows][r]
    DevBuf<double> lr_scr;   // set-time scratch: 3 vectors of D*m + partial maxima
    DevBuf<double> lr_pw;    // the power iteration's vectors (lr_verify (iv))
    DevBuf<double> lr_sel;   // ... and the selector couplings of its groups of tops
    std::vector<double> lr_vstat;   // host [max_tops][4]: the last verification's measurements per top
                                    // (trial ratio, tail ratio, ||E v||, ||T w||: rl_gridop_form_stats)
    DevBuf<double> lr_Cc;    // dev [max_tops][r][r]: C of the polynomial tops only, contiguous
    DevBuf<double> lr_Bc;    // dev [max_tops][D][D]: their couplings (operators that mix forms)
    int lr_np = 0;              // polynomial tops among the Q
    // per-top forms (decided by forms_setup at every parameter update):
    //   0 transform kernels, 1 polynomial-subspace form, 2 recursive filter (rl_filter.h)
    std::vector<double> h_tops;     // host copy of the top rows [Q][m] (every grid, every set_* path)
    std::vector<double> pc_hB;      // host [Q][D][D]: the dense couplings of the current parameters (every grid;
                                    // the pivoted-Cholesky preconditioner's diagonal, rl_pivchol.h)
    unsigned long long pc_ver = 0;  // bumped with them (param_ver does not move on a wide handle)
    std::vector<int> top_form;
    bool st_ok = false;         // every top is 1 or 2 and at least one is 2: the operator runs as
                                // polynomial part + filter part, nothing through the transforms
    bool sf_try = false;        // eligible for the filter form: 1-D grid, not switched off
    int sf_n = 0;               // filter tops
    int sf_nfac = 0;            // rank-one factors that belong to them
    int sf_ns = 2;              // states per direction the operator's filters need (2, 3 or 4)
    std::vector<int> sf_slot;   // per top: its place among the filter tops, or -1
    std::vector<int> sf_top_ns; // per top: 2, 3 or 4
    DevBuf<SfTop> sf_tops;   // dev [max_tops]
    DevBuf<double> sf_pwp;   // dev [max_tops][2 G]: the chunk states' parity weights (k_sf_carries2)
    DevBuf<double> sf_blob;  // dev: the filter part's block for k_sf_apply (rl_filter.h)
    DevBuf<double> sf_blob_top;  // dev [max_tops][...]: the same for each top alone (B = I)
    DevBuf<double> sf_pw;    // dev [max_tops][G + 1]
    DevBuf<double> sf_kappa; // dev [max_tops][D]
    DevBuf<double> sf_facA;  // dev [max_fac][D]
    DevBuf<double> sf_facAW; // dev [max_fac][D]
    DevBuf<int> sf_facJ;     // dev [max_fac]
    DevBuf<double> sf_E;     // chunk states [nchunks][rows][NF][2][NS]
    DevBuf<double> sf_Cin;   // incoming states [nchunks][nvec][nchan][2][NS]
    DevBuf<int> sf_next;     // k_sf_apply's tile counter (zeroed by k_sf_scan)
    DevBuf<double> mixtab;   // dev [D + nfac][L]: dc rows then gs rows (k_mix_tables)
    size_t mixtab_rows = 0;     // rows allocated
    bool mixtab_ok = false;     // tables match the current parameters
    int max_tops = 0;
    FftPlan plan1, plan2;
    DevBuf<cplx> tw1, tw2, twlo, twhi;
    DevBuf<int> freq1;
    TwiddleL twl;
    std::vector<int> h_freq1, h_freq2;
    // parameters
    int Q = 0, nfac = 0;
    DevBuf<double> tops;    // dev [max_tops][m]
    DevBuf<double> spec;    // dev [max_tops][L]
    DevBuf<double> facA;    // dev [max_fac][D]
    DevBuf<double> facW;    // dev [max_fac]
    DevBuf<int> facQ;       // dev [max_fac]
    DevBuf<double> kappa;   // dev [max_tops][D]
    DevBuf<double> ones;    // dev [D]  (identity mix for mvm_top)
    int max_fac = 0;
    // workspace: packed intermediates [pairs][D][L] complex
    DevBuf<cplx> T;
    size_t T_pairs = 0;
    // a second chunk of intermediates and a side stream: consecutive chunks of a
    // large batched product run on two streams, so that one chunk's kernels fill
    // the compute units another chunk's tail leaves idle
    DevBuf<cplx> T2[3];         // workspaces of the side streams
    size_t T2_pairs = 0;
    int nside = 0;              // side streams prepared (product runs on 1 + nside streams)
    cplx* Tcur = nullptr;       // workspace of the chunk being launched
    hipStream_t aux[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    size_t chunk_pairs = 1;
    bool affine = false;        // pair-affine order of the three transform kernels (rl_kernels2.h)
    // single-tile product (k1_product): grids short enough that all D transforms
    // of a pair fit one LDS tile
    bool v1p = false;
    FftPlan planL;
    DevBuf<cplx> twL;       // exp(-2 pi i k / L)
    DevBuf<double> spec1;   // dev [max_tops][L], scrambled order of the single-level transform
    size_t lds1 = 0;
    int thr1 = 256;
    int v1p_min = 64;          // vectors from which the single-tile product is used
};

// ---------------------------------------------------------------------------
// SKI operator
// ---------------------------------------------------------------------------
// one W K_UU W^T term of the operator (kernels that share an
// active-dimension set share a grid, hence a term)
struct SkiTerm {
    rl_gridop* g = nullptr;
    int ngrid = 0;
    DevBuf<int> W_indptr, W_indices;
    DevBuf<double> W_data;
    DevBuf<int> WT_indptr, WT_indices;
    DevBuf<double> WT_data;
    int nnzWT = 0;
    // Interpolation structure, when W has it (every row at most 4 entries in
    // consecutive columns, rows sorted by first column -- cubic interpolation of
    // sorted inputs): W as base column + 4 weights per row, and W^T rebuilt so
    // that the data rows of every grid row are one CONSECUTIVE range starting
    // at WT_lo[r] (zero weights kept).  Both remove one level of dependent
    // loads from the fused products of the small-batch solver.
    DevBuf<int> W4_base;
    DevBuf<double> W4_w;
    DevBuf<int> WT_lo;
    // largest data range / entry count of any RL_THREADS consecutive grid rows
    // (k_spmv_wt_staged stages them in LDS); 0 = no structure
    int wt_xmax = 0, wt_emax = 0;
    int w_xmax = 0;            // largest grid range of RL_THREADS consecutive data rows
    std::vector<int> h_base;   // host copy of W4_base (row blocks per output, polynomial rounds)
};

// Pivoted-Cholesky preconditioner P = L L^T + E of a handle (rl_pivchol.h; rl_solve.hip pc_*):
// opt-in (rank > 0), built where the polynomial factorisation is not available, cached by the
// parameter versions of ALL the handle's grids and the noise version, internal row order.
struct PcState {
    int rank = 0;                       // requested (0: off)
    double rel_tol = 1e-10;
    bool valid = false;                 // built for the versions below
    bool active = false;                // the factorisation the last dz_ensure settled on is this one (mode 4)
    unsigned long long param_sum = 0, noise_ver = 0;
    int k = 0, kp = 0;                  // rank clipped to n; rounded up to 16 (rows of L)
    int rank_used = 0;                  // columns before the first zero column (less what the sample map dropped)
    double logdet = 0.0, cond = 0.0;    // log det P; squared pivot ratio of chol(G)
    std::vector<int> h_piv;             // host [k]
    std::vector<double> h_pivval;       // host [k]
    DevBuf<double> L;                // dev [kp][n]
    DevBuf<double> d, row, e;   // dev [n]: residual diagonal, K e_p, one-hot vector
    DevBuf<int> mark;                // dev [n]: 1 on rows that were pivots
    DevBuf<int> piv;                 // dev [RL_PC_MAXRANK]
    DevBuf<double> pivval;           // dev [RL_PC_MAXRANK + 1]: d at the pivots, then max d^(0)
    DevBuf<double> pv;               // dev [RL_PC_NBLK]: arg-max partials
    DevBuf<int> pi;
    DevBuf<double> inv, isq, sq;   // dev [n]: 1 / eps, 1 / sqrt(eps), sqrt(eps)
    unsigned long long eps_ver = ~0ull;
    double sum_log_eps = 0.0;
    DevBuf<double> Mt, Mst;   // dev [kp][kp]: -G^-1 and the sample map, transposed
    bool sample_ok = false;
    DevBuf<double> part;             // dev [chunks][nvp][kp]: k_pc_project's partial sums
    DevBuf<double> cT;               // dev [kp][nvp]
    std::vector<DevBuf<double>> tops;   // dev, per term: top rows [Q][m] where the grid keeps none
    std::vector<DevBuf<double>> B;      // dev, per term: couplings [Q][D][D]
    double build_ms[4] = {0, 0, 0, 0};  // last build: diagonal / products / step kernels / Gram + host
};

// buffers of one rl_solve_batch call: a plain view of pointers, copied into launch closures
struct SolverWork {
    double* vec[10] = {nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr};
    double* S[2] = {nullptr, nullptr};
    int* I = nullptr;
    double* part[4] = {nullptr, nullptr, nullptr, nullptr};
    int* count = nullptr;   // [0] active systems, [1] global iteration counter, [2] done blocks
    double* resid = nullptr; // [nrhs] explicit residual norms
    double* lanczos = nullptr;  // rl_ski::lanczos_buf
};
// ... and their owner: a solve's local (rl_solve.hip SolverWorkGuard), or the handle between solves
struct SolverBufs {
    DevBuf<double> vec[10], S[2], part[4], resid;
    DevBuf<int> I, count;
    SolverWork view() const {
        SolverWork w;
        for (int i = 0; i < 10; ++i) w.vec[i] = vec[i];
        for (int i = 0; i < 2; ++i) w.S[i] = S[i];
        for (int i = 0; i < 4; ++i) w.part[i] = part[i];
        w.I = I; w.count = count; w.resid = resid;
        return w;
    }
};

struct rl_ski {
    RlKnobs kn;         // environment switches as they were when the handle was created
    // Lanczos coefficients of a solve: kept between calls (a hipMalloc / hipFree
    // pair per solve costs ~200 us, as much as four C2 solver rounds)
    DevBuf<double> lanczos_buf;
    int device = 0;     // copy of g->device: the grid operator may be gone at destroy time
    std::vector<SkiTerm> terms;   // terms[0]: the term of rl_ski_create, on g; then rl_ski_add_term's
    int max_ngrid = 0;
    rl_gridop* g = nullptr;
    int n = 0, ngrid = 0, nnz = 0;
    DevBuf<double> noise_diag;   // dev [n]
    bool has_noise = false;
    DevBuf<double> G1, G2;   // dev [cap][D*m] grid-side temporaries
    int cap = 0;
    // Internal row order: data points sorted by grid position (W, WT and
    // noise_diag above are stored in THAT order); perm[i] = caller's row of
    // internal row i.  P1/P2: dev [pcap][n] staging for caller-order entry points.
    // polynomial rounds of small solves (rl_solver.h, Minres2Bufs::poly_part): row
    // blocks that lie inside one output, first block of each output, partial sums
    DevBuf<int> poly_tab, poly_ob;
    int poly_nblk = 0;              // 0: not built yet, -1: not applicable
    DevBuf<double> poly_part;
    // row-polynomial form of large solver rounds (rl_rowpoly.h): F = W Phi, built per rank
    DevBuf<double> rp_F;
    int rp_R = 0;                   // rank F was built for (0: none)
    DevBuf<double> rp_Fc;        // the same in the CALLER's row order (rl_ski_mvm: no row permutations)
    int rp_Fc_R = 0;
    DevBuf<int> rp_base_c;       // interpolation entries in the caller's row order (k_rp_expand computes F from them)
    DevBuf<double> rp_w4_c;
    DevBuf<int> rp_runs, rp_run_ptr, rp_out_end;
    int rp_nruns = 0;
    DevBuf<double> rp_part;
    DevBuf<double> rp_nrm;       // fused B: [nrhs] coefficients + [nrhs][rp_nruns] partial norms
    // MINRES's P inside the expansion or the staged W product (SkiCall::pfuse): the head's
    // coefficients [nrhs][RL_RP_PCW] and three arrays of [nrhs][ceil(n / 256)] partial sums
    DevBuf<double> rp_pp;
    std::vector<int> eps_end;       // noise in runs: rows [eps_end[k-1], eps_end[k]) carry eps_val[k]
    std::vector<double> eps_val;    // (empty: more than RL_MAX_D runs)
    bool permuted = false;
    DevBuf<int> perm;
    std::vector<int> h_perm;
    // rl_ski_mvm's row-polynomial form in the CALLER's row order reuses the runs, the output
    // borders and the noise array of the SORTED order: valid only when every output's rows
    // occupy the same range in both orders (checked once on the host, caller_order_same) and
    // the noise array reads the same in both (rl_ski_set_noise).  -1: not checked yet
    int caller_ranges_same = -1;
    bool caller_noise_same = true;
    DevBuf<double> P1, P2;
    int pcap = 0;
    hipStream_t solver_stream = nullptr;   // capturable stream of rl_solve_batch
    int* pin_count = nullptr;              // pinned host [2]: active-system counts in flight
    hipEvent_t count_ev[2] = {nullptr, nullptr};
    // the solver's buffers are kept between calls (a solve frees eighteen of them
    // and a hipFree is ~100 us: 1.7 of the 2.9 ms a C2 solve spent outside its
    // rounds); capacities in elements.  RUNLMC_WS_CACHE_MB bounds what is kept.
    SolverBufs ws;
    bool ws_valid = false;
    size_t ws_vec_cap = 0, ws_rhs_cap = 0, ws_part_cap = 0;
    // direct solves through the polynomial form (rl_direct.h): K~ = F M F^T + E
    unsigned long long noise_ver = 0;   // bumped by rl_ski_set_noise
    std::vector<double> h_noise;        // host copy of noise_diag (internal row order)
    std::vector<int> h_run_ptr, h_out_end;   // host copies of rp_run_ptr / rp_out_end
    std::vector<double> dz_U;           // host [D][r][r]: F_d^T F_d on the unnormalised q_j, per (handle, rank)
    int dz_U_R = 0;
    DevBuf<double> dz_Zt;            // dev [D r][D r]: the solve map, scalings folded in
    DevBuf<double> dz_inv;           // dev [n]: 1 / eps per row
    std::vector<double> dz_eps;         // host [D]: the noise level of each output ...
    const char* dz_eps_why = nullptr;   // ... or why there is none (not constant per output, not positive)
    unsigned long long dz_eps_ver = ~0ull;   // noise_ver those (and dz_inv) were derived from
    bool dz_valid = false;              // ... for the parameters / noise of the versions below
    bool dz_exact = false;              // every top row in the polynomial form: the factorisation IS K~^-1;
                                        // else it inverts the operator's projection on the subspace: a preconditioner
    const char* dz_fail_why = nullptr;  // "not available" decided for the versions below (not recomputed per solve)
    unsigned long long dz_fail_param_ver = 0, dz_fail_noise_ver = 0;
    int dz_fail_streak = 0, dz_fail_skip = 0;   // back-off of the attempts after failures in a row
    DevBuf<double> dz_p, dz_q;       // dev [cap][n]: PCG's direction and operator product
    size_t dz_pq_cap = 0;
    DevBuf<double> dz_scal;          // dev [cap][2]: PCG's (rho, rho_prev); a capacity of
                                     // its own (rl_solve_direct grows dz_part / dz_go without it)
    unsigned long long dz_param_ver = 0, dz_noise_ver = 0;
    int dz_R = 0;
    // the 96-function preconditioner of an operator without a polynomial row (rl_solve.hip: hz_*)
    bool dz_want_sample = false;        // rl_ski_precond_sample was called: factorisations keep the square-root map
    DevBuf<double> dz_Zh;            // dev [D r][D r]: that map, transposed (rl_solve.hip dz_host_map)
    bool dz_Zh_valid = false;
    DevBuf<double> dz_isq;           // dev [n]: 1 / sqrt(eps) per row
    unsigned long long dz_isq_ver = ~0ull;
    DevBuf<double> dz_smp;           // dev [cap][n]: scaled probes
    DevBuf<double> dz_rec;           // dev [cap][nrhs][2]: conjugate gradients' scalars of a recorded run
    bool dz_hz = false;                 // the valid factorisation is THAT one (dz_Zt: [D 96][D 96])
    int hz_R = 0;                       // its basis size (blocks of 48; "96" below stands for it)
    bool hz_traced = false;
    int hz_Ruse = 0;                    // ... of which the current factorisation uses the first hz_Ruse
    bool hz_basis_tried = false;        // basis generated (or found unusable) once per handle
    const char* hz_why = nullptr;       // why the handle has none (decided once)
    std::vector<double> hz_hnu;         // host [96]: normalisation of the basis
    DevBuf<double> hz_beta;          // dev [96]: recurrence coefficients
    DevBuf<double> hz_phi;           // dev [96 rounded up to D][m]: the functions on the grid
    DevBuf<double> hz_tphi;          // dev, same size: a top row applied to them
    DevBuf<double> hz_C;             // dev [96][96]
    DevBuf<double> hz_F;             // dev [96][n]: F = W Phi, unnormalised, degree-major
    DevBuf<double> hz_ones;          // dev [n]
    std::vector<double> hz_U;           // host [D][96][96]: F_d^T F_d, once per handle
    DevBuf<double> hz_part;          // dev [2][runs][cap][48]
    DevBuf<double> hz_zhat;          // dev [2][cap][D][48]
    DevBuf<double> hz_tmp;           // dev [cap][n]: the first half's expansion
    DevBuf<double> hz_S;             // dev [cap][D R]: projections summed over the runs
    DevBuf<double> hz_P;             // dev [RL_HZ_FS][cap][D R]: the map's partial products
    size_t hz_vec_cap = 0;
    double dz_logdet = 0.0;             // log det K~ of that factorisation
    double dz_cond = 0.0;               // ratio of the largest to the smallest pivot of chol(S), squared
    DevBuf<double> dz_res, dz_cor;   // dev [cap][n]: residuals, corrections
    size_t dz_vec_cap = 0;
    DevBuf<double> dz_part;          // dev [cap][RL_DZ_NBLK] partial sums, then [cap] norms
    DevBuf<int> dz_go;               // dev [cap]: systems still being refined
    size_t dz_rhs_cap = 0;
    PcState pc;                         // the pivoted-Cholesky preconditioner (rl_ski_set_pivchol)
    // per-observation noise (rl_rownoise.h): the factorisation of a handle whose noise came from
    // rl_ski_set_noise_rows runs on the unit-noise problem of the scaled table F~ = diag(e^-1/2) F
    bool row_noise = false;             // the noise is rl_ski_set_noise_rows' (rl_ski_set_noise clears it)
    bool dz_rows = false;               // the valid factorisation (dz_Zt, dz_logdet) is of that scaled form
    DevBuf<double> rn_isq, rn_sq, rn_inv, rn_one;   // dev [n]: e^-1/2, e^1/2, 1 / e, ones (internal row order)
    double rn_sumlog = 0.0;             // sum_i log e_i, rows in internal order
    const char* rn_why = nullptr;       // why those do not exist (a noise that is not positive)
    unsigned long long rn_ver = ~0ull;  // noise_ver they were derived from
    DevBuf<double> rn_F;                // dev [R][n]: F~, degree-major like rp_F (which stays unscaled)
    int rn_F_R = 0;
    unsigned long long rn_F_ver = ~0ull;
    std::vector<double> rn_U;           // host [D][R][R]: F~_d^T F~_d, per noise update (dz_U stays F's)
    DevBuf<double> rn_tmp;              // dev [cap][n]: the scaled input of an apply
};

inline bool single_term(const rl_ski* s) { return s->terms.size() == 1; }

// destroys a half-built handle on every early return of a create function
template <class H, int (*Destroy)(H*)>
struct HandleGuard {
    H* h;
    explicit HandleGuard(H* h_) : h(h_) {}
    ~HandleGuard() { if (h) (void)Destroy(h); }
    H* release() { H* r = h; h = nullptr; return r; }
};

// ---------------------------------------------------------------------------
// Routes: which kernels a product runs and the buffers they need, decided by ONE function per
// level (const, no HIP call) that the product, the preparation before a capture and the solver's
// choice of fusions all ask.  Nothing is allocated inside a capture: a level's entry function
// (mvm_with_mix, ski_mvm_int) asks the stream once, reserves outside a capture and inside one
// takes the route only if its buffers are there, else the fallback (DESIGN.md sections 6, 11).
// ---------------------------------------------------------------------------
enum GridForm { GRID_TRANSFORM, GRID_K1, GRID_POLY, GRID_FILTER /* one top */,
                GRID_FILTER_POLY /* all rows: filter part + polynomial part */, GRID_POLY_SMALL };
struct GridRoute {
    GridForm form = GRID_TRANSFORM;
    GridForm fallback = GRID_TRANSFORM;     // unverified parameters, or buffers short in a capture
    bool deferrable = false;                // GRID_POLY: the W kernel may take the expansion over
    size_t lr_part = 0, lr_zhat = 0, sf_E = 0, sf_Cin = 0, lr_spart = 0;    // elements needed
};
GridRoute grid_route(const rl_gridop* g, int q, int nvec);      // (q: one top row, or -1: all rows)
struct SkiRoute {
    bool rowpoly = false;       // F M F^T (rl_rowpoly.h); otherwise W^T, grid product, W:
    bool w_poly = false;        // the grid product may leave its expansion to k_spmv_w_poly
    bool wt_staged = false, w_staged = false;   // k_spmv_wt_staged / k_spmv_w_staged (else CSR)
    bool w_staged_p = false;    // k_spmv_w_staged_p may carry MINRES's P
    bool grid_poly = false;     // the grid operator is wholly in the (verified) polynomial form
    int rank = 0;               // rowpoly: basis size, partial sums per run, mixed coefficients
    size_t rp_part_per_run = 0, lr_zhat = 0;
};
SkiRoute ski_route(const rl_ski* s, int nvec);
bool ski_ready(const rl_ski* s, const SkiRoute& r);
// What the caller of ONE K~ product asks for beyond it (default: nothing).  The solver's rounds
// ride inside the product's kernels (rl_rowpoly.h): B in the projection (fuse), P in the expansion
// or the staged W product (pfuse), its scalar head launched from `head` just before that kernel.
struct Minres2Bufs;
struct SkiCall {
    RpFuse fuse{nullptr, nullptr, nullptr};
    RpPFuse pfuse{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const Minres2Bufs* head = nullptr;     // (stays where the solver keeps it) ...
    int head_par = 0;                      // ... and the round's parity
    int* bump = nullptr;                   // the solver's round counter (first kernel bumps it)
    bool noise = true;                     // false: W K_UU W^T x only, the caller adds eps (.) x
};

// ---------------------------------------------------------------------------
// functions one translation unit defines and another calls
// ---------------------------------------------------------------------------
// rl_gridop.hip
bool stream_capturing(hipStream_t stream);
int lr_ensure(rl_gridop* g);
int lr_prepare(rl_gridop* g, int nvec);
int lr_reserve(rl_gridop* g, int nvec);
int gridop_prepare(rl_gridop* g, int nvec);
// (rl_gridop_mvm + the W kernel's offer to expand lr_zhat itself; *expansion_deferred: taken)
int gridop_mvm_int(rl_gridop* g, const double* X, double* Y, int nvec, hipStream_t stream,
                   bool allow_deferred_expand, bool* expansion_deferred);
int lr_all_coeffs(rl_gridop* g, int R, std::vector<double>* hC, std::vector<char>* exact,
                  std::vector<double>* captured);
// (one chunk of a batched product on the transform kernels, optionally gathering W^T x itself:
// the solver's fused rounds call them directly)
int mvm_chunk_v2(rl_gridop* g, const MixParams& mp, const double* Xc, double* Yc, int nv, size_t pairs,
                 hipStream_t st, const Gather* gather = nullptr, int* bump = nullptr,
                 cplx* Tbuf = nullptr);
int mvm_chunk_v1(rl_gridop* g, const MixParams& mp, const double* Xc, double* Yc, int nv, size_t pairs,
                 hipStream_t stream, const Gather* gather = nullptr, int* bump = nullptr);
// rl_ski.hip
int ski_reserve(rl_ski* s, int nvec);
int ski_wt_int(rl_ski* s, const SkiRoute& route, const double* Xp, double* G, int nvec, hipStream_t st,
               int* bump = nullptr);
int ski_reserve_perm(rl_ski* s, int nvec);
void permute_rows(rl_ski* s, const double* X, double* Y, int nvec, int scatter, hipStream_t st);
int rp_prepare(rl_ski* s, int nvec);
int ski_mvm_int(rl_ski* s, const double* Xp, double* Yp, int nvec, hipStream_t st,
                const SkiCall& call = SkiCall());
// rl_solve.hip (the one call UP from rl_ski.hip into the solver's unit: SkiCall::head, k_minres2_ph)
void minres2_head(const Minres2Bufs& mb, int par, hipStream_t st);
