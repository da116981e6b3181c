// Lifecycle walk of every handle of the C ABI on the emulator library: create, grow, update,
// solve, destroy -- at the smallest shapes that still reach each path.  The program checks
// statuses (and two bit-equalities), not numbers; what it is FOR is a sanitizer run, where the
// handles' device memory is host memory and every buffer a handle forgets to free, frees twice
// or uses after a reallocation is reported:
//
//     python -m runlmc_amd.build --emu --asan
//     g++ -std=c++17 -g -fsanitize=address,undefined -Iinclude tests/emu/lifecycle_main.cpp
//         -o /tmp/lifecycle -Ltests/emu -lrunlmc_emu_asan -Wl,-rpath,$PWD/tests/emu -pthread
//     /tmp/lifecycle
//
// (a stand-alone executable: nothing is preloaded.  ASan's warning about swapcontext -- the
// emulator's fibers -- is not a finding.)  Required: exit status 0 and no report.
// tests/test_lifecycle_emu.py runs the same program against the plain emulator library.
// On the emulator a device pointer is a host pointer, so plain vectors serve as device arrays.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "runlmc_hip.h"

static int g_bad = 0;
#define EXPECT(call, want)                                                                  \
    do {                                                                                    \
        const int rc_ = (call);                                                             \
        if (rc_ != (want)) {                                                                \
            std::printf("%s:%d: %s returned %d, expected %d (%s)\n", __FILE__, __LINE__,    \
                        #call, rc_, (int)(want), rl_last_error());                          \
            ++g_bad;                                                                        \
        }                                                                                   \
    } while (0)
#define OK(call) EXPECT(call, RL_OK)
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond);            \
            ++g_bad;                                                                        \
        }                                                                                   \
    } while (0)

typedef std::vector<double> vec;

// top rows on a unit-length grid of m points
static vec rbf_row(int m, double ell) {
    vec t(m);
    for (int i = 0; i < m; ++i) t[i] = std::exp(-0.5 * std::pow(i / (m - 1.0) / ell, 2));
    return t;
}
static vec exp_row(int m, double ell) {
    vec t(m);
    for (int i = 0; i < m; ++i) t[i] = std::exp(-i / (m - 1.0) / ell);
    return t;
}
static vec matern32_row(int m, double ell) {
    vec t(m);
    for (int i = 0; i < m; ++i) {
        const double s = std::sqrt(3.0) * i / (m - 1.0) / ell;
        t[i] = (1.0 + s) * std::exp(-s);
    }
    return t;
}
static vec concat(const vec& a, const vec& b) {
    vec r(a);
    r.insert(r.end(), b.begin(), b.end());
    return r;
}
// Q symmetric positive definite D x D couplings
static vec couplings(int Q, int D, double off) {
    vec B((size_t)Q * D * D, 0.0);
    for (int q = 0; q < Q; ++q)
        for (int a = 0; a < D; ++a)
            for (int b = 0; b < D; ++b) B[((size_t)q * D + a) * D + b] = a == b ? 1.0 + 0.1 * q : off;
    return B;
}
static vec ramp(size_t len, double scale) {
    vec x(len);
    for (size_t i = 0; i < len; ++i) x[i] = scale * std::sin(0.37 * (double)i + 0.2);
    return x;
}

// cubic-convolution interpolation of n rows (outputs one after another, sorted within an output)
// on D blocks of m grid points, and its transpose
struct Interp {
    int n = 0, ngrid = 0;
    std::vector<int> ptr, idx, tptr, tidx;
    vec val, tval;
};
static Interp interp(int n, int D, int m) {
    Interp w;
    w.n = n;
    w.ngrid = D * m;
    w.ptr.push_back(0);
    const int per = n / D;
    for (int i = 0; i < n; ++i) {
        const int d = std::min(i / per, D - 1), k = i - d * per, cnt = d == D - 1 ? n - d * per : per;
        const double x = 1.0 + (k + 0.37) / cnt * (m - 3.0);
        const int b = std::min((int)x - 1, m - 4);
        const double s = x - (b + 1);
        const double wt[4] = {((-0.5 * s + 1.0) * s - 0.5) * s, (1.5 * s - 2.5) * s * s + 1.0,
                              ((-1.5 * s + 2.0) * s + 0.5) * s, (0.5 * s - 0.5) * s * s};
        for (int j = 0; j < 4; ++j) {
            w.idx.push_back(d * m + b + j);
            w.val.push_back(wt[j]);
        }
        w.ptr.push_back((int)w.idx.size());
    }
    w.tptr.assign(w.ngrid + 1, 0);
    for (int c : w.idx) ++w.tptr[c + 1];
    for (int r = 0; r < w.ngrid; ++r) w.tptr[r + 1] += w.tptr[r];
    w.tidx.resize(w.idx.size());
    w.tval.resize(w.idx.size());
    std::vector<int> at(w.tptr.begin(), w.tptr.end() - 1);
    for (int i = 0; i < n; ++i)
        for (int k = w.ptr[i]; k < w.ptr[i + 1]; ++k) {
            w.tidx[at[w.idx[k]]] = i;
            w.tval[at[w.idx[k]]++] = w.val[k];
        }
    return w;
}
static int ski_create(rl_gridop* g, const Interp& w, rl_ski** out) {
    return rl_ski_create(g, w.n, w.ptr.data(), w.idx.data(), w.val.data(), w.tptr.data(), w.tidx.data(),
                         w.tval.data(), out);
}

static void create_destroy() {
    rl_gridop* g = nullptr;
    OK(rl_gridop_create(0, 2, 128, 2, &g));
    OK(rl_gridop_destroy(g));
    OK(rl_gridop_create_2d(0, 2, 8, 8, 2, &g));
    OK(rl_gridop_destroy(g));
    OK(rl_gridop_create_3d(0, 2, 5, 6, 7, 2, &g));          // a child per leading frequency
    OK(rl_gridop_destroy(g));
    OK(rl_gridop_create(0, 17, 64, 2, &g));                 // wide: a one-output child
    OK(rl_gridop_destroy(g));
    g = nullptr;
    EXPECT(rl_gridop_create_2d(0, 2, 4096, 8, 2, &g), RL_ELIMIT);
    CHECK(g == nullptr);
    OK(rl_gridop_destroy(nullptr));
}

// grow, no shrink, a parameter update, and the same bits as a fresh handle
static void gridop_walk() {
    const int D = 2, m = 128, Q = 2;
    const vec tops1 = concat(rbf_row(m, 0.8), exp_row(m, 0.3)), B1 = couplings(Q, D, 0.3);
    const vec tops2 = concat(rbf_row(m, 0.6), exp_row(m, 0.5)), B2 = couplings(Q, D, -0.2);
    const vec X = ramp((size_t)40 * D * m, 1.0);
    vec Y((size_t)40 * D * m), Yf((size_t)3 * D * m);
    rl_gridop *g = nullptr, *f = nullptr;
    OK(rl_gridop_create(0, D, m, Q, &g));
    OK(rl_gridop_set_form_gate(g, 1));
    OK(rl_gridop_set_dense(g, Q, tops1.data(), B1.data()));
    for (int nvec : {1, 40, 3}) OK(rl_gridop_mvm(g, X.data(), Y.data(), nvec, nullptr));
    OK(rl_gridop_set_dense(g, Q, tops2.data(), B2.data()));
    OK(rl_gridop_mvm(g, X.data(), Y.data(), 3, nullptr));
    OK(rl_gridop_create(0, D, m, Q, &f));
    OK(rl_gridop_set_form_gate(f, 1));
    OK(rl_gridop_set_dense(f, Q, tops2.data(), B2.data()));
    OK(rl_gridop_mvm(f, X.data(), Yf.data(), 3, nullptr));
    CHECK(std::memcmp(Y.data(), Yf.data(), Yf.size() * sizeof(double)) == 0);
    OK(rl_gridop_destroy(f));
    OK(rl_gridop_destroy(g));
}

// two terms on grids of different lengths; destroyed before its grid operators
static void ski_two_terms() {
    const int D = 2, n = 300, mA = 128, mB = 160;
    const Interp wA = interp(n, D, mA), wB = interp(n, D, mB);
    rl_gridop *gA = nullptr, *gB = nullptr;
    rl_ski* s = nullptr;
    OK(rl_gridop_create(0, D, mA, 2, &gA));
    OK(rl_gridop_create(0, D, mB, 1, &gB));
    const vec topsA = concat(rbf_row(mA, 0.8), exp_row(mA, 0.3)), BA = couplings(2, D, 0.3);
    const vec topsB = matern32_row(mB, 0.2), BB = couplings(1, D, 0.1);
    OK(rl_gridop_set_dense(gA, 2, topsA.data(), BA.data()));
    OK(rl_gridop_set_dense(gB, 1, topsB.data(), BB.data()));
    OK(ski_create(gA, wA, &s));
    const double noise[2] = {0.1, 0.2};
    const int lens[2] = {150, 150};
    OK(rl_ski_set_noise(s, noise, lens));
    const vec X = ramp((size_t)20 * n, 1.0);
    vec Y((size_t)20 * n), G((size_t)D * mB);
    OK(rl_ski_mvm(s, X.data(), Y.data(), 1, nullptr));
    OK(rl_ski_add_term(s, gB, wB.ptr.data(), wB.idx.data(), wB.val.data(), wB.tptr.data(), wB.tidx.data(),
                       wB.tval.data()));                    // a longer grid: the grid-side temporaries grow
    std::vector<int> bad(wB.idx);
    bad[7] = wB.ngrid;
    EXPECT(rl_ski_add_term(s, gB, wB.ptr.data(), bad.data(), wB.val.data(), wB.tptr.data(), wB.tidx.data(),
                           wB.tval.data()), RL_EINVAL);
    OK(rl_ski_apply_wt_term(s, 1, X.data(), G.data(), 1, nullptr));
    EXPECT(rl_ski_apply_wt_term(s, 2, X.data(), G.data(), 1, nullptr), RL_EINVAL);   // still two terms
    for (int nvec : {1, 20, 2}) OK(rl_ski_mvm(s, X.data(), Y.data(), nvec, nullptr));
    OK(rl_ski_destroy(s));
    OK(rl_gridop_destroy(gA));
    OK(rl_gridop_destroy(gB));
}

// the solvers of a one-term handle; its grid operator is destroyed FIRST
static void ski_solves() {
    const int D = 2, n = 300, m = 128;
    const Interp w = interp(n, D, m);
    rl_gridop* g = nullptr;
    rl_ski* s = nullptr;
    OK(rl_gridop_create(0, D, m, 2, &g));
    const vec tops = concat(rbf_row(m, 0.8), exp_row(m, 0.3)), B = couplings(2, D, 0.3);
    OK(rl_gridop_set_dense(g, 2, tops.data(), B.data()));
    OK(ski_create(g, w, &s));
    const double noise[2] = {0.1, 0.2};
    const int lens[2] = {150, 150};
    OK(rl_ski_set_noise(s, noise, lens));
    const vec R = ramp((size_t)20 * n, 1.0);
    vec X((size_t)20 * n);
    std::vector<int> iters(20), istop(20);
    vec resid(20);
    // the solver's workspace: kept, too small and replaced, kept again
    for (int nrhs : {3, 20, 3})
        OK(rl_solve_batch(s, R.data(), X.data(), nrhs, RL_MINRES, 1e-8, 10, 40, iters.data(), resid.data(),
                          istop.data(), nullptr));
    vec lanczos((size_t)3 * 16 * 2);
    OK(rl_solve_batch_lanczos(s, R.data(), X.data(), 3, RL_MINRES, 1e-8, 10, 40, iters.data(), resid.data(),
                              istop.data(), lanczos.data(), 16, nullptr));
    // every row in the polynomial form: the Woodbury factorisation and the direct solve
    int avail = -1;
    double logdet = 0.0, cond = 0.0;
    const vec smooth = rbf_row(m, 0.8), B1 = couplings(1, D, 0.3);
    OK(rl_gridop_set_dense(g, 1, smooth.data(), B1.data()));
    OK(rl_ski_factor(s, &avail, &logdet, &cond));
    CHECK(avail == 1);
    EXPECT(rl_solve_direct(s, R.data(), X.data(), 3, 1e-8, 3, iters.data(), resid.data(), istop.data(), nullptr),
           avail == 1 ? RL_OK : RL_ELIMIT);
    // a short Matern row: no polynomial factorisation, the pivoted-Cholesky preconditioner
    const vec rough = matern32_row(m, 0.004);
    OK(rl_gridop_set_dense(g, 1, rough.data(), B1.data()));
    OK(rl_ski_set_pivchol(s, 8, 1e-10));
    OK(rl_ski_factor(s, &avail, &logdet, &cond));
    if (avail != 4) std::printf("rl_ski_factor: available = %d (%s)\n", avail, rl_last_error());
    CHECK(avail == 4);
    OK(rl_solve_pcg(s, R.data(), X.data(), 3, 1e-8, 40, iters.data(), resid.data(), istop.data(), nullptr));
    double logdet_p = 0.0;
    OK(rl_ski_precond_sample(s, R.data(), X.data(), 2, &logdet_p, nullptr));
    OK(rl_solve_pcg(s, R.data(), X.data(), 5, 1e-8, 40, iters.data(), resid.data(), istop.data(), nullptr));
    OK(rl_gridop_destroy(g));
    OK(rl_ski_destroy(s));
}

static void exact_and_sampler() {
    {
        const int n = 40, D = 2;
        rl_exact* h = nullptr;
        OK(rl_exact_create(0, n, 1, &h));
        vec X(n);
        for (int i = 0; i < n; ++i) X[i] = (i % 20) / 20.0 + 0.01 * (i / 20);
        const int lens[2] = {20, 20}, kinds[1] = {RL_EXACT_RBF}, cols[4] = {0, -1, -1, -1};
        const double params[4] = {4.0, 0.0, 0.0, 0.0}, noise[2] = {0.1, 0.2};
        const vec B = couplings(1, D, 0.3);
        OK(rl_exact_set(h, X.data(), lens, D, 1, kinds, params, cols, B.data(), noise));
        double logdet = 0.0;
        int bad_col = 0;
        OK(rl_exact_factor(h, &logdet, &bad_col));
        CHECK(bad_col == -1 && std::isfinite(logdet));
        OK(rl_exact_destroy(h));
    }
    {
        const int D = 2, m = 128, Ls = 256, nsamp = 3;
        rl_gridop* g = nullptr;
        rl_sampler* h = nullptr;
        OK(rl_gridop_create(0, D, m, 1, &g));
        OK(rl_sampler_create(g, &h));
        vec ext(Ls / 2 + 1);
        for (int i = 0; i <= Ls / 2; ++i) ext[i] = std::exp(-0.5 * std::pow(i / (m - 1.0) / 0.2, 2));
        const int nchan[1] = {D}, forms[1] = {0};
        const double F[4] = {1.0, 0.0, 0.3, 1.0};
        double clipped = 0.0;
        long long zlen = 0;
        OK(rl_sampler_set(h, 1, nchan, F, forms, Ls, 0, ext.data(), 0, nullptr, &clipped, &zlen));
        CHECK(zlen == (long long)D * Ls);
        const vec Z = ramp((size_t)4 * (size_t)zlen, 1.0);
        vec U((size_t)nsamp * D * m);
        OK(rl_sampler_draw(h, Z.data(), U.data(), nsamp, nullptr));
        OK(rl_sampler_destroy(h));
        OK(rl_gridop_destroy(g));
    }
}

int main() {
    create_destroy();
    gridop_walk();
    ski_two_terms();
    ski_solves();
    exact_and_sampler();
    if (g_bad) {
        std::printf("lifecycle: %d unexpected result(s)\n", g_bad);
        return 1;
    }
    std::printf("lifecycle ok (%s)\n", rl_backend());
    return 0;
}
