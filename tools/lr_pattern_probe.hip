// Where do the polynomial form's two streaming kernels lose their bandwidth?  The REAL kernels
// (rl_lowrank.h) at the C5 launch shape, with the arithmetic scaled down by the rank template
// parameter (rank 2: the same loads / stores, a twelfth of the multiply-adds) and with row
// lengths that are / are not multiples of a 128-byte line (m = 100004: rows start 32 bytes
// past a line boundary three times out of four):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Irunlmc_amd/csrc -o /tmp/lr_pattern_probe tools/lr_pattern_probe.hip
// Part 4 (`lr_pattern_probe lines`: that part alone) is the ladder of the expansion's STORE mapping,
// profiles/expand_lines: rung 0 k_lr_expand as it is, rung 1 the ascending half in whole lines by row
// class (k_lr_expand_lines, mirror half from its own thread), rung 2 the mirror half through LDS (k_probe_expand_staged), rung 3
// the row blocks padded to a multiple of 8 (column neighbours on one XCD); and, to tell the rungs apart, rung 4
// = rung 0 + that padding alone (k_lr_expand has nothing to do in a surplus row block), rung 5 = rung 1 + the
// padding (no LDS: the library's default).  -DPROBE_RUNGS=<bit mask> compiles a subset (default 0x3F: all six).
// Part 5 (`lr_pattern_probe pair`: that part alone), profiles/pair_policy: the two kernels alternating on
// SEPARATE buffers under every cache policy of the loads and the stores and both depths of the projection.
#include "rl_kernels.h"
#include "rl_lowrank.h"
#include <cstdio>
#include <string>
#include <vector>
#include <algorithm>

template <int R>
static void run(int m, int nrows, int steps) {
    double *X, *part, *beta, *zhat;
    hipMalloc(&X, (size_t)nrows * m * 8);
    hipMemset(X, 0, (size_t)nrows * m * 8);
    const int slots = (m + 1) / 2, chunks = (slots + 64 * steps - 1) / (64 * steps);
    hipMalloc(&part, (size_t)chunks * nrows * R * 8);
    hipMalloc(&beta, 64 * 8);
    hipMemset(beta, 0, 64 * 8);
    hipMalloc(&zhat, (size_t)nrows * R * 8);
    hipMemset(zhat, 0, (size_t)nrows * R * 8);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    std::vector<float> tp, te;
    const int nbx = (slots + 255) / 256, rpb = 16;
    for (int rep = 0; rep < 12; ++rep) {
        float ms;
        hipEventRecord(e0);
        hipLaunchKernelGGL((k_lr_project<R>), dim3(chunks, (nrows + RL_LR_ROWS(R) - 1) / RL_LR_ROWS(R)),
                           dim3(64 * RL_LR_WAVES), (size_t)RL_LR_WAVES * R * 65 * 8, 0, (const double*)X, nrows, m,
                           (const double*)beta, steps, part);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
        if (rep >= 2) tp.push_back(ms);
        hipEventRecord(e0);
        hipLaunchKernelGGL((k_lr_expand<R, false>), dim3(nbx, (nrows + rpb - 1) / rpb), dim3(256), 0, 0,
                           (const double*)zhat, nrows, m, (const double*)beta, rpb, X);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
        if (rep >= 2) te.push_back(ms);
    }
    // ... and each kernel alone, back to back (no write of the other kernel draining meanwhile)
    std::vector<float> tpa, tea;
    for (int rep = 0; rep < 12; ++rep) {
        float ms;
        hipEventRecord(e0);
        hipLaunchKernelGGL((k_lr_project<R>), dim3(chunks, (nrows + RL_LR_ROWS(R) - 1) / RL_LR_ROWS(R)),
                           dim3(64 * RL_LR_WAVES), (size_t)RL_LR_WAVES * R * 65 * 8, 0, (const double*)X, nrows, m,
                           (const double*)beta, steps, part);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
        if (rep >= 2) tpa.push_back(ms);
    }
    for (int rep = 0; rep < 12; ++rep) {
        float ms;
        hipEventRecord(e0);
        hipLaunchKernelGGL((k_lr_expand<R, false>), dim3(nbx, (nrows + rpb - 1) / rpb), dim3(256), 0, 0,
                           (const double*)zhat, nrows, m, (const double*)beta, rpb, X);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
        if (rep >= 2) tea.push_back(ms);
    }
    std::sort(tpa.begin(), tpa.end());
    std::sort(tea.begin(), tea.end());
    printf("   alone: project %6.1f us | expand %6.1f us\n", 1e3 * tpa[tpa.size() / 2], 1e3 * tea[tea.size() / 2]);
    std::sort(tp.begin(), tp.end());
    std::sort(te.begin(), te.end());
    const double gb = (double)nrows * m * 8 / 1e9;
    printf("rank %2d  m %6d  steps %3d (chunks %3d): project %6.1f us %5.2f TB/s | expand %6.1f us %5.2f TB/s\n", R, m,
           steps, chunks, 1e3 * tp[tp.size() / 2], gb / tp[tp.size() / 2], 1e3 * te[te.size() / 2], gb / te[te.size() / 2]);
    hipFree(X); hipFree(part); hipFree(beta); hipFree(zhat);
}

// ---- part 2: a bare reader with the projection's access pattern, one ingredient changed at a time
// wave: RB rows; MIRROR: a point and its mirror per lane-step (ascending + descending stream per
// row) or the whole row ascending; WAVES waves per workgroup; OCC waves per SIMD (attribute);
// rowfast: workgroups numbered with the row block fastest instead of the chunk
template <int RB, bool MIRROR, int WAVES, int OCC, int G>
__global__ void __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(OCC)))
k_read(const double* __restrict__ X, int nrows, int m, int steps, int rowfast, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int pbx = blockIdx.x, pby = blockIdx.y;
    if (rowfast) {
        const int lin = blockIdx.y * gridDim.x + blockIdx.x;
        pbx = lin / gridDim.y;
        pby = lin - pbx * gridDim.y;
    }
    const int row0 = (pby * WAVES + wave) * RB;
    const int n_begin = pbx * (64 * steps);
    const int span = MIRROR ? (m + 1) / 2 : m;
    const double* xrow[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) xrow[r] = X + (size_t)(row0 + r < nrows ? row0 + r : nrows - 1) * m;
    const unsigned rowbytes = (unsigned)m * 8u;
    double xr[G][RB], xm[G][RB], acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 0.0;
#pragma unroll
    for (int k = 0; k < G; ++k)
#pragma unroll
        for (int r = 0; r < RB; ++r) xr[k][r] = xm[k][r] = 0.0;
    for (int t = -G; t < steps; t += G) {
#pragma unroll
        for (int k = 0; k < G; ++k) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < RB; ++r) acc[r] += xr[k][r] + (MIRROR ? xm[k][r] : 0.0);
            const int st = t + k + G < steps ? t + k + G : steps - 1;
            const int n = n_begin + lane + 64 * st;
            const int nc = n < span ? n : span - 1;
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                xr[k][r] = rl_row_load(xrow[r], rowbytes, (unsigned)nc * 8u);
                if (MIRROR) xm[k][r] = rl_row_load(xrow[r], rowbytes, (unsigned)(m - 1 - nc) * 8u);
            }
        }
    }
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < RB; ++r) s += acc[r];
    if (s == 1.2345) out[0] = s;
}
template <int RB, bool MIRROR, int WAVES, int OCC, int G>
static void read_run(const char* what, int m, int nrows, int steps, int rowfast) {
    double *X, *out;
    hipMalloc(&X, (size_t)nrows * m * 8);
    hipMemset(X, 0, (size_t)nrows * m * 8);
    hipMalloc(&out, 8);
    const int span = MIRROR ? (m + 1) / 2 : m, chunks = (span + 64 * steps - 1) / (64 * steps);
    const int rows_wg = RB * WAVES;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    std::vector<float> tp;
    for (int rep = 0; rep < 12; ++rep) {
        float ms;
        hipEventRecord(e0);
        hipLaunchKernelGGL((k_read<RB, MIRROR, WAVES, OCC, G>), dim3(chunks, (nrows + rows_wg - 1) / rows_wg),
                           dim3(64 * WAVES), 0, 0, (const double*)X, nrows, m, steps, rowfast, out);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
        if (rep >= 2) tp.push_back(ms);
    }
    std::sort(tp.begin(), tp.end());
    const double gb = (double)nrows * m * 8 / 1e9;
    printf("%-58s steps %3d chunks %3d wgs %5d: %6.1f us %5.2f TB/s\n", what, steps, chunks,
           chunks * ((nrows + rows_wg - 1) / rows_wg), 1e3 * tp[tp.size() / 2], gb / tp[tp.size() / 2]);
    hipFree(X); hipFree(out);
}

// ---- part 3: the plain ceilings of this box: read-only, write-only and copy of the same 1.03 GB
__global__ void __launch_bounds__(256) k_copy(const double2* __restrict__ a, double2* __restrict__ b, size_t n2, int mode) {
    double2 s = {0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (size_t)gridDim.x * 256) {
        if (mode == 0) { const double2 v = a[i]; s.x += v.x; s.y += v.y; }       // read
        else if (mode == 1) b[i] = double2{1.0, 2.0};                            // write
        else b[i] = a[i];                                                        // copy
    }
    if (mode == 0 && s.x == 1.2345) b[0] = s;
}
static void ceilings() {
    const size_t n2 = (size_t)1290 * 100004 / 2;
    double2 *a, *b;
    hipMalloc(&a, n2 * 16);
    hipMalloc(&b, n2 * 16);
    hipMemset(a, 0, n2 * 16);
    hipMemset(b, 0, n2 * 16);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    const char* names[3] = {"read 1.03 GB", "write 1.03 GB", "copy 1.03 -> 1.03 GB"};
    for (int blocks : {2048, 8192})
        for (int mode = 0; mode < 3; ++mode) {
            std::vector<float> t;
            for (int rep = 0; rep < 12; ++rep) {
                float ms;
                hipEventRecord(e0);
                hipLaunchKernelGGL(k_copy, dim3(blocks), dim3(256), 0, 0, (const double2*)a, b, n2, mode);
                hipEventRecord(e1);
                hipEventSynchronize(e1);
                hipEventElapsedTime(&ms, e0, e1);
                if (rep >= 2) t.push_back(ms);
            }
            std::sort(t.begin(), t.end());
            const double gb = (mode == 2 ? 2.0 : 1.0) * n2 * 16 / 1e9;
            printf("%-22s blocks %5d: %6.1f us  %5.2f TB/s (bytes moved / time)\n", names[mode], blocks, 1e3 * t[t.size() / 2],
                   gb / t[t.size() / 2]);
        }
    hipFree(a); hipFree(b);
}

#ifndef PROBE_RUNGS
#define PROBE_RUNGS 0x3F
#endif
// Rungs 2 and 3: k_lr_expand_lines with the MIRROR half through LDS, so that it leaves in whole lines too.
// Measured (profiles/expand_lines) and kept out of the library: not distinguishable from rung 5.  The block's
// mirror values are the 256 contiguous elements from E0 = row m + m - 1 - (256 bx + 255 - phase), at line offset
// b = (2 phase + m) mod 16.  Thread tid leaves ev - od in stage[buf][255 - tid] (two buffers: ONE barrier per
// row); thread u then takes entry i = (u + h) mod 256, h = (16 - b) mod 16, and stores element E0 + i: waves 0-2
// store whole lines, the block's two fragments (h and b elements) sit in wave 3.  The trip count of the row loop
// is the same for every thread of a block and no dead lane leaves before it (the barrier sits inside).
template <int R>
__global__ void __launch_bounds__(256)
k_probe_expand_staged(const double* __restrict__ Zhat, int nrows, int m, const double* __restrict__ beta,
                      int rows_per_block, int period, int nby, double* __restrict__ Y) {
    __shared__ double stage[2 * 256];
    const int slots = lr_slots(m), tid = threadIdx.x;
    const int lin = blockIdx.y * gridDim.x + blockIdx.x;
    const int bx = lin / gridDim.y, by = lin - bx * gridDim.y;
    if (by >= nby) return;
    const int cls = by % period, kb = by / period;
    const int rfirst = cls + kb * rows_per_block * period;
    if (rfirst >= nrows) return;
    int nr = (nrows - rfirst + period - 1) / period;
    nr = nr < rows_per_block ? nr : rows_per_block;
    const int p0 = (int)((reinterpret_cast<unsigned long long>(Y) >> 3) & 15ull);
    const int phase = (p0 + cls * (m & 15)) & 15;
    const int n = bx * 256 + tid - phase;
    const int nc = n < 0 ? 0 : (n < slots ? n : slots - 1);
    const bool live = n >= 0 && n < slots;
    // the mirror element this thread STORES: entry i2 of the block's 256
    const int h = (16 - ((2 * phase + m) & 15)) & 15;
    const int i2 = (tid + h) & 255;
    const int n2 = bx * 256 + 255 - i2 - phase;
    const int n2c = n2 < 0 ? 0 : (n2 < slots ? n2 : slots - 1);
    const int mir2 = m - 1 - n2c;
    const bool pair2 = n2 >= 0 && n2 < slots && mir2 != n2c;
    const double s = lr_point(nc, m);
    double p[R];
    {
        double qm = 0.0, q = 1.0;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            p[j] = q;
            const double qn = fma(s, q, -beta[j] * qm);
            qm = q;
            q = qn;
        }
    }
    for (int k = 0; k < nr; ++k) {
        const int row = rfirst + k * period;
        const double* z = Zhat + (size_t)row * R;
        double zz[R];
#pragma unroll
        for (int j = 0; j < R; ++j) zz[j] = z[j];
        double* yr = Y + (size_t)row * m;
        __builtin_amdgcn_sched_barrier(0);
        double ev = 0.0, od = 0.0;
#pragma unroll
        for (int j = 0; j + 1 < R; j += 2) {
            ev = fma(zz[j], p[j], ev);
            od = fma(zz[j + 1], p[j + 1], od);
        }
        double* sb = stage + (k & 1) * 256;
        sb[255 - tid] = ev - od;
        if (live) yr[nc] = ev + od;
        __syncthreads();
        const double v = sb[i2];
        if (pair2) yr[mir2] = v;
    }
}
// the expansion of rung RUNG by the library's launch rule (rl_gridop.hip lr_expand); rung 4 is
// RUNLMC_LR_EXPAND_PLAIN=2
template <int R, int RUNG>
static void expand_rung(const double* zhat, int nrows, int m, const double* beta, double* Y) {
    if constexpr (RUNG == 2 || RUNG == 3) {
        const int p0 = (int)((reinterpret_cast<unsigned long long>(Y) >> 3) & 15ull);
        if ((m & 15) == 0 && p0 == 0) {
            lr_expand_launch<R>(zhat, nrows, m, beta, Y, false, 16, 8 * RL_LR_CUS, 1, 0, 0);
            return;
        }
        const LrLinesGrid g = lr_expand_lines_grid(nrows, m, 16, 8 * RL_LR_CUS);
        hipLaunchKernelGGL((k_probe_expand_staged<R>), dim3(g.nbx, RUNG == 3 ? (g.nby + 7) / 8 * 8 : g.nby), dim3(256), 0,
                           0, zhat, nrows, m, beta, g.rpb, g.period, g.nby, Y);
    } else {
        lr_expand_launch<R>(zhat, nrows, m, beta, Y, false, 16, 8 * RL_LR_CUS, RUNG == 0 ? 1 : (RUNG == 4 ? 2 : 0), 0, 0,
                            RUNG == 5);
    }
}
template <int R, int RUNG>
static void ladder_rung(int m, int nrows, int steps) {
    if constexpr (((PROBE_RUNGS >> RUNG) & 1) != 0) {
        double *X, *part, *beta, *zhat;
        hipMalloc(&X, (size_t)nrows * m * 8);
        hipMemset(X, 0, (size_t)nrows * m * 8);
        const int slots = (m + 1) / 2, chunks = (slots + 64 * steps - 1) / (64 * steps);
        hipMalloc(&part, (size_t)chunks * nrows * R * 8);
        hipMalloc(&beta, 64 * 8);
        hipMemset(beta, 0, 64 * 8);
        hipMalloc(&zhat, (size_t)nrows * R * 8);
        hipMemset(zhat, 0, (size_t)nrows * R * 8);
        hipEvent_t e0, e1;
        hipEventCreate(&e0);
        hipEventCreate(&e1);
        std::vector<float> tp, te, tea;
        for (int rep = 0; rep < 13; ++rep) {
            float ms;
            hipEventRecord(e0);
            hipLaunchKernelGGL((k_lr_project<R>), dim3(chunks, (nrows + RL_LR_ROWS(R) - 1) / RL_LR_ROWS(R)),
                               dim3(64 * RL_LR_WAVES), (size_t)RL_LR_WAVES * R * 65 * 8, 0, (const double*)X, nrows, m,
                               (const double*)beta, steps, part);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            hipEventElapsedTime(&ms, e0, e1);
            if (rep >= 2) tp.push_back(ms);
            hipEventRecord(e0);
            expand_rung<R, RUNG>(zhat, nrows, m, beta, X);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            hipEventElapsedTime(&ms, e0, e1);
            if (rep >= 2) te.push_back(ms);
        }
        for (int rep = 0; rep < 13; ++rep) {
            float ms;
            hipEventRecord(e0);
            expand_rung<R, RUNG>(zhat, nrows, m, beta, X);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            hipEventElapsedTime(&ms, e0, e1);
            if (rep >= 2) tea.push_back(ms);
        }
        std::sort(tp.begin(), tp.end());
        std::sort(te.begin(), te.end());
        std::sort(tea.begin(), tea.end());
        const size_t h = tp.size() / 2;
        printf("rung %d rank %2d m %6d: project %6.1f us | expand %6.1f us (min %6.1f max %6.1f) | pair %6.1f | expand alone %6.1f us\n",
               RUNG, R, m, 1e3 * tp[h], 1e3 * te[h], 1e3 * te.front(), 1e3 * te.back(), 1e3 * (tp[h] + te[h]),
               1e3 * tea[h]);
        fflush(stdout);
        hipFree(X); hipFree(part); hipFree(beta); hipFree(zhat);
        hipEventDestroy(e0);
        hipEventDestroy(e1);
    }
}
template <int R>
static void ladder(int m, int nrows) {
    ladder_rung<R, 0>(m, nrows, 32);
    ladder_rung<R, 1>(m, nrows, 32);
    ladder_rung<R, 2>(m, nrows, 32);
    ladder_rung<R, 3>(m, nrows, 32);
    ladder_rung<R, 4>(m, nrows, 32);
    ladder_rung<R, 5>(m, nrows, 32);
}

// ---- part 5 (`lr_pattern_probe pair`: that part alone), profiles/pair_policy: projection and expansion
// ALTERNATING in steady state on SEPARATE buffers X and Y of 1.03 GB each, as a product does (part 1 alternates
// on one buffer), under every value of RUNLMC_LR_POLICY (rl_lowrank.h LrPolicy: load policy x store policy x
// depth of the projection), through the library's two launchers.  No host synchronisation inside the 13 pairs
// of a combination (two to warm up): each kernel starts behind the other one's traffic.  What a policy buys
// shows in the kernel BEHIND the access it changes, so each kernel and the pair's sum are reported.
struct PairBufs {
    double *X, *Y, *part, *beta, *zhat;
};
template <int R>
static void pair_combo(const PairBufs& b, int m, int nrows, int steps, int policy) {
    constexpr int REPS = 13, WARM = 2;
    static hipEvent_t ev[3 * REPS];
    static bool have = false;
    if (!have) {
        for (hipEvent_t& e : ev) hipEventCreate(&e);
        have = true;
    }
    const LrPolicy pol = lr_policy_of(policy, true, (size_t)nrows * m * 8);
    for (int rep = 0; rep < REPS; ++rep) {
        hipEventRecord(ev[3 * rep]);
        lr_project_launch<R>(b.X, nrows, m, b.beta, steps, b.part, pol, 0);
        hipEventRecord(ev[3 * rep + 1]);
        lr_expand_launch<R>(b.zhat, nrows, m, b.beta, b.Y, false, 16, 8 * RL_LR_CUS, 0, policy, 0);
        hipEventRecord(ev[3 * rep + 2]);
    }
    hipEventSynchronize(ev[3 * REPS - 1]);
    std::vector<float> tp, te, ts;
    for (int rep = WARM; rep < REPS; ++rep) {
        float p, e;
        hipEventElapsedTime(&p, ev[3 * rep], ev[3 * rep + 1]);
        hipEventElapsedTime(&e, ev[3 * rep + 1], ev[3 * rep + 2]);
        tp.push_back(p);
        te.push_back(e);
        ts.push_back(p + e);
    }
    std::sort(tp.begin(), tp.end());
    std::sort(te.begin(), te.end());
    std::sort(ts.begin(), ts.end());
    const size_t h = tp.size() / 2;
    printf("pair rank %2d m %6d policy %2d (load %-5s store %-5s rows x ring %s): project %6.1f (%6.1f %6.1f) | expand %6.1f "
           "(%6.1f %6.1f) | sum %6.1f (%6.1f %6.1f) us\n",
           R, m, policy, pol.load == RL_POL_NT ? "nt" : "plain",
           pol.store == RL_POL_NT ? "nt" : (pol.store == RL_POL_SC1 ? "sc1" : "plain"), pol.deep ? "2x4" : "4x2",
           1e3 * tp[h], 1e3 * tp.front(), 1e3 * tp.back(), 1e3 * te[h], 1e3 * te.front(), 1e3 * te.back(), 1e3 * ts[h],
           1e3 * ts.front(), 1e3 * ts.back());
    fflush(stdout);
}
template <int R>
static void pair_all(const PairBufs& b, int m, int nrows) {
    // (the launch without any policy first and last: what moves between the two is drift)
    for (int policy : {0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 0}) pair_combo<R>(b, m, nrows, 32, policy);
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "pair") {
        const int nrows = 1290, mmax = 100004;
        PairBufs b;
        const size_t bytes = (size_t)nrows * mmax * 8;
        const int chunks = ((mmax + 1) / 2 + 64 * 32 - 1) / (64 * 32);
        if (hipMalloc(&b.X, bytes) != hipSuccess || hipMalloc(&b.Y, bytes) != hipSuccess ||
            hipMalloc(&b.part, (size_t)chunks * nrows * 24 * 8) != hipSuccess || hipMalloc(&b.beta, 64 * 8) != hipSuccess ||
            hipMalloc(&b.zhat, (size_t)nrows * 24 * 8) != hipSuccess) {
            fprintf(stderr, "pair: allocation failed\n");
            return 1;
        }
        hipMemset(b.X, 0, bytes);
        hipMemset(b.Y, 0, bytes);
        hipMemset(b.beta, 0, 64 * 8);
        hipMemset(b.zhat, 0, (size_t)nrows * 24 * 8);
        printf("median (min max) of 11, us; sum = the pair's two kernels, per repetition\n");
        for (int pass = 0; pass < 2; ++pass) {
            printf("-- pass %d\n", pass);
            for (int m : {100004, 100000}) {
                pair_all<2>(b, m, nrows);
                pair_all<24>(b, m, nrows);
            }
        }
        if (hipDeviceSynchronize() != hipSuccess) {
            fprintf(stderr, "pair: %s\n", hipGetErrorString(hipGetLastError()));
            return 1;
        }
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "lines") {
        // (two passes: what moves between them is this box's spread, not a rung)
        for (int pass = 0; pass < 2; ++pass) {
            printf("-- pass %d\n", pass);
            for (int m : {100004, 100000}) {
                ladder<2>(m, 1290);
                ladder<24>(m, 1290);
            }
        }
        return 0;
    }
    ceilings();
    {
        const int m = 100004, nr = 1290;
        read_run<4, true, 4, 2, 2>("as the projection: 4 rows/wave, mirror, 4 waves, occ 2, ring 2", m, nr, 32, 0);
        read_run<4, true, 4, 2, 2>("same again (another allocation)", m, nr, 32, 0);
        read_run<4, true, 4, 8, 2>("occupancy 8", m, nr, 32, 0);
        read_run<4, true, 4, 8, 4>("occupancy 8, ring 4", m, nr, 32, 0);
        read_run<4, false, 4, 2, 2>("no mirror (rows ascending)", m, nr, 32, 0);
        read_run<4, false, 4, 8, 4>("no mirror, occupancy 8, ring 4", m, nr, 32, 0);
        read_run<1, true, 4, 8, 4>("1 row/wave, mirror, occupancy 8, ring 4", m, nr, 32, 0);
        read_run<1, false, 4, 8, 4>("1 row/wave, no mirror, occupancy 8, ring 4", m, nr, 32, 0);
        read_run<2, true, 4, 4, 4>("2 rows/wave, mirror, occ 4, ring 4", m, nr, 32, 0);
        read_run<4, true, 4, 2, 2>("row block fastest", m, nr, 32, 1);
        read_run<4, true, 4, 2, 2>("steps 8", m, nr, 8, 0);
        read_run<4, true, 4, 2, 2>("steps 16", m, nr, 16, 0);
        read_run<4, true, 2, 2, 2>("2 waves per workgroup", m, nr, 32, 0);
        read_run<4, true, 8, 2, 2>("8 waves per workgroup", m, nr, 32, 0);
        read_run<8, true, 4, 2, 2>("8 rows/wave", m, nr, 32, 0);
    }

    const int nrows = 1290;
    for (int m : {100004, 100000}) {
        run<2>(m, nrows, 32);
        run<24>(m, nrows, 32);
    }
    run<24>(100004, nrows, 64);
    return 0;
}
