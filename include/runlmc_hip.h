/* runlmc_hip.h -- C ABI of the MI355X-native LMC inference hot path.
 *
 * Drop-in boundary for vlad17/runlmc's matrix-free path.  Every entry point
 * names the reference interface it replaces (file:line in the reference
 * tree).  INTEGRATION.md shows the ctypes binding a runlmc maintainer adds.
 *
 * Conventions
 *   - every function returns 0 on success, nonzero on failure;
 *     rl_last_error() then holds a message (thread-local).  Shape / argument
 *     errors are RL_EINVAL (the Python wrapper raises ValueError, as the
 *     reference does: runlmc/linalg/matrix.py:20-21, bttb.py:93-101).
 *   - "host" pointers are ordinary CPU memory, copied during the call.
 *   - "dev" pointers are device memory owned by the caller (e.g.
 *     torch.Tensor.data_ptr()); fp64, contiguous, vectors stored one after
 *     another: X[v][i].  Grid vectors are output-major, index d*m + i
 *     (reference kronecker.py:42-46); data vectors are the concatenation of
 *     the outputs (reference likelihood.py:30-31).
 *   - `stream` is a hipStream_t (NULL = default stream).  Calls enqueue work
 *     and return; rl_solve_batch / rl_*_host helpers synchronise themselves.
 *   - handles are not thread-safe; one handle per device.
 */
#ifndef RUNLMC_HIP_H
#define RUNLMC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define RL_OK 0
#define RL_EINVAL 1   /* bad argument / shape */
#define RL_EHIP 2     /* HIP runtime error */
#define RL_ENOMEM 3
#define RL_ELIMIT 4   /* problem exceeds a documented kernel limit */
#define RL_ENOTPD 5   /* a Cholesky factorisation met a pivot that is not a positive finite number */

typedef struct rl_gridop rl_gridop;
typedef struct rl_ski rl_ski;
typedef struct rl_exact rl_exact;

/* Version of this ABI: bumped whenever a declared signature changes (2: rl_solve_batch_lanczos
 * gained `method`, round 4; 3: rl_gridop_form_stats added, round 5; 4: rl_ski_factor,
 * rl_solve_direct, rl_solve_pcg, rl_ski_project,
 * rl_gridop_project, rl_gridop_set_rank_hint, rl_gridop_poly_coeffs, rl_slq_log_quadrature,
 * rl_probes_to_int8 added, round 6; 5: the rl_exact_* handle of the exact likelihood; 6: rl_exact_cross_dev
 * and rl_row_dots, the tiled predictive variances; 7: rl_sampler_*, rl_normal_fill and
 * rl_pathwise_residual, the function draws; 8: rl_ski_inverse_diag, rl_ski_precond_apply,
 * rl_diag_accumulate and rl_loo_reduce, leave-one-out cross-validation; callers
 * built against an older version must be rebuilt; rl_exact_set_factors joined version 8
 * without a bump: no declared signature changed, and so did rl_gridop_create_3d and
 * rl_gridop_info_3d, the three-dimensional grids, and rl_ski_set_pivchol, rl_ski_pivchol_info,
 * rl_ski_pivchol_factor and rl_ski_pivchol_build_ms, the pivoted-Cholesky preconditioner).  A binding
 * compares rl_abi_version() with the RL_ABI_VERSION it was written against before its
 * first call (runlmc_amd/_lib.py does) instead of finding out through shifted arguments. */
#define RL_ABI_VERSION 8
int rl_abi_version(void);

const char* rl_last_error(void);
/* "hip-gfx950" for the product library. */
const char* rl_backend(void);
int rl_device_count(int* count);

/* ---- grid operator  K_UU = sum_q B_q (x) T_q  ------------------------------
 * Replaces BTTB.__init__/_cyclic_extend_n (runlmc/linalg/bttb.py:91-120),
 * BTTB.matvec (bttb.py:144-148), Kronecker.matvec (kronecker.py:39-46),
 * SumMatrix.matvec (sum_matrix.py:31-32) and the three grid representations
 * _gen_sum_grid/_gen_bt_grid/_gen_slfm_grid (runlmc/lmc/grid_kernel.py:77-136),
 * which are the same linear operator.
 *   D outputs, m grid points (1-D grid), embedding length L = the smallest
 *   odd * 2^k >= 2m with odd in {1, 3, 5, 9, 15, 25} (any length >= 2m - 1
 *   embeds the Toeplitz matrix exactly; the reference takes the next power
 *   of two, bttb.py:16-19).  max_tops bounds Q in later rl_gridop_set_* calls.
 *   D is not limited (the reference's Kronecker has no limit, kronecker.py:39-46):
 *   up to 16 outputs the D x D mix runs inside the product's kernels; above, the
 *   handle applies T_q to the nvec * D rows through a one-output handle of its own
 *   and mixes the outputs in a pass of its own (Q products + Q mix passes).      */
int rl_gridop_create(int device, int D, int m, int max_tops, rl_gridop** out);
/* Same for a two-dimensional m1 x m2 grid: T_q is then a block-Toeplitz matrix
 * of Toeplitz blocks, BTTB(top, (m1, m2)) (bttb.py:91-148 with two sizes; grid
 * index i1*m2 + i2, top rows are k_q of the distances to grid point (0, 0)).
 * The embedding is an N1 x N2 two-dimensional circulant, N_k = pow2 >= 2 m_k.
 * Every other entry point is unchanged (m = m1*m2 points per output).
 * Limits: N_k <= 4096, i.e. at most 2048 points per axis (RL_ELIMIT beyond, from a
 * host check before any launch).  A row tile of D outputs that exceeds the LDS
 * (N2 = 1024: D >= 8; 2048: D >= 4; 4096: D >= 2) runs through the one-output
 * handle and the mix pass described above, as D > 16 does.                    */
int rl_gridop_create_2d(int device, int D, int m1, int m2, int max_tops, rl_gridop** out);
/* Same for a three-dimensional m0 x m1 x m2 grid: T_q is a three-level block-Toeplitz
 * matrix, BTTB(top, (m0, m1, m2)) (bttb.py:91-148 with three sizes; grid index
 * (i0*m1 + i1)*m2 + i2, m = m0*m1*m2 points per output).  The leading axis is embedded
 * in a circulant of N0 = pow2 >= 2 m0 (>= 4) points; a real transform along it
 * (csrc/rl_lead.h) turns the product into F = N0/2 + 1 two-dimensional products over
 * (m1, m2), one per leading frequency, each run by a complete rl_gridop_create_2d
 * operator the handle owns (its real top rows are sum_j c_q[j] cos(2 pi f j / N0), set
 * on the host in fp64 by rl_gridop_set_*), on the real and the imaginary slab as two
 * ordinary vectors; the inverse transform follows.  All on the caller's stream, in order.
 * Every product entry point is unchanged; rl_gridop_info reports the inner
 * (L, N1, N2, colsA, rowsB).  The structured forms do not exist on these grids:
 * rl_gridop_form reports rank 0, rl_gridop_top_forms 0 for every row,
 * rl_gridop_project / rl_gridop_spectrum_host answer RL_ELIMIT, rl_ski_factor reports
 * available = 0, rl_sampler_create RL_ELIMIT.
 * Limits (RL_ELIMIT from host checks before any launch): m0 <= 64 -- put the shortest
 * axis first --, the two-dimensional limits above on (m1, m2), m0*m1*m2 <= 2^27.
 * Workspace: 2 F 2 nvec D m1 m2 doubles and the children's own at 2 nvec vectors,
 * allocated by the first product of that many vectors outside a stream capture
 * (inside one an unreserved workspace is RL_EINVAL, never an allocation).       */
int rl_gridop_create_3d(int device, int D, int m0, int m1, int m2, int max_tops,
                        rl_gridop** out);
/* Leading axis of a three-dimensional handle: its extent, its embedding length and the
 * number of leading frequencies (all 0 for one- and two-dimensional handles; any
 * pointer may be NULL).                                                         */
int rl_gridop_info_3d(const rl_gridop* g, int* m0, int* N0, int* F);
int rl_gridop_destroy(rl_gridop* g);
/* L = N1*N2 and tile parameters actually chosen (any pointer may be NULL). */
int rl_gridop_info(const rl_gridop* g, int* L, int* N1, int* N2, int* colsA, int* rowsB);
/* Which form of the product the CURRENT parameters run in (valid after a
 * rl_gridop_set_* call; any pointer may be NULL):
 *   *rank          0: transform (FFT) kernels only;  r > 0: every top row is,
 *                  to 2e-13 of its products, Phi C_q Phi^T with Phi the r
 *                  orthonormal polynomials on the grid, and batches of at
 *                  least *min_elements = nvec*D*m elements run as
 *                  project -> r x r map -> expand (csrc/rl_lowrank.h) -- the
 *                  same operator of bttb.py:144-148, verified per top row
 *                  against the transform kernels inside the set call.
 *   RUNLMC_NO_LOWRANK=1 keeps every handle on the transform kernels (an A/B
 *   hook like RUNLMC_NO_FILTER and RUNLMC_LR_MIN below: read ONLY when
 *   RUNLMC_DEBUG=1 is set as well -- without it the library runs its defaults and
 *   names every hook it ignored once on stderr; the switches that are always
 *   read are RUNLMC_POW2_ONLY, RUNLMC_WS_CACHE_MB and RUNLMC_TRACE).           */
int rl_gridop_form(const rl_gridop* g, int* rank, long long* min_elements);
/* The form EACH top row runs in for the current parameters (forms host [Q], may
 * be NULL): 0 transform kernels; 1 polynomial-subspace form; 2 recursive
 * filter -- an exponential-polynomial row t_i = (c0 + c1 i + c2 i^2) rho^i, i.e.
 * the reference's Matern-3/2 kernel on a regular grid and its derivative
 * (runlmc/kern/matern32.py:40-55), is exactly semiseparable and its product a
 * two-sided scan (csrc/rl_filter.h), detected from the row itself.
 * *structured = 1 when no top needs the transform kernels, so that operator
 * products of batches above the gate move x and y and nothing else.  Single-top
 * products (rl_gridop_mvm_top) take each top's own form either way.
 * RUNLMC_NO_FILTER=1 (with RUNLMC_DEBUG=1) switches form 2 off.                  */
int rl_gridop_top_forms(const rl_gridop* g, int* forms, int* structured);
/* What the last set-time verification of the polynomial form measured for top row q
 * (host out4; zeros when the row was never a candidate): [0] max|T x - Phi C Phi^T x| /
 * max|T x| for the fixed trial vector, [1] the largest response to the first omitted
 * polynomials relative to the largest response inside the subspace, [2] the power
 * iteration's estimate of ||T - Phi C Phi^T||_2 (8 steps through the two products of this
 * handle, from the unit-norm trial vector), [3] the same iteration's ||T||_2.  The row is
 * accepted when [0], [1] <= 2e-13 and [2] <= 2e-13 [3].  [2] and [3] are ESTIMATES FROM
 * BELOW (a power iteration climbs towards the norm; after 8 steps from a vector with a
 * ~1/sqrt(m) component along the leading eigenvector it holds roughly half of it or
 * more), not upper bounds: the test catches an error the sampled tests miss in whatever
 * direction it lies, with a margin of three decades to the honest rows' 2e-16, it does
 * not prove ||E||_2 <= 2e-13 ||T||_2.
 * (Diagnostics of this library's own forms; the operator is bttb.py:144-148 either way.) */
int rl_gridop_form_stats(const rl_gridop* g, int q, double* out4);
/* Moves that batch gate for this handle (0: every batch; < 0: back to the
 * default, 2^20 elements or RUNLMC_LR_MIN under RUNLMC_DEBUG=1).  Below the gate the polynomial
 * form is slower than the transform kernels (too few workgroups).           */
int rl_gridop_set_form_gate(rl_gridop* g, long long min_elements);
/* Parameters of the LMC kernel, in the reference's own factored form
 * B_q = A_q^T A_q + diag(kappa_q) (runlmc/lmc/functional_kernel.py:280-287):
 *   tops        host [Q][m]   first rows k_q(grid distances)
 *   ranks       host [Q]      R_q >= 0
 *   coreg_vecs  host [sum R_q][D]   rows of A_0, then A_1, ...
 *   coreg_diags host [Q][D]
 * Rebuilds the Q circulant spectra on the device (per optimiser step).      */
int rl_gridop_set_lmc(rl_gridop* g, int Q, const double* tops, const int* ranks,
                      const double* coreg_vecs, const double* coreg_diags);
/* Same with arbitrary symmetric B_q given densely, host [Q][D][D]
 * (Kronecker(NumpyMatrix(B), BTTB(top)), kronecker.py:30-46).               */
int rl_gridop_set_dense(rl_gridop* g, int Q, const double* tops, const double* B);

/* Y[v] = K_UU X[v], v < nvec.  X, Y dev [nvec][D*m]; may not alias.         */
int rl_gridop_mvm(rl_gridop* g, const double* X, double* Y, int nvec, void* stream);
/* Y[v] = (I_D (x) T_q) X[v]: one top row applied to every output block
 * (BTTB.matmat, matrix.py:55-67 + bttb.py:144-148).                          */
int rl_gridop_mvm_top(rl_gridop* g, int q, const double* X, double* Y, int nvec, void* stream);
/* Circulant spectrum of top q in NATURAL frequency order, host out[L]
 * (test hook; the reference's BTTB._circ_fft real part, bttb.py:108).       */
int rl_gridop_spectrum_host(rl_gridop* g, int q, double* out);

/* ---- SKI operator  K~ = W K_UU W^T + diag(eps)  ----------------------------
 * Replaces SKI / Composition.matvec (runlmc/approx/ski.py:8-16,
 * linalg/composition.py:14-17), Diag.matvec (linalg/diag.py:24-25) and the
 * SumMatrix assembled by gen_grid_kernel (lmc/grid_kernel.py:70-74).
 *   W   CSR n x (D*m)  (host; int32 indices; reference
 *       approx/interpolation.py:119-176), WT its transpose in CSR.
 * The handle keeps a pointer to `g` (not owned): every product and solve uses
 * it, so destroy the SKI handle BEFORE its grid operator(s).  (rl_ski_destroy
 * itself does not touch `g`, so the other order only leaks nothing and crashes
 * nothing -- but no other call on the handle is valid once `g` is gone.)     */
int rl_ski_create(rl_gridop* g, int n, const int* W_indptr, const int* W_indices,
                  const double* W_data, const int* WT_indptr, const int* WT_indices,
                  const double* WT_data, rl_ski** out);
int rl_ski_destroy(rl_ski* s);
/* Kernels split over several active-dimension sets live on several grids:
 * K~ = sum_t W_t K_t W_t^T + diag(eps) (the SumMatrix of one GridKernel per
 * active-dimension set that gen_grid_kernel builds, grid_kernel.py:51-74).
 * Adds term t >= 1: its grid operator (same D, same device, not owned) and its
 * interpolant pair, n x (D*m_t).  Terms are numbered in the order added.     */
int rl_ski_add_term(rl_ski* s, rl_gridop* g, const int* W_indptr, const int* W_indices,
                    const double* W_data, const int* WT_indptr, const int* WT_indices,
                    const double* WT_data);
/* noise host [D], lens host [D] (sum lens == n): eps repeated per output
 * (np.repeat(noise, lens), grid_kernel.py:70).                               */
int rl_ski_set_noise(rl_ski* s, const double* noise, const int* lens);
/* Known per-observation variances on top: e = np.repeat(noise, lens) + extra, extra host [n] >= 0
 * in the CALLER's row order (the order of W's rows; the handle permutes it as it permutes the
 * diagonal of rl_ski_set_noise).  K~ = sum_t W_t K_t W_t^T + diag(e); extra is never a parameter.
 * The handle becomes a row-noise handle: its factorisation (rl_ski_factor, rl_solve_direct,
 * rl_solve_pcg*, rl_ski_precond_*, rl_ski_inverse_diag) is that of the symmetrically scaled
 * unit-noise problem K~ = E^1/2 (F~ M F~^T + I) E^1/2, F~ = diag(e^-1/2) F, whatever the rows'
 * order; the 96-function preconditioner (mode 3) declines and the 48 functions (mode 2) take its
 * place.  A later rl_ski_set_noise returns the handle to the per-output state.  RL_EINVAL: NULL,
 * a negative or non-finite extra, sum(lens) != n.  (Joined ABI version 8 without a bump: no
 * declared signature changed.)                                                                  */
int rl_ski_set_noise_rows(rl_ski* s, const double* noise, const int* lens, const double* extra);
/* Y[v] = K~ X[v];  X, Y dev [nvec][n]; may not alias.                        */
int rl_ski_mvm(rl_ski* s, const double* X, double* Y, int nvec, void* stream);
/* G[v] = W^T X[v] (dev [nvec][D*m])  /  Y[v] = W G[v] (dev [nvec][n]).      */
int rl_ski_apply_wt(rl_ski* s, const double* X, double* G, int nvec, void* stream);
int rl_ski_apply_w(rl_ski* s, const double* G, double* Y, int nvec, void* stream);
/* The same with the interpolants of term `term` (0 = the first).             */
int rl_ski_apply_wt_term(rl_ski* s, int term, const double* X, double* G, int nvec, void* stream);
int rl_ski_apply_w_term(rl_ski* s, int term, const double* G, double* Y, int nvec, void* stream);

/* ---- batched Krylov solves  K~ X = B  --------------------------------------
 * Replaces Iterative.solve (runlmc/approx/iterative.py:23-62) and the N+1
 * pool-mapped solves of StochasticDerivService._concurrent_solve
 * (runlmc/lmc/stochastic_deriv.py:39-52).  All right-hand sides advance
 * together, each with its own recurrence scalars and stopping state.
 *   B, X      dev [nrhs][n]   (X is written; initial guess is 0 as in the
 *                              reference)
 *   method    RL_MINRES (reference default, stochastic_deriv.py:37), RL_CG, or
 *             RL_MINRES_RULE: MINRES with SciPy's own stopping tests (istop 1-4:
 *             test1 / test2 / Acond / epsx) switched off, so that a system ends
 *             only on the reference's explicit residual rule below or at
 *             maxiter -- how the reference's PUBLISHED runs ended (iteration
 *             counts are multiples of 100 and residuals < 1e-4 in
 *             benchmarks/representation-cmp/out/inv-run-1.txt:3-20; SciPy
 *             1.15's test1 <= rtol exit fires long before on the same systems,
 *             DESIGN.md section 5).  Needs check_every > 0.
 *   tol       absolute residual target of the reference's rule; the inner
 *             method runs with rtol = min(1e-10, tol) (iterative.py:50-51)
 *   check_every  explicit-residual check period (reference: 100,
 *             iterative.py:39); a system whose ||b - K~x||_2 < tol at a check
 *             is frozen; 0 disables the rule
 *   maxiter   <= 0 means n (iterative.py:51)
 *   iters_out host [nrhs] iterations run (the reference's callback count),
 *   resid_out host [nrhs] final ||b - K~x||_2 (iterative.py:54),
 *   istop_out host [nrhs] exit reason: SciPy minres istop codes 1..6, -1;
 *             10 = reference residual rule; 11 = zero right-hand side.
 * Any of the three output pointers may be NULL.  Synchronises before it
 * returns.  Non-convergence is NOT an error (the reference logs and returns
 * the iterate, iterative.py:55-58).  The solver's work vectors stay on the
 * handle between calls (freed by rl_ski_destroy; environment variable
 * RUNLMC_WS_CACHE_MB bounds what is kept).                                     */
#define RL_MINRES 0
#define RL_CG 1
#define RL_MINRES_RULE 2
int rl_solve_batch(rl_ski* s, const double* B, double* X, int nrhs, int method, double tol,
                   int check_every, int maxiter, int* iters_out, double* resid_out,
                   int* istop_out, void* stream);

/* Same solve, additionally returning the Lanczos tridiagonal MINRES builds for
 * each system: lanczos_out host [nrhs][lanczos_cap][2] = (alfa_k, beta_{k+1})
 * for k = 1..min(iterations, lanczos_cap) (untouched beyond).  With
 * Rademacher right-hand sides these give a stochastic-Lanczos-quadrature
 * estimate of log det K~ at no extra operator products -- the matrix-free
 * log-determinant the reference lists as future work (README.md:88-89; its
 * own log_det_K is a dense Cholesky, models/interpolated_llgp.py:262-276).
 * method: RL_MINRES or RL_MINRES_RULE; lanczos_out may be NULL (then identical to
 * rl_solve_batch). */
int rl_solve_batch_lanczos(rl_ski* s, const double* B, double* X, int nrhs, int method,
                           double tol, int check_every, int maxiter, int* iters_out,
                           double* resid_out, int* istop_out, double* lanczos_out,
                           int lanczos_cap, void* stream);

/* Host helper for that estimate: out[v] = sqnorms[v] * e_1^T log(T_v) e_1 for the Lanczos
 * tridiagonal T_v of system v (lanczos host [nrhs][cap][2] as rl_solve_batch_lanczos fills
 * it, k = min(iters[v], cap) steps) -- Gauss quadrature of r^T log(K~) r by the implicit QL
 * iteration carrying one row of the eigenvector matrix, O(k^2) per system, systems spread
 * over `nthreads` host threads; out[v] = NaN for a system whose iteration did not settle
 * (the caller falls back to LAPACK for it).  No device work.  (The mean of out over Rademacher probes,
 * sqnorms = n, estimates log det K~.)                                                      */
int rl_slq_log_quadrature(const double* lanczos, int nrhs, int cap, const int* iters,
                          const double* sqnorms, double* out, int nthreads);
/* Host helper: the reference draws its Rademacher probes as an int64 matrix
 * (lmc/stochastic_deriv.py:35: randint(0, 2, (N, n)) * 2 - 1 -- 1 GB at BASELINE's C5).  One
 * pass over it on `nthreads` host threads: dst[r][k] = (int8) src[r * row_stride + k] for
 * nrows rows of n entries, *all_pm1 = 1 iff every entry is +1 or -1 (else the caller sends the
 * matrix the plain way).  dst may be pinned memory; no device work.                        */
int rl_probes_to_int8(const long long* src, int nrows, long long row_stride, long long n,
                      signed char* dst, int nthreads, int* all_pm1);

/* ---- direct solves through the polynomial form ------------------------------
 * The reference's Iterative.solve takes a preconditioner from the operator
 * (runlmc/approx/iterative.py:47-51: M = getattr(K, 'preconditioner', None), handed to
 * SciPy's minres / cg) and no reference operator provides one.  This library does, for
 * operators whose top rows are ALL in the polynomial-subspace form (rl_gridop_form,
 * rank r): such a K~ is  F M F^T + diag(eps)  with F = W Phi block-diagonal by output
 * (n x D r) -- a diagonal plus rank D r -- and the Woodbury identity gives
 *     K~^-1 b = E^-1 b - E^-1 F Z F^T E^-1 b          (Z: D r x D r, host Cholesky)
 *     log det K~ = sum_d n_d log eps_d + log det(I + L^T M L),   F^T E^-1 F = L L^T
 * (csrc/rl_direct.h).  With M = K~^-1 to roundoff a preconditioned iteration IS
 * iterative refinement, and the reference's own residual rule ends it.
 *
 * rl_ski_factor: (re)builds the factorisation for the CURRENT parameters and noise
 * (cached on the handle until either changes; runs the pending set-time verification of
 * the polynomial form whatever the batch gate).  *available = 0 when the operator has
 * no such form (a top row on the transform or filter kernels, several grids, a 2-D
 * grid, D > 16, noise not constant per output, an output with fewer rows than the
 * basis, D r > 576 on a system of fewer than 10^5 (D r / 576)^3 rows: there the host's
 * ~1.5 (D r)^3 multiply-adds cost more than the Krylov solve) -- rl_last_error() then says
 * which; that is not an error.  *logdet receives
 * log det K~ of the handle's operator -- the quantity the reference computes by a dense
 * Cholesky (models/interpolated_llgp.py:262-276) -- and *cond an estimate of the condition
 * number of the D r x D r system (squared ratio of its Cholesky pivots).  Any pointer may
 * be NULL.                                                                              */
int rl_ski_factor(rl_ski* s, int* available, double* logdet, double* cond);
/* *available = 2: NOT every top row is in the polynomial form (a Matern row, say, on the filter
 * kernels), but the polynomial subspace still holds at least 0.8 of every row's spectrum: the
 * factorisation then inverts the operator's PROJECTION on the subspace,  F M_r F^T + E  with
 * C_q = Phi^T T_q Phi of every row -- not K~^-1 (no log det), but the symmetric positive definite
 * M of the reference's  sla.cg(op, y, M=M)  (iterative.py:47-51).  rl_solve_pcg runs SciPy's
 * statements of preconditioned conjugate gradients with it, all systems in lockstep, each ended
 * by the reference's rule ||b - K~ x||_2 < tol (the recurrence's residual norm every iteration,
 * the explicit residual before a system is let go), at most maxiter iterations (<= 0: n).
 * BASELINE's 'mix' family (four smooth rows and a Matern row) ends in 4-5 iterations where
 * MINRES runs 590 without meeting the rule; Matern rows alone take ~100.
 * *available = 3: the same on a LARGER basis of the handle's own -- operators of >= 10^5 rows
 * not entirely in the polynomial form: up to 192 polynomials per output (as many blocks of 48
 * as D * R <= 2048, m >= 8 R and n >= 10^5 (D R / 960)^3 allow; a factorisation uses the
 * first blocks that hold all but 1e-5 of every row's trace), table, Gram matrices once per
 * handle, the map per parameter update
 * (csrc/rl_solve.hip hz_*).  C5 (n = 10^6): Matern rows 38 iterations (48 functions: 1358),
 * the mix family 11 (59).  Callers treat 2 and 3 alike.  Also valid with
 * *available = 1 (then M is K~^-1 and one iteration suffices: rl_solve_direct is the shorter way).
 *   iters_out / resid_out / istop_out as rl_solve_direct (istop 6: maxiter reached).       */
int rl_solve_pcg(rl_ski* s, const double* B, double* X, int nrhs, double tol, int maxiter,
                 int* iters_out, double* resid_out, int* istop_out, void* stream);
/* log det K~ on that path (the reference's log_det_K, models/interpolated_llgp.py:262-276, is a dense
 * Cholesky; rounds 1-5 answered with Lanczos quadrature of the UNpreconditioned solves, which these
 * operators' solves no longer run):  log det K~ = log det P + tr log(P^-1/2 K~ P^-1/2),  P the
 * factorised matrix (its log det exact, determinant lemma), the trace by Hutchinson + Gauss
 * quadrature on the Lanczos matrices conjugate gradients build anyway -- unbiased when the right-hand
 * sides have covariance P.  The preconditioned operator is close to I, so the estimator's variance
 * is orders of magnitude below the plain quadrature's: a dozen probes do.
 * rl_ski_precond_sample: Rout[v] = P^1/2 Win[v]  (P = E^1/2 B B^T E^1/2, B = I + Q (C - I) Q^T from
 *   the factorisation's own Cholesky factors: one projection, one dense map, one expansion; Win, Rout
 *   dev [nvec][n], caller's row order; Win rows of identity covariance, e.g. the reference's +-1
 *   probes), *logdet_p = log det P.  The first call makes the handle keep that map with every later
 *   factorisation.
 * rl_solve_pcg_lanczos: rl_solve_pcg that also leaves each system's Lanczos matrix of P^-1/2 K~ P^-1/2
 *   (lanczos_out host [nrhs][cap][2]: diagonal, off-diagonal; as rl_solve_batch_lanczos) and
 *   sqnorms_out[v] = r0^T P^-1 r0 -- what rl_slq_log_quadrature takes; at most cap iterations, no
 *   restarts from explicit residuals.                                                       */
int rl_ski_precond_sample(rl_ski* s, const double* Win, double* Rout, int nvec, double* logdet_p,
                          void* stream);
int rl_solve_pcg_lanczos(rl_ski* s, const double* B, double* X, int nrhs, double tol, int maxiter,
                         int* iters_out, double* resid_out, int* istop_out, double* lanczos_out,
                         int cap, double* sqnorms_out, void* stream);
/* The pieces of that form, for callers that work in its coefficient space (the gradient's
 * Gram terms: with T = Phi C Phi^T,  u~_a . T v~_b = c_u[a]^T C c_v[b],  c_u = Phi^T W^T u
 * -- runlmc_amd/lmc/likelihood.py; reference loops: lmc/likelihood.py:48-96):
 * rl_ski_project: out[v][d][j] = (Phi^T W^T X[v])[d][j], the r coefficients per output on the
 * ORTHONORMAL polynomials (dev out [nvec][D][r], *rank = r; X dev [nvec][n], caller's row
 * order); RL_ELIMIT when rl_ski_factor reports *available = 0.
 * rl_gridop_poly_coeffs: C_q = Phi^T T_q Phi (symmetrised) of top row q into host out
 * [r][r] (cap >= r * r values) and *rank = r -- or *rank = 0 when the row is not in the
 * polynomial form (the pending verification runs first; out may be NULL to ask only).   */
int rl_ski_project(rl_ski* s, const double* X, int nvec, double* out, int* rank, void* stream);
/* The same for GRID vectors and any of the basis sizes: out[v][d][j] = (Phi_rank^T X[v][d])[j]
 * (X dev [nvec][D*m], out dev [nvec][D][rank], rank one of 24, 32, 36, 40, 48) -- for callers
 * whose derivative rows need a larger basis than the operator's own (Phi is nested: the first
 * r functions of a larger basis are the smaller one).                                       */
int rl_gridop_project(rl_gridop* g, const double* X, int nvec, int rank, double* out, void* stream);
/* Where the set-time verification of the polynomial form starts its ladder of basis sizes
 * (24, 32, 36, 40, 48; 0 = from the bottom): a handle holding the derivative rows of kernels
 * whose own rows were accepted at rank r elsewhere need not try the smaller ones.  Only speed
 * depends on it (a rank that is larger than needed costs proportionally more).           */
int rl_gridop_set_rank_hint(rl_gridop* g, int rank);
int rl_gridop_poly_coeffs(rl_gridop* g, int q, double* out, int cap, int* rank);
/* X[v] = K~^-1 B[v]:  x = M b, then  x += M (b - K~ x)  while the reference's rule
 * ||b - K~ x||_2 < tol (iterative.py:36-42,54-58) does not hold, at most max_refine
 * times (the residual is taken through the handle's ordinary product, rl_ski_mvm's
 * path).  B, X dev [nrhs][n], may not alias.
 *   iters_out host [nrhs]  applications of M (1 + refinements) -- the count a
 *                          preconditioned Krylov method would report
 *   resid_out host [nrhs]  final ||b - K~ x||_2
 *   istop_out host [nrhs]  10 = the reference's residual rule; 12 = tolerance not
 *                          reached within max_refine refinements (the iterate is
 *                          returned, as the reference returns its own: iterative.py:55-58)
 * RL_ELIMIT when rl_ski_factor would report *available = 0.  Synchronises.            */
int rl_solve_direct(rl_ski* s, const double* B, double* X, int nrhs, double tol,
                    int max_refine, int* iters_out, double* resid_out, int* istop_out,
                    void* stream);

/* ---- partial sums of the Hutchinson gradient --------------------------------
 * Replace the P*(N+1) operator products of StochasticDeriv.d_normal_quadratic
 * / d_logdet_K (runlmc/lmc/stochastic_deriv.py:69-78) driven by
 * LMCLikelihood's loops (runlmc/lmc/likelihood.py:48-96): with u~ = W^T u
 * reshaped D x m,  u^T W (dB (x) T) W^T v = sum_ab dB[a,b] u~_a . (T v~_b), so
 * one D x D Gram matrix per (vector pair, top row) serves every
 * coregionalisation parameter at once.
 *   out[v][a][b] = sum_i U[v][a*m+i] * V[v][b*m+i];  U, V dev [nvec][D*m],
 *   out dev [nvec][D][D].                                                     */
int rl_cross_dots(const double* U, const double* V, int nvec, int D, int m, double* out,
                  void* stream);
/* out[v][d] = sum_{i in output d} U[v][i] * V[v][i] over data-space vectors
 * (noise gradient, likelihood.py:89-96 with Diag(repeat(e_d, lens))):
 * offsets dev int[D+1], U, V dev [nvec][n], out dev [nvec][D].                */
int rl_segment_dots(const double* U, const double* V, const int* offsets, int nvec, int n,
                    int D, double* out, void* stream);

/* ---- exact (dense) LMC likelihood ------------------------------------------
 * Replaces ExactLMCLikelihood (runlmc/lmc/likelihood.py:137-217: the dense K, scipy's
 * cho_factor, ExactDeriv's alpha and K^-1, exact_deriv.py:13-23) and the dense pieces the model
 * takes from it (models/interpolated_llgp.py:248-260 K(), 262-276 log det, 350-356 'exact'
 * variances).  fp64 throughout; ONE n x n device buffer (K, then L, then the lower triangle of
 * K^-1) plus O(64 n) workspaces, so n is bounded by free device memory (RL_ENOMEM past it).
 *   K = sum_q B_q[d(i), d(j)] k_q(r_q(x_i, x_j)) + diag(noise[d(i)]),  r_q the Euclidean distance
 *   over kernel q's active input columns, rows = outputs concatenated (likelihood.py:30-31).
 * Limits (RL_ELIMIT): D <= 64, Q + sum_q p_q <= 32 (p_q: parameters of kernel q), <= 4 active
 * columns per kernel.  Synchronous except rl_exact_solve.                                        */
#define RL_EXACT_RBF 0          /* exp(-g r^2 / 2)              params [g]        (kern/rbf.py) */
#define RL_EXACT_MATERN32 1     /* (1 + s) e^-s, s = sqrt(3) g r  params [g]      (kern/matern32.py) */
#define RL_EXACT_STDPERIODIC 2  /* exp(-g sin^2(pi r / T) / 2)  params [g, T]     (kern/std_periodic.py) */
#define RL_EXACT_MATERN52 3     /* (1 + s + s^2 / 3) e^-s, s = sqrt(5) g r  params [g]  (no reference twin) */
#define RL_EXACT_SCALED 16      /* OR'ed in: c k(r), params[2] = c, one more parameter (kern/scaled.py) */
/* n data points of P input columns each. */
int rl_exact_create(int device, int n, int P, rl_exact** out);
int rl_exact_destroy(rl_exact* h);
/* Parameters (per optimiser step; nothing is computed yet):
 *   X host [n][P]; lens host [D] (sum n); kinds host [Q]; params host [Q][4];
 *   active_cols host [Q][4] (column indices, -1 after the last); B host [Q][D][D]; noise host [D].
 * The parameters of kernel q are ordered as its kernel_gradient (derivatives), which fixes the
 * slots of rl_exact_grad_sums.                                                                  */
int rl_exact_set(rl_exact* h, const double* X, const int* lens, int D, int Q, const int* kinds,
                 const double* params, const int* active_cols, const double* B, const double* noise);
/* The same with every latent kernel a product  c prod_{f < nfact[q]} k_f(r)  of 1 .. 3 leaf
 * kernels on ONE distance over the kernel's active columns (runlmc_amd/kern/stationary.py:
 * Product, Cosine; the reference has neither):
 *   nfact host [Q] (1 .. RL_EXACT_MAX_FACT); leaf_kinds host [Q][3]: RL_EXACT_RBF .. RL_EXACT_COSINE
 *   (no RL_EXACT_SCALED here); leaf_params host [Q][3][2]: a leaf's parameters as listed above;
 *   scaled host [Q] (0 / 1) and scales host [Q]: the factor c, a parameter when scaled[q];
 *   entries of factors f >= nfact[q] are not read.  X, lens, active_cols, B, noise as above.
 * Derivative order of kernel q (the slots of rl_exact_grad_sums): the factors in order, each
 * factor's parameters in its own order (product rule: dk_f / dtheta_p prod_{g != f} k_g, times c),
 * then the scale's (prod_f k_f): at most 2 * 3 + 1 = 7, and Q + sum_q p_q <= 32 as above
 * (RL_ELIMIT, the message names the count).  RL_EINVAL: an unknown leaf kind, nfact outside
 * 1 .. 3.  A one-factor list computes what rl_exact_set computes, bit for bit; every later call
 * works unchanged in the state either call leaves.                                             */
#define RL_EXACT_COSINE 4       /* cos(2 pi f r)               params [f]   (a leaf of rl_exact_set_factors only) */
#define RL_EXACT_MAX_FACT 3
int rl_exact_set_factors(rl_exact* h, const double* X, const int* lens, int D, int Q,
                         const int* nfact, const int* leaf_kinds, const double* leaf_params,
                         const int* scaled, const double* scales, const int* active_cols,
                         const double* B, const double* noise);
/* The same with every LEAF on a distance of its own: a latent kernel is the separable product
 *   c prod_{f < nfact[q]} k_f(r_f),  r_f the Euclidean distance over leaf f's own input columns
 * (runlmc_amd/kern/stationary.py: Separable, RBF.ard; the reference has neither):
 *   nfact, leaf_kinds, leaf_params, scaled, scales, X, lens, B, noise as rl_exact_set_factors;
 *   leaf_cols host [Q][3][4]: the column indices of leaf f of kernel q, -1 after the last; the
 *   lists of factors f >= nfact[q] are not read.  Leaves of one kernel may share columns (a Product
 *   factor of a Separable) -- nothing here asks the lists to be disjoint.
 * Derivative order and slots: identical to rl_exact_set_factors.  Limits: at most 3 leaves and
 * 4 columns per leaf; Q + sum_q p_q <= 32 (RL_ELIMIT, the message names the count).  RL_EINVAL: a
 * column index >= P, a leaf without a column, nfact outside 1 .. 3, an unknown leaf kind.
 * Every leaf's distance is summed as a kernel's is, so a set whose leaves all list their kernel's
 * columns computes what rl_exact_set_factors computes, bit for bit.  Every later call works
 * unchanged in the state this leaves; a later rl_exact_set / rl_exact_set_factors on the same
 * handle returns to those paths.  (Joined ABI version 8 without a bump: no declared signature
 * changed.)                                                                                    */
int rl_exact_set_separable(rl_exact* h, const double* X, const int* lens, int D, int Q,
                           const int* nfact, const int* leaf_kinds, const double* leaf_params,
                           const int* leaf_cols, const int* scaled, const double* scales,
                           const double* B, const double* noise);
/* Known per-observation variances extra host [n] >= 0 (rows as in rl_exact_set*; NULL clears
 * them), added to the diagonal wherever the per-output noise is: rl_exact_assemble and
 * rl_exact_dense_host.  The noise-free cross-covariances (rl_exact_cross_*,
 * rl_exact_explained_variance's right-hand sides) do not see them.  Kept on the handle across
 * rl_exact_set* calls; a matrix assembled or factored before the call is dropped.  The noise
 * slot of rl_exact_grad_sums stays the sum of M_ii per output.  RL_EINVAL: a negative or
 * non-finite value.  (Joined ABI version 8 without a bump.)                                    */
int rl_exact_set_row_noise(rl_exact* h, const double* extra);
/* K into the device buffer (lower triangle; rl_exact_factor does it when needed). */
int rl_exact_assemble(rl_exact* h);
/* Blocked Cholesky K = L L^T in place (cho_factor, likelihood.py:153) and
 * *logdet = 2 sum log L_ii (models/interpolated_llgp.py:262-276), summed in a fixed order.  A pivot
 * that is not a positive finite number returns RL_ENOTPD with *bad_col = its column (else -1);
 * the handle keeps its parameters and can be set and factored again.                           */
int rl_exact_factor(rl_exact* h, double* logdet, int* bad_col);
/* X[v] = K^-1 B[v] (cho_solve, exact_deriv.py:18-19), B, X dev [nrhs][n] (may alias).        */
int rl_exact_solve(rl_exact* h, const double* B, double* X, int nrhs, void* stream);
/* out[t] = || L^-1 K(X, x_t) ||^2 = diag(K_*X K^-1 K_X*) for test rows Xtest host [nt][P] of
 * outputs test_lens [D] (interpolated_llgp.py:350-356); out host [nt].  Needs the factor.      */
int rl_exact_explained_variance(rl_exact* h, const double* Xtest, const int* test_lens, double* out);
/* The noise-free cross-covariance K(Xtest, X), out host [nt][n]
 * (ExactLMCLikelihood.kernel_from_indices, likelihood.py:176-199).  Needs only rl_exact_set.    */
int rl_exact_cross_host(rl_exact* h, const double* Xtest, const int* test_lens, double* out);
/* nrows of those rows, K(Xtest[row0 : row0 + nrows], X), into the DEVICE buffer out dev [nrows][n]
 * in the operator's row order: the right-hand sides of the predictive variances, which the
 * reference builds on the host and hands to its solver one by one
 * (models/interpolated_llgp.py:358-397).  Xtest host [nt][P] and test_lens host [D] describe ALL
 * test points (nt = sum test_lens), as in rl_exact_cross_host; only the window's rows are copied,
 * during the call.  The kernel (csrc/rl_exact.h: k_ex_cross_rows, written for few rows by many
 * columns; entries as rl_exact_cross_host's) is queued on `stream`.  Needs only rl_exact_set and
 * allocates O(nrows P) on the handle, nothing of size n^2.  RL_EINVAL: NULL, row0 + nrows > nt,
 * no parameters; RL_ELIMIT: P + Q D > 4096 (one test row must fit the kernel's LDS).            */
int rl_exact_cross_dev(rl_exact* h, const double* Xtest, const int* test_lens, int row0, int nrows,
                       double* out, void* stream);
/* The reduction of those variances, fused: dots[v] = sum_i B[v][i] X[v][i] (the np.einsum /
 * diagonal of interpolated_llgp.py:358-397 once X[v] = K~^-1 B[v]) and sqnorms[v] = sum_i X[v][i]^2
 * in ONE pass over B, X dev [nvec][n]; dots, sqnorms dev [nvec]; ws dev [nvec][RL_ROW_DOTS_WS]
 * partial sums.  Two stages in a fixed order, no atomics: bit-identical from call to call.
 * Queued on `stream` of the current device; nvec <= 65535 (RL_ELIMIT).                          */
#define RL_ROW_DOTS_WS 128
int rl_row_dots(const double* B, const double* X, int nvec, long long n, double* dots,
                double* sqnorms, double* ws, void* stream);
/* The whole K, out host [n][n] (likelihood.py:149-151; interpolated_llgp.py:248-260).  Built
 * anew in row panels: valid in any state after rl_exact_set, O(n^2) host memory.               */
int rl_exact_dense_host(rl_exact* h, double* out);
/* K^-1 (lower) in place of the factor: L^-1 (blocked trtri), then L^-T L^-1 (blocked lauum).
 * Afterwards rl_exact_solve / rl_exact_explained_variance need rl_exact_factor again.          */
int rl_exact_invert(rl_exact* h);
/* Gradient block sums of the exact likelihood (the loops of likelihood.py:48-96 over
 * exact_deriv.py:13-23), with M = alpha alpha^T - K^-1 (never formed):
 *   out[s][a][b] = sum_{i in a, j in b} M_ij v_s(i, j)   for s < S = Q + sum_q p_q:
 *                  v_q = k_q (s = q), then dk_q / dtheta_p (s = Q + sum_{q' < q} p_q' + p);
 *   out[S D^2 + d] = sum_{i in d} M_ii.
 * alpha dev [n] (= K^-1 y); out host [S D^2 + D].  Inverts first if needed.  Bit-identical from
 * call to call (fixed reduction order).  dL/dtheta = 1/2 sum_ab dB[a, b] out[s][a][b].           */
int rl_exact_grad_sums(rl_exact* h, const double* alpha, double* out);

/* ---- function draws (pathwise sampling) -------------------------------------
 * No reference twin: the reference predicts means and marginal variances only
 * (models/interpolated_llgp.py:293-397).  A draw of the grid prior
 *     u ~ N(0, K_UU),   K_UU = sum_q B_q (x) T_q,   B_q = A_q^T A_q + diag(kappa_q)
 * is  u = sum_q (F_q (x) S_q) z_q  with white noise z_q, the D x C_q "channel" matrix
 * F_q = [A_q^T, diag sqrt(kappa_q)] (F_q F_q^T = B_q; no factorisation of B_q, exact for
 * R_q = 0 and singular B_q) and S_q S_q^T = T_q in one of two forms per top row:
 *   form 0, circulant embedding of the EXTENDED row: the kernel itself evaluated at lags
 *     0 .. Ls/2 (1-D) or on the (N1s/2 + 1) x (N2s/2 + 1) lag lattice (2-D), mirrored to a
 *     circulant of length Ls (N1s x N2s), whose real spectrum lambda is clipped at zero.  One
 *     complex inverse transform makes TWO independent draws: with xi = z_{2p} + i z_{2p+1},
 *         Y_a(w) = sum_q sqrt(lambda_q(w) / Ls) sum_c F_q[a][c] xi_{q,c}(w),
 *         y = sum_w Y(w) exp(+2 pi i w x / Ls)  cropped to the grid,
 *     Re y is draw 2p and Im y draw 2p + 1 (w = w1 * N2s + w2 and Ls -> N1s N2s on 2-D grids).
 *   form 1, polynomial rows (1-D grids; rl_gridop_top_forms reports 1): S_q = Phi_r G_q with
 *     G_q G_q^T = C_q clipped at zero (the caller's eigendecomposition of rl_gridop_poly_coeffs'
 *     C_q, r <= 48), r reals of noise per channel and draw.
 * Noise layout: one draw's noise is zlen doubles: the rows q = 0 .. Q-1 one after another,
 * row q holding C_q channels of len_q values each (channel-major: offset c * len_q + w), len_q =
 * Ls (N1s * N2s) for form 0 and r for form 1.  The noise of draw s for a form-0 row is used
 * together with its pair partner's (s ^ 1), so Z always holds 2 ceil(nsamp / 2) rows, a
 * trailing odd draw's partner included.
 * The sampler's lengths are its own (not the product handle's L): an embedding that clips
 * nothing often needs a multiple of 2m.  Allowed lengths are odd * 2^k, odd in
 * {1, 3, 5, 9, 15, 25}, k >= 1, at most 2^22 (at most 2048 per axis of a 2-D grid; RL_ELIMIT
 * beyond); rl_sampler_length gives the smallest one >= want.
 * Up to RL_SAMPLER_LDS_MAX points the transform of a 1-D pair runs inside one launch
 * (k_smp_embed1, the transform in LDS); longer ones and 2-D grids in two (k_smp_cols: scale,
 * mix and the first pass; k_smp_rows: the second pass and the crop; csrc/rl_sample.h).      */
typedef struct rl_sampler rl_sampler;
#define RL_SAMPLER_LDS_MAX 2048
int rl_sampler_length(long long want, int* length);
/* Borrows the grid handle as rl_ski_create does (D, the grid's shape, the polynomial basis):
 * destroy the sampler BEFORE its grid operator.                                             */
int rl_sampler_create(rl_gridop* g, rl_sampler** out);
int rl_sampler_destroy(rl_sampler* h);
/* Parameters of the draws (per parameter update of the model):
 *   nchan     host [Q]            C_q >= 1
 *   F         host                the Q blocks [D][C_q] one after another
 *   forms     host [Q]            0 / 1 as above
 *   N1s, N2s  the embedding: 1-D grids N1s = Ls, N2s = 0; 2-D grids one length per axis
 *             (ignored when no row has form 0); N_k / 2 >= m_k - 1
 *   ext_rows  host                for every form-0 row in order its N1s/2 + 1 kernel values
 *                                 (2-D: [(N1s/2 + 1)][(N2s/2 + 1)])
 *   poly_rank, poly_sqrt  host    for every form-1 row in order G_q, [r][r] row-major, r =
 *                                 poly_rank = the rank rl_gridop_poly_coeffs reported
 *   clipped   host [Q] out        sum |lambda_-| / sum |lambda| of every form-0 row (0 for
 *                                 form 1: the caller knows what it clipped); may be NULL
 *   zlen      out                 doubles of noise per draw
 * The host computes the spectra (a mixed-radix transform, O(Ls log Ls)).  Form 1 reads the
 * grid handle's basis: the grid's parameters must be those poly_sqrt was derived from.       */
int rl_sampler_set(rl_sampler* h, int Q, const int* nchan, const double* F, const int* forms,
                   int N1s, int N2s, const double* ext_rows, int poly_rank,
                   const double* poly_sqrt, double* clipped, long long* zlen);
/* The clipped spectrum lambda_+ the draws of form-0 row q use, natural frequency order, host
 * out [Ls] ([N1s][N2s]) (test hook, as rl_gridop_spectrum_host; RL_EINVAL for a form-1 row).  */
int rl_sampler_spectrum_host(const rl_sampler* h, int q, double* out);
/* U[s] = one draw of N(0, K_UU) from the noise rows Z: Z dev [2 ceil(nsamp / 2)][zlen],
 * U dev [nsamp][D*m].  Linear in Z; queued on `stream`.                                     */
int rl_sampler_draw(rl_sampler* h, const double* Z, double* U, int nsamp, void* stream);
/* Standard normal noise from a counter-based generator (splitmix64 mixing, Box-Muller in
 * fp64): Z[i][j], i < ndraws, j < zlen, is a function of (seed, draw0 + i, j) ONLY, so a draw
 * does not depend on how draws are tiled or how many are asked for.  Z dev [ndraws][zlen].
 * Queued on `stream` of the CURRENT device (no handle names one, as rl_row_dots): a process
 * with several devices selects Z's device before the call.                                   */
int rl_normal_fill(unsigned long long seed, long long draw0, int ndraws, long long zlen,
                   double* Z, void* stream);
/* R[s][i] = y[i] - WU[s][i] - sqrt_eps_rows[i] * E[s][i]: the right-hand sides of Matheron's
 * rule (y dev [n], sqrt_eps_rows dev [n]: sqrt of the noise of each data row; WU, E, R dev
 * [nsamp][n]; R may alias WU or E).  Queued on `stream` of the current device, as above.      */
int rl_pathwise_residual(const double* y, const double* WU, const double* E,
                         const double* sqrt_eps_rows, double* R, int nsamp, long long n,
                         void* stream);

/* ---- Leave-one-out cross-validation (csrc/rl_loo.h; no reference twin) -------------------------
 * With alpha = K~^-1 y and d = diag(K~^-1), observation i predicted from all the others has mean
 * y_i - alpha_i / d_i and variance 1 / d_i (Rasmussen & Williams 5.4.2).
 *
 * rl_ski_inverse_diag: out dev [n], caller's row order = the diagonal of the inverse of the matrix
 *   rl_ski_factor factorised, in ONE pass over the table of F (k_dz_diag) and no solve:
 *   *exact = 1: diag(K~^-1) (*available = 1); *exact = 0: diag(P^-1) of the preconditioner
 *   (*available = 2).  Rebuilds the factorisation after parameter / noise updates first.
 *   RL_ELIMIT with the reason in rl_last_error() when *available is 0, or 3 (the 96-function basis
 *   keeps its map in blocks).  Queued on `stream`.
 * rl_ski_precond_apply: X = P^-1 B, ONE application of the factorisation (what rl_solve_pcg applies
 *   every iteration; K~^-1 B to roundoff when *available = 1).  B, X dev [nvec][n], caller's row
 *   order, not aliased.  *available 1, 2 and 3; RL_ELIMIT for 0.
 * rl_diag_accumulate: with t = Z[v][i] (X[v][i] - C[v][i]), v ascending:  sum[i] += t,
 *   sumsq[i] += t^2  (Z, X, C dev [nvec][n]; C may be NULL = 0; sum, sumsq dev [n], distinct).
 *   Every entry's order over v is fixed, so probes accumulated in tiles of any size give the same
 *   bits.  Queued on `stream` of the current device, as rl_row_dots.
 * rl_loo_reduce: mean = y - alpha / d, var = 1 / d (dev [n]) and the log densities
 *   -log(2 pi var) / 2 - (y - mean)^2 / (2 var) - logscale[i]  (logscale dev [n] or NULL = 0) summed
 *   per block in a fixed order: logp_partials dev [2][RL_LOO_PARTIALS], [0][b] block b's sum over
 *   its valid rows, [1][b] its count of rows whose d is not a positive finite number (those rows
 *   get mean = var = NaN and stay out of the sum: reported, not clamped); *nblk = blocks used.  The
 *   caller adds the *nblk partial sums in order.  Outputs may not alias inputs or each other.
 *   Queued on `stream` of the current device.                                                   */
#define RL_LOO_PARTIALS 256
int rl_ski_inverse_diag(rl_ski* s, double* out, int* exact, void* stream);
int rl_ski_precond_apply(rl_ski* s, const double* B, double* X, int nvec, void* stream);
int rl_diag_accumulate(const double* Z, const double* X, const double* C, int nvec, long long n,
                       double* sum, double* sumsq, void* stream);
int rl_loo_reduce(const double* y, const double* alpha, const double* dinv, const double* logscale,
                  long long n, double* mean, double* var, double* logp_partials, int* nblk,
                  void* stream);

/* ---- Pivoted-Cholesky preconditioner (csrc/rl_pivchol.h; no reference twin) ------------------
 * rl_ski_factor reports *available = 0 for every operator without the polynomial form: 2-D and 3-D
 * grids, kernels on several grids, D > 16, rows whose spectrum the polynomial subspace does not
 * hold.  The standard preconditioner of such operators needs their product and their diagonal only:
 *     P = L L^T + E,   L (n x k) the rank-k pivoted (greedy, largest residual diagonal first)
 *     Cholesky factor of the kernel part  sum_t W_t K_t W_t^T,   E = diag(eps),
 *     P^-1 r = E^-1 r - E^-1 L G^-1 L^T E^-1 r,   G = I + L^T E^-1 L  (k x k, host Cholesky G = C C^T),
 *     log det P = sum_i log eps_i + 2 sum_j log C_jj.
 * Opt-in per handle, nothing changes without it:
 * rl_ski_set_pivchol: rank 0 .. 256 (RL_EINVAL beyond), 0 = off (the default), clipped to n at the
 *   build; rel_tol in [0, 1): a step whose pivot d_p <= rel_tol max_i d_i^(0) ends the factor (zero
 *   columns from there on; 1e-10 is the usual value: the residual is then roundoff of the product).
 * With a rank set, rl_ski_factor still prefers the polynomial factorisation (*available 1, 2, 3 as
 * before, bit for bit); only where it would report 0 it builds P and reports *available = 4,
 * *logdet = 0 (P is not K~; rl_ski_precond_sample gives log det P), *cond = the squared pivot ratio
 * of chol(G).  The build runs once per parameter / noise update (k single-vector products, no host
 * synchronisation between them; every sum in a fixed order: two builds of one operator give the
 * same bits) and is cached on the handle.  The only condition on the noise: positive (it need not
 * be constant per output).  Zero noise: *available = 0 with the reason.
 * In mode 4 rl_solve_pcg, rl_solve_pcg_lanczos, rl_ski_precond_apply and rl_ski_precond_sample work
 * as in modes 2 and 3 (the sample map is S = E^1/2 + L Ms L^T E^-1/2 with S S^T = P: when the Gram
 * matrix L^T E^-1 L is numerically singular the trailing columns of L are dropped until its Cholesky
 * holds, and the reduced rank is reported); rl_solve_direct, rl_ski_project and
 * rl_ski_inverse_diag answer RL_ELIMIT and name the pivoted-Cholesky preconditioner.
 * Test readouts (RL_ELIMIT unless the handle is in mode 4; any pointer may be NULL):
 * rl_ski_pivchol_info: *rank_used = columns in use; pivots host [min(rank, n)]: the pivot rows in
 *   the caller's numbering; pivot_values host [min(rank, n)]: the residual diagonal at each pivot
 *   when it was chosen; resid_diag_dev dev [n], caller's row order: the residual diagonal after
 *   the last step.
 * rl_ski_pivchol_factor: L_dev dev [rank_used][n], caller's row order: the factor's columns.
 * rl_ski_pivchol_build_ms: host out3 = milliseconds of the last build on the host's clock:
 *   diagonal; the k products with their step kernels; Gram matrix and host maps.               */
int rl_ski_set_pivchol(rl_ski* s, int rank, double rel_tol);
int rl_ski_pivchol_info(rl_ski* s, int* rank_used, int* pivots, double* pivot_values,
                        double* resid_diag_dev);
int rl_ski_pivchol_factor(rl_ski* s, double* L_dev);
int rl_ski_pivchol_build_ms(rl_ski* s, double* out3);

#ifdef __cplusplus
}
#endif
#endif /* RUNLMC_HIP_H */
