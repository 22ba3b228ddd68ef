/*
 * hs_kernels.h -- kernel-level test hooks of libhs_solver (used by tests/ only).
 *
 * These drive the same HIP kernels the hot path (hs_factor_* / hs_ldiv_* in hs_solver.h) launches,
 * on caller-supplied dense host data, so each kernel can be checked against the oracle alone.
 * Column-major everywhere; complex = interleaved (re, im) doubles (Julia ComplexF64).
 */
#ifndef HS_KERNELS_H
#define HS_KERNELS_H
#include <stdint.h>
#include "hs_solver.h"
#ifdef __cplusplus
extern "C" {
#endif

/* C = C - A*B (minus != 0) or C = A*B (minus == 0) with the MFMA GEMM kernel
 * (the contraction of src/factorization.jl:40,72 and src/blockmatrix.jl:97,118).
 * repeat > 0 additionally times `repeat` back-to-back launches (ms per launch in *ms_out). */
int hsk_gemm_d(int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb,
               double* C, int64_t ldc, int minus, int repeat, double* ms_out);
int hsk_gemm_z(int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb,
               double* C, int64_t ldc, int minus, int repeat, double* ms_out);

/* Eliminate the first ni DOFs of `count` dense fronts F[k] ((ni+nb) x (ni+nb), front order [int; bnd]):
 * the per-front work of _factor_leaf / _factor_branch (src/factorization.jl:30-42, 62-75).
 *   outLF  (ni+nb) x ni : [L\U of P*Aii ; Abi*U^-1]      outUR  ni x nb : L^-1*P*Aib
 *   outSB  nb x nb      : Abb - Abi*Aii^-1*Aib           out_rperm ni   : (P x)[i] = x[rperm[i]] (0-based)
 *   info[k]             : 0, or 1 + first column with an exactly zero pivot */
int hsk_front_factor_d(int64_t count, int64_t ni, int64_t nb, const double* F, double* outLF, double* outUR,
                       double* outSB, int64_t* out_rperm, int64_t* info, double* ms_out);
int hsk_front_factor_z(int64_t count, int64_t ni, int64_t nb, const double* F, double* outLF, double* outUR,
                       double* outSB, int64_t* out_rperm, int64_t* info, double* ms_out);

/* The same elimination for a batch of `count` fronts of their own sizes ni[k], nb[k] (F packed column-major, one front after another),
 * scheduled as hs_numeric schedules a level.  mode 0: tournament pivoting, no solve descriptors (hsk_front_factor_*); 1: optimistic
 * pivoting, no descriptors; 2: optimistic pivoting with descriptors (the default path: diagonal-block-first 256-column groups and the
 * inverses of the 256 x 256 diagonal blocks); 3: tournament pivoting with descriptors (a redone level).  Every output may be null; each is
 * packed per front in batch order: outLF m x ni, outUR ni x nb, outSB nb x nb, out_rperm ni, info[k], growth[k] (1: optimistic
 * pivoting met a multiplier above HS_GROWTH_MAX = 4, a NaN multiplier or a diagonal block singular on its own rows), outInvL / outInvU
 * ceil(ni/32) column-major 32 x 32 inverses of the diagonal blocks of L (unit lower) and U, outInv256L / outInv256U ceil(ni/256)
 * 256 x 256 ones (modes 2 and 3 only).
 * mode + 4 (bit 2; mode & 3 is the mode above): the batch runs with Sched::aligned16 = true, as hs_numeric runs the dense batch of a level --
 * the hook lays LF / UR / SB out at multiples of 32 elements with even leading dimensions, so the Float64 plain updates go to
 * gemm_op_lds_kernel or the edge kernels wherever hs_gemm_lds_route allows (hsk_gemm_lds_enable still decides).  ComplexF64 accepts the bit
 * and runs what it runs without it.  Modes outside 0..7: HS_ERR_ARGUMENT.
 *   hsk_lookahead_runs : batches that Sched::factor_fronts has sent to the look-ahead schedule (factor_fronts_lookahead: maxni >= HS_LA_MIN,
 *                        block columns of HS_LA_NB, a side stream) since the last call with reset != 0; process-wide, counted on the host,
 *                        factorizations through hs_numeric included. */
long long hsk_lookahead_runs(int reset);
int hsk_front_batch_d(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, double* outLF, double* outUR,
                      double* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth, double* outInvL, double* outInvU,
                      double* outInv256L, double* outInv256U, double* ms_out);
int hsk_front_batch_z(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, double* outLF, double* outUR,
                      double* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth, double* outInvL, double* outInvU,
                      double* outInv256L, double* outInv256U, double* ms_out);
/* hsk_front_batch_d with block envelopes made by the caller (optimistic modes 1, 2, with or without bit 2): env holds, per front in batch
 * order, firstL then firstU, ceil(ni/32) + ceil(nb/32) entries each, as hsk_leaf_envelope lays them out; the caller vouches that every entry
 * of F outside them is zero.  The batch then runs as hs_numeric runs a level whose fronts carry tables (Sched::env).  env == NULL: dense. */
int hsk_front_batch_env_d(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, const int32_t* env, double* outLF,
                          double* outUR, double* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth);
/* hsk_front_batch_{d,z} with the symmetric schedule (Sched::sym, hs_options.symmetric): the caller vouches that every front equals its plain
 * transpose.  Same arguments and outputs; modes 1, 2 and 2 | 4 only (the schedule needs optimistic pivoting), any other mode: HS_ERR_ARGUMENT. */
int hsk_front_batch_sym_d(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, double* outLF, double* outUR,
                          double* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth, double* outInvL, double* outInvU,
                          double* outInv256L, double* outInv256U, double* ms_out);
int hsk_front_batch_sym_z(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, double* outLF, double* outUR,
                          double* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth, double* outInvL, double* outInvU,
                          double* outInv256L, double* outInv256U, double* ms_out);

/* One tree level of ldiv!: the batch of hsk_front_batch_* (same packing of ni, nb, F), factored in mode 2 or 3 so that the stored inverses are
 * the production ones, then the level's forward and backward sweeps on the global vector b (length n), through the per-level driver that
 * ldiv! (N), ldiv!(transpose(F), .) and ldiv!(adjoint(F), .) call for every level, without the low-rank and HSS parts.
 *   flags[k] (NULL: all 0)  bit 0 `compressed`: the descriptor carries compressed = 1, mrows = ni (the dense sweeps leave the front's boundary
 *                           alone and the backward sweep starts from v = y); bit 1 `blank`: after the factorization the descriptor gets
 *                           ni = nb = m = mrows = 0 (a front whose interior block is an HSS matrix): the sweeps skip it
 *   fidx                    the global ids (0-based, < n) of every front, m = ni + nb per front in front order [int; bnd], one front after
 *                           another; no id may occur twice (the fronts of a level are disjoint)
 *   path                    0: dataflow sweeps, one launch per level and direction; 1: 256 columns per launch; 2: 32 columns per launch
 *                           (trans = 0 only)
 *   trans                   0: N, 1: T, 2: H (ComplexF64 only; Float64 refuses it: use 1)
 *   tall                    -1: the forward dataflow sweep chooses its boundary tiles by its own rule (hsk_flow_tall_rule), 0 / 1: forced
 *                           (path 0, trans 0; ignored elsewhere)
 * The work vectors are laid out as hs_analyze lays them out (packed: woff += ni, poff += ceil(nb/512) * ni).  Per call: forward sweep
 * (gather, sweep), y = the level's solved vector (sum of ni entries, packed per front; T / H: z) and b_fwd = b after it; backward sweep on
 * those (interior update, sweep, scatter), x (packed like y) and b_bwd.  outLF .. outInv256U as in hsk_front_batch_*.  *tall_used: the tile
 * shape the forward sweep ran with (0 when path != 0 or trans != 0).  Every output may be null.
 * HS_ERR_ARGUMENT before any device work and with the outputs untouched: mode outside 2..3, path / trans / tall out of range, path = 2 with
 * trans != 0, trans = 2 for Float64, an id outside [0, n) or one that occurs twice.  HS_ERR_DEVICE: a workgroup of a dataflow sweep ran
 * out of its bounded wait (checked after each direction; nothing is launched after it). */
int hsk_sweep_level_d(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, const int64_t* flags, int64_t n,
                      const int64_t* fidx, const double* b, int path, int trans, int tall, double* outLF, double* outUR, int64_t* out_rperm,
                      int64_t* info, int64_t* growth, double* outInvL, double* outInvU, double* outInv256L, double* outInv256U, double* y,
                      double* b_fwd, double* x, double* b_bwd, int* tall_used);
int hsk_sweep_level_z(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, const int64_t* flags, int64_t n,
                      const int64_t* fidx, const double* b, int path, int trans, int tall, double* outLF, double* outUR, int64_t* out_rperm,
                      int64_t* info, int64_t* growth, double* outInvL, double* outInvU, double* outInv256L, double* outInv256U, double* y,
                      double* b_fwd, double* x, double* b_bwd, int* tall_used);
/* The rule by which the forward dataflow sweep of a level of nbatch fronts with at most maxnb boundary DOFs takes tall boundary tiles
 * (1) or not (0); -1 for arguments out of range.  Host only. */
int hsk_flow_tall_rule(int is_complex, int64_t nbatch, int64_t maxnb);
/* The `path` ldiv! takes in this process, read once from the environment: 0 dataflow (the default; HS_SOLVE_FLOW unset or not 0, whatever
 * HS_SOLVE_WIDE says), 1 (HS_SOLVE_FLOW=0) 256 columns per launch, 2 (HS_SOLVE_FLOW=0 HS_SOLVE_WIDE=0) 32 columns per launch.  Host only. */
int hsk_sweep_path(void);

/* Low-rank compression X (rows x cols) ~= C (rows x r) * Z (r x cols) to tolerance max(atol, rtol*|u_11|): the
 * device primitive behind the compressed Gauss transforms (`_lgauss_transform` / `_rgauss_transform`,
 * src/factorization.jl:171-182, which call LowRankApprox.pqrfact).  cap = capacity (in columns of C / rows of Z)
 * of the output arrays; kinit = initial sketch width. */
int hsk_lowrank_d(int64_t rows, int64_t cols, const double* X, double atol, double rtol, int64_t kinit, int64_t seed,
                  int64_t* r_out, double* Cout, double* Zout, int64_t cap);
int hsk_lowrank_z(int64_t rows, int64_t cols, const double* X, double atol, double rtol, int64_t kinit, int64_t seed,
                  int64_t* r_out, double* Cout, double* Zout, int64_t cap);

/* The rank-revealing orthogonalisation behind every HSS rank and interpolation matrix (qr_refine, csrc/hs_hss.hip), piece by piece
 * (tests/qr_mirror.py restates it; tests/test_qr_refine_gpu.py).  W = 64 below is the window width hsk_qr_params reports.
 *   hsk_qr_params : out4 = window width (HS_QW), conditioning cut-off (HS_CHOL_COND), theta (HS_QR_THETA), noise_rel (HS_NOISE_REL) as this
 *                   process runs them.  Host only.
 *   hsk_qr_chol_* : chol_block_kernel on njobs windows in one launch.  Per job a: b[a] in 1..W candidates, their Gram matrix G + a*W*W
 *                   (column-major, leading dimension W), first[a], thr + 5*a = (atol [already times atol_scale], rtol, scale_floor, floor_abs,
 *                   next2 [negative: none]), top[a] (read when first[a] == 0, written when it is not), p + a*W (b candidates, re-ordered in
 *                   place: accepted first).  Outputs, W x W each with leading dimension W: L, Linv, LinvP; d + a*W, lperm + a*W, nacc[a].
 *                   Every output array is read first: what the kernel does not write comes back as it went in.
 *   hsk_qr_select : qr_select_kernel on njobs lists in one launch.  Per job: m, done (0..m), want (1..W); p (m entries of 0..m-1) and res2
 *                   (m doubles) packed one job after another; outmax + 2*a.
 *   hsk_qr_refine_* : one qr_refine call on njobs blocks.  Packed one job after another: M (m x q column-major, leading dimension m), p and d
 *                   (m entries per job; p a permutation of 0..m-1, with norm_select the identity), T ((m - r) x r column-major, leading
 *                   dimension m - r, in a slot of m * min(m, q)), blocks ((offset, width) pairs in a slot of 2*m ints), nblocks[a].
 *                   counters[0] = windows run, counters[1] = residual-norm recomputations, over the whole call. */
int hsk_qr_params(double* out4);
int hsk_qr_chol_d(int64_t njobs, const int32_t* b, const int32_t* first, const double* G, const double* thr, double* top, int32_t* p, double* L,
                  double* Linv, double* LinvP, double* d, int32_t* lperm, int32_t* nacc);
int hsk_qr_chol_z(int64_t njobs, const int32_t* b, const int32_t* first, const double* G, const double* thr, double* top, int32_t* p, double* L,
                  double* Linv, double* LinvP, double* d, int32_t* lperm, int32_t* nacc);
int hsk_qr_select(int64_t njobs, const int32_t* m, const int32_t* done, const int32_t* want, int32_t* p, const double* res2, double* outmax);
int hsk_qr_refine_d(int64_t njobs, const int32_t* m, const int32_t* q, const double* M, int32_t* p, const int32_t* rmax, const double* atol_scale,
                    const double* floor_abs, int norm_select, double atol, double rtol, double scale_floor, int32_t* r, double* top, double* d,
                    double* T, int32_t* blocks, int32_t* nblocks, int64_t* counters);
int hsk_qr_refine_z(int64_t njobs, const int32_t* m, const int32_t* q, const double* M, int32_t* p, const int32_t* rmax, const double* atol_scale,
                    const double* floor_abs, int norm_select, double atol, double rtol, double scale_floor, int32_t* r, double* top, double* d,
                    double* T, int32_t* blocks, int32_t* nblocks, int64_t* counters);

/* The tall-skinny panel product of the block solves (kernels_solve_multi.hip) on host data: C = A X (minus == 0) or C = C - A X, A M x K
 * (column-major, lda), X K x kc and C M x kc column-major with kc in 1..64 (they reach the kernel row-major with a pitch of 64, as the work
 * blocks of hs_ldiv_block_* do).  trap != 0: A stands for its unit lower trapezoid.  map (NULL: none): M entries in 0..M-1, row i of the
 * product belongs to row map[i] of C (the kernel's cmap: C[map[i], :] = C[map[i], :] - (A X)[i, :]); an entry outside that range gives
 * HS_ERR_ARGUMENT. */
int hsk_multi_prob_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                     int minus, int trap, const int32_t* map);
int hsk_multi_prob_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                     int minus, int trap, const int32_t* map);

/* The panel product of the transposed block solves (kernels_solve_multi_t.hip) on host data: C = op(A)^T X (minus == 0) or C = C - op(A)^T X,
 * A K x M (column-major, lda >= K), X K x kc and C M x kc column-major with kc in 1..64 (row-major with a pitch of 64 on the device).
 * trap != 0: A stands for its unit lower trapezoid (K x M); conj != 0: op = conj (ComplexF64; ignored for Float64).  map (NULL: none): K
 * entries in 0..K-1, row k of A meets row map[k] of X (the kernel's xmap: C = C - op(A)^T X[map, :]); an entry outside that range gives
 * HS_ERR_ARGUMENT. */
int hsk_multi_prob_t_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                       int minus, int trap, int conj, const int32_t* map);
int hsk_multi_prob_t_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                       int minus, int trap, int conj, const int32_t* map);

/* One triangular product of hs_mul_* (kernels_solve_multi_mul.hip) on host data, staged like hsk_multi_prob_*: C = tri(A) X (plus == 0) or
 * C = C + tri(A) X, A M x K (column-major, lda), X K x kc, C M x kc, kc in 1..64.  tri = 1: the unit lower trapezoid of A (entries above the
 * diagonal and the diagonal itself are not used), tri = 2: its upper triangle with the diagonal (entries below it are not used); the
 * kernel does not read a 16-column chunk that lies wholly in the unused part for a workgroup's rows.  map (NULL: none): M entries in
 * 0..M-1, row i of the product belongs to row map[i] of C. */
int hsk_multi_tri_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                    int plus, int tri, const int32_t* map);
int hsk_multi_tri_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                    int plus, int tri, const int32_t* map);
/* The transposed counterpart: C = op(tri(A))^T X or C + op(tri(A))^T X with A K x M (column-major, lda >= K), tri as above (of the K x M
 * matrix), conj != 0: op = conj (ComplexF64).  map (NULL: none): K entries in 0..K-1, row k of A meets row map[k] of X. */
int hsk_multi_tri_t_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                      int plus, int tri, int conj, const int32_t* map);
int hsk_multi_tri_t_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                      int plus, int tri, int conj, const int32_t* map);

/* The two panel products over a Float32 panel (kernels_solve_multi_f32.hip; hs_f32_*, include/hs_solver.h) on host data: the arguments of
 * hsk_multi_prob_* / hsk_multi_prob_t_*.  A is given in Float64 (ComplexF64) and demoted on the device by the library's demotion kernel
 * (round to nearest even, real and imaginary parts separately) before the product reads it; X, C and the accumulation stay Float64.  On
 * the same rounded values the result has the bits of hsk_multi_prob_* / hsk_multi_prob_t_*. */
int hsk_multi_prob_f32_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                         int minus, int trap, const int32_t* map);
int hsk_multi_prob_f32_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                         int minus, int trap, const int32_t* map);
int hsk_multi_prob_t_f32_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                           int minus, int trap, int conj, const int32_t* map);
int hsk_multi_prob_t_f32_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc,
                           int minus, int trap, int conj, const int32_t* map);
/* Rounds IN PLACE, through the job list and the conversion of hs_f32_create, every stored element of F that a demoted copy would hold:
 * x <- (double)(float)x.  F stays an ordinary Float64 handle (to be thrown away afterwards): hs_ldiv_block_t_* on it returns the bits
 * hs_f32_ldiv_* returns on a copy demoted from the unrounded factors.  counts2 = {elements finite in Float64 that overflow Float32 (they
 * become +-Inf here), nonzero elements that became zero or subnormal}.  Refuses what hs_f32_create refuses of the handle. */
int hsk_round_factors_f32(hs_handle* F, int64_t* counts2);

/* The product of hs_interface_matrix_* (kernels_interface.hip) on host data: S[rperm[i], j] = sum over k <= min(i, j) of L[i, k] U[k, j] for the
 * packed factors LF (nb x nb, column-major, ldl >= nb; unit lower L below the diagonal, U on and above it), rperm nb distinct entries in
 * 0..nb-1 ((P x)[i] = x[rperm[i]]; an entry outside gives HS_ERR_ARGUMENT), S nb x nb column-major with lds >= nb (rows past nb are left as
 * they are).  *flops_out (may be NULL) = the real flops the launch executed on the matrix pipe, K padding included. */
int hsk_lu_product_d(int64_t nb, const double* LF, int64_t ldl, const int32_t* rperm, double* S, int64_t lds, double* flops_out);
int hsk_lu_product_z(int64_t nb, const double* LF, int64_t ldl, const int32_t* rperm, double* S, int64_t lds, double* flops_out);

/* ONE grouped launch of the product of the transposed ULV solves of the HSS module (kernels_ulv_t.hip) on host data.  Job i is described by
 * the ten entries desc[10 i ..]: M, K, N, lda, ldx, ldc, aoff, xoff, coff, flags.  A = Abuf + aoff is K x M column-major (lda >= K), X = Xbuf +
 * xoff K x N (ldx >= K), C = Cbuf + coff M x N (ldc >= M); offsets and buffer lengths (na, nx, nc) count elements (ComplexF64: pairs of
 * doubles).  flags bit 0: C = C - op(A)^T X (otherwise C = op(A)^T X); bits 1-2: 0 all of A, 1 only its entries k >= m, 2 only k <= m.
 * conj != 0: op = conj (ignored for Float64).  Jobs with M, K or N equal to 0 are skipped; their C is left as it is.  HS_ERR_ARGUMENT when a
 * job reaches outside its buffers; the C blocks of different jobs must be disjoint (the caller's concern). */
int hsk_ulv_t_group_d(int64_t njobs, const int64_t* desc, const double* Abuf, int64_t na, const double* Xbuf, int64_t nx, double* Cbuf, int64_t nc, int conj);
int hsk_ulv_t_group_z(int64_t njobs, const int64_t* desc, const double* Abuf, int64_t na, const double* Xbuf, int64_t nx, double* Cbuf, int64_t nc, int conj);

/* The CSR SpMM of hs_gmres_block_* (hs_gmres_block.hip) on host data: Y = A X (B == NULL) or Y = B - A X, A n x n CSC with 1-based colptr /
 * rowval, X, B, Y column-major n x nrhs blocks (ldx, ldb, ldy >= n; rows of Y beyond n are left as they are). */
int hsk_spmm_d(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* X, int64_t ldx, const double* B, int64_t ldb, double* Y,
               int64_t ldy, int64_t nrhs);
int hsk_spmm_z(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* X, int64_t ldx, const double* B, int64_t ldb, double* Y,
               int64_t ldy, int64_t nrhs);

/* The SpMM of hs_gmres_block_t_* over "entry ranges as rows" (hs_gmres_common.h) on host data: Y = op(A) X (B == NULL) or Y = B - op(A) X,
 * op by trans (0: A, through its CSR; 1: transpose(A), 2: adjoint(A), both through the CSC arrays of A read as rows, the adjoint conjugating
 * every value as it is loaded).  Arguments as hsk_spmm_*. */
int hsk_spmm_op_d(int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* X, int64_t ldx, const double* B, int64_t ldb,
                  double* Y, int64_t ldy, int64_t nrhs);
int hsk_spmm_op_z(int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* X, int64_t ldx, const double* B, int64_t ldb,
                  double* Y, int64_t ldy, int64_t nrhs);

/* The reduction kernel of hs_sens_* (kernels_sens.hip) on host data: a sampled dense-dense product over the CSC pattern colptr / rowval
 * (1-based, n columns, any order of the rows inside a column).  For every stored entry p = (i, j):
 *   G[p] <- G[p] - sum over c = 0 .. kc-1 of f(L[a, c]) * g(R[b, c]),   (a, b) = (i, j), or (j, i) with swap != 0,
 * f = conj with conjl != 0, g = conj with conjr != 0 (ComplexF64; ignored for Float64); L, R column-major n x kc (ldl, ldr >= n).  G holds
 * the initial values on entry (nnz elements).  One chain per entry, the columns in order, continued from G[p], every step the same unfused
 * expression: columns fed in several calls give the bits of one call.  diag != 0: G has n elements, G[j] continues its chain where (j, j) is
 * stored and is set to 0 where it is not.  form: 0 = one lane per entry reading the column-major blocks (what hs_sens_* runs), 1 = the blocks
 * transposed into row-major work blocks first (same bits; kept for measurements; ignored with diag).  seconds: NULL, or receives the median
 * device time of three runs (after one warm-up, on a copy of G; form 1: the two transpositions included). */
int hsk_sddmm_d(int64_t n, const int64_t* colptr, const int64_t* rowval, int64_t kc, const double* L, int64_t ldl, const double* R, int64_t ldr, int swap, int conjl,
                int conjr, int diag, int form, double* G, double* seconds);
int hsk_sddmm_z(int64_t n, const int64_t* colptr, const int64_t* rowval, int64_t kc, const double* L, int64_t ldl, const double* R, int64_t ldr, int swap, int conjl,
                int conjr, int diag, int form, double* G, double* seconds);

/* The right-hand side kernel of hs_tangent_* / hs_gn_hessvec_* (kernels_gn.hip) on host data: P = -op(E) X for a perturbation E on the CSC
 * pattern colptr / rowval (1-based, n columns, rows ascending within a column) and X column-major n x kc (ldx >= n); P is n x kc (ldp >= n,
 * the padding rows are left as they are).  pattern 0: E has nnz values in CSC order; op(E) = E, E^T, E^H for trans = 0 / 1 / 2 and
 *   P[i, c] = 0 - sum over the stored entries of row i of op(E), by ascending column of op(E), of op(E)[i, j] X[j, c],
 * one lane per row, every step the unfused acc - e * x.  pattern 1: E has n values, P[i, c] = 0 - e_i X[i, c] (e_i conjugated for trans = 2)
 * where (i, i) is stored, 0 elsewhere.  The hook builds the CSR map for trans = 0 on the host as the handle keeps it on the device. */
int hsk_gn_rhs_d(int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* E, int pattern, const double* X, int64_t ldx, int64_t kc, double* P,
                 int64_t ldp);
int hsk_gn_rhs_z(int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* E, int pattern, const double* X, int64_t ldx, int64_t kc, double* P,
                 int64_t ldp);
/* The row square sums of hs_gn_diag_* (kernels_gn.hip) on host data: acc[i] <- acc[i] + |X[i, c]|^2 for c = 0 .. kc-1 in order (Float64:
 * x * x; ComplexF64: re^2 + im^2), X column-major n x kc (ldx >= n), acc n doubles holding the initial values on entry.  One lane per row,
 * unfused: columns fed in several calls give the bits of one call. */
int hsk_gn_rowsq_d(int64_t n, int64_t kc, const double* X, int64_t ldx, double* acc);
int hsk_gn_rowsq_z(int64_t n, int64_t kc, const double* X, int64_t ldx, double* acc);

/* Host-only: the order in which the HSS form of a front's interior block lists its DOFs (hs_options.hss_d): recursive bisection of
 * the graph of A (1-based CSC pattern colptr / rowval of the n x n matrix) restricted to the ni DOFs `ids` (1-based), split where the
 * HSS cluster tree splits its index range.  perm_out[new position] = position in `ids` (0-based). */
int hsk_bisect_perm(int64_t n, const int64_t* colptr, const int64_t* rowval, int64_t ni, const int64_t* ids, int64_t* perm_out);

/* Accounting of the GROUPED MFMA products (`gemm_probs_kernel`: every product of the HSS module, of the low-rank compressions and of the
 * matrix-free fronts -- the flops of the compressed branch that `hs_stats.gemm_flops` (the fronts' `gemm_op_kernel`) does not see).
 *   hs_probs_stats_mode(0 | 1 | 2) : off / count flops and launches / also time every launch with a HIP event pair; resets the counters
 *   hs_probs_stats(out3)           : {real flops executed (complex: 8 M N K), launches, summed launch seconds}; synchronises the device
 * Process-wide (the products are issued from several host threads and streams). */
int hs_probs_stats_mode(int mode);
int hs_probs_stats(double* out3);

/* Block envelope of leaf and branch fronts (optimistic pivoting eliminates a front inside the envelope of its sparsity pattern, taken per
 * 32-row / 32-column block).
 *   hsk_leaf_envelope   : host only, no device.  The builder the analysis runs for every leaf: CSC pattern of A (1-based colptr / rowval, n
 *                         columns), fidx = ni + nb global ids (0-based) in front order [int; bnd]; firstL / firstU receive
 *                         ceil(ni / 32) + ceil(nb / 32) entries each (interior blocks first, boundary blocks counted from the start of the
 *                         boundary part): first interior column / row, rounded down to a multiple of 32, with a structural entry in the
 *                         block's rows / columns; 2^30 = none.  Returns 0, or -1 for a bad argument.
 *   hsk_branch_envelope : the same for a branch front [int1; int2 | bnd1; bnd2] with ni1 = |int1|, nb1 = |bnd1|: the pattern is every pair of
 *                         positions of the same child, the stored entries of A between the front's DOFs and the interior diagonal.
 *   hsk_branch_envelope_enable : 1 / 0 turns the branch fronts' tables alone on / off (default: on unless HS_BRANCH_ENVELOPE=0); returns the
 *                         previous setting.  Effective only while hsk_envelope_enable is on.
 *   hsk_envelope_enable : 1 / 0 turns the envelope on / off for the factorizations that follow (default: on unless HS_LEAF_ENVELOPE=0);
 *                         returns the previous setting.  Off, every front is eliminated as a dense matrix.
 *   hsk_op_flops_mode   : 1: the plain updates add the flops of the K-steps they really run to a device counter (one atomic per tile);
 *                         resets the counter.  Counting changes which kernel runs: while it is on, every plain update -- of dense fronts
 *                         too -- is launched as `gemm_op_env_kernel` (the same tile code; `gemm_op_kernel` holds no counter).
 *                         hsk_op_flops(out) reads the counter (synchronises the device): equals hs_stats.gemm_flops.
 *   hsk_env_order_enable : the tile order of the enveloped plain updates (HS_ENV_ORDER): 2 the K-sorted order (default: tiles of one K start
 *                         run side by side; Float64 fronts of at least 2048 tiles, every other launch runs 1), 1 the balanced order, 0 off -- an enveloped
 *                         launch maps block ids to tiles as a dense one does.  Returns the previous setting.  Which
 *                         workgroup runs a tile changes, never what the tile computes: every stored value keeps its bits.
 *   hsk_env_tile_order  : host only, no device.  For bid = 0 .. tiles_m * tiles_n - 1, the tile (tm[bid], tn[bid]) that block `bid` of a
 *                         launch with one workgroup per tile runs (first front of a batch), by the functions the kernels call; order 0 /
 *                         1 as the switch.  Blocks bid, bid + 8, ... share an XCD.  Returns 0, or -1 for a bad argument (a tile count outside
 *                         1 .. 32768, more than 2^24 tiles in all, a null pointer).
 *   hsk_env_phase_order : the same for the K-sorted order (2), host only: kr[tiles_m] / kc[tiles_n] are the K starts of the tile rows / columns
 *                         (0 .. 2^24), shift 0 .. 7 the XCD of the front's first block in a batched launch; at most 512 tile rows /
 *                         columns.  pos (may be null): the position of every block id in the sequence the tiles are dealt from.
 *                         Positions 64 u .. 64 u + 63 of the sequence, u below (tiles_m / 8) * (tiles_n / 8), are one unit
 *                         of 8 sorted tile rows x 8 sorted tile columns.
 *   hsk_env_perm        : the kernel that writes the tables of the K-sorted order, on one front (ni, nb; env: firstL then firstU as
 *                         hsk_leaf_envelope lays them out, or null) for the plain update (cmat, bmat, rows r0 .. r1, columns c0 .. c1,
 *                         k0 .. k1) as a factorization poses it; edge != 0: the tiling of the direct-to-LDS edge kernel (a front whose A
 *                         sits at an odd row is tiled from one row higher; Float64 only).  slot: tile rows / columns the tables hold, a
 *                         multiple of 8 in 8 .. 512.  out: 2 + 2 slot^2 + 2 slot + (slot / 8)^2 entries -- [0] 1 = valid (0: the front has
 *                         more tile rows or columns than the slot), from [2] the pairs (tile row, tile column) of block id 0, 1, ... of the
 *                         first front of a launch, then from [2 + 2 slot^2] rowperm[slot], colperm[slot] and the unit order.
 *   hsk_env_perm_slot_limit : caps the slot the factorizations and hooks that follow use (tests: fronts that do not fit take the balanced
 *                         order); returns the previous cap.
 *   hsk_env_perm_min_tiles : fronts with fewer tiles than this keep the balanced order under order 2 (HS_ENV_ORDER_MIN_TILES, default 2048);
 *                         a negative value restores the default.  Returns the previous limit.  hsk_env_perm itself applies none.
 *   hsk_env_perm_launches : enveloped updates that really ran the K-sorted order since the last reset (launches of the table kernel).  The
 *                         order runs on the Float64 direct-to-LDS tile only: ComplexF64 launches, Float64 launches with an odd k0 and
 *                         counted launches (hsk_op_flops_mode) run the balanced order under setting 2.
 *   (hsk_leaf_envelope checks fidx, colptr and rowval against n.) */
int hsk_leaf_envelope(int64_t n, const int64_t* colptr, const int64_t* rowval, const int32_t* fidx, int64_t ni, int64_t nb, int32_t* firstL, int32_t* firstU);
int hsk_branch_envelope(int64_t n, const int64_t* colptr, const int64_t* rowval, const int32_t* fidx, int64_t ni, int64_t nb, int64_t ni1, int64_t nb1,
                        int32_t* firstL, int32_t* firstU);
int hsk_envelope_enable(int on);
int hsk_branch_envelope_enable(int on);
int hsk_env_order_enable(int on);
int hsk_env_tile_order(int tiles_m, int tiles_n, int order, int32_t* tm, int32_t* tn);
int hsk_env_phase_order(int tiles_m, int tiles_n, const int32_t* kr, const int32_t* kc, int shift, int32_t* tm, int32_t* tn, int32_t* pos);
int hsk_env_perm(int is_complex, int ni, int nb, const int32_t* env, int cmat, int bmat, int r0, int r1, int c0, int c1, int k0, int k1, int edge,
                 int slot, uint16_t* out);
int hsk_env_perm_slot_limit(int limit);
int hsk_env_perm_min_tiles(int min_tiles);
long long hsk_env_perm_launches(int reset);
int hsk_op_flops_mode(int on);
int hsk_op_flops(double* out);

/* The plain update C -= A * B of a level through the launch path of a factorization (Sched::gemm -> launch_gemm_op; Float64), for a batch of
 * `count` fronts with M[f] x N[f] results and a common K: the U12 update UR[r0.., :] -= LF[r0.., k0:k1) * UR[k0:k1, :] with k0 = koff,
 * k1 = koff + K, r0 = k1 + roff.  A (M[f] x K), B (K x N[f]) and C (M[f] x N[f], overwritten) are packed column-major, front after front.
 * A launch runs `gemm_op_lds_kernel` (operands loaded straight into LDS) when every front qualifies -- K a multiple of 16, A and B 16-byte
 * aligned: koff / roff = 1 shift B / A by one double -- and `gemm_op_kernel` otherwise; *routed (may be null) receives the number of
 * launches that took the former.  repeat / ms_out as in hsk_gemm_d.
 * A launch with an even koff that does not qualify -- a K tail, roff = 1 -- runs `gemm_op_lds_edge_kernel`, which is counted apart.
 *   hsk_gemm_lds_enable        : 0 sends every launch to the register-staged gemm_op_kernel / gemm_op_env_kernel (default: on unless
 *                                HS_GEMM_LDS=0); returns the previous setting.
 *   hsk_gemm_lds_launches      : launches sent to gemm_op_lds_kernel since the last call with reset != 0.
 *   hsk_gemm_lds_edge_launches : the same for gemm_op_lds_edge_kernel and its enveloped twin gemm_op_env_lds_kernel.
 *   hsk_gemm_reg_launches      : the same for plain Float64 updates that went to gemm_op_kernel / gemm_op_env_kernel (not counted while
 *                                hsk_op_flops_mode is on).
 *   hsk_gemm_lds_route         : the routing rule itself, per front, on the host (no device needed): 0 register-staged (odd k0, or no K at
 *                                all), 1 gemm_op_lds_kernel (K = min(k1, ni) - k0 a multiple of 16, k0 even, A's row offset r0 (+ ni when
 *                                cmat is SB = 2) even), 2 the edge kernel (k0 even, K tail and / or odd row offset).  cmat: 0 LF, 1 UR, 2 SB.
 *                                A launch takes the lowest class one of its fronts needs: 0 before 2 before 1. */
int hsk_gemm_op_d(int64_t count, const int64_t* M, const int64_t* N, int64_t K, int64_t koff, int64_t roff, const double* A, const double* B,
                  double* C, int64_t* routed, int repeat, double* ms_out);
int hsk_gemm_lds_enable(int on);
long long hsk_gemm_lds_launches(int reset);
long long hsk_gemm_lds_edge_launches(int reset);
long long hsk_gemm_reg_launches(int reset);
int hsk_gemm_lds_route(int cmat, int r0, int k0, int k1, int ni);

/* The Schur update SB -= LF[ni.., 0:ni) * UR of a level through the same launch path, for `count` fronts with their own ni[f] and nb[f]
 * (K = ni[f], A's row offset = ni[f]: a batch mixes K tails and odd / even offsets as a real level does).  A (nb x ni), B (ni x nb) and
 * C (nb x nb, overwritten) are packed column-major, front after front; the rest of every front holds a finite non-zero value.  All three
 * null: no host data, timing only.  env != 0: an enveloped launch, every front with the block envelope of the zeros of its A and B.
 * *routed_lds / *routed_edge (may be null): launches that took gemm_op_lds_kernel / the edge kernels.  repeat / ms_out as in hsk_gemm_d. */
int hsk_gemm_schur_d(int64_t count, const int64_t* ni, const int64_t* nb, const double* A, const double* B, double* C, int env,
                     int64_t* routed_lds, int64_t* routed_edge, int repeat, double* ms_out);

/* The 256-row TRSM base case UR[r0 : r0 + wl, c0 : c1) <- inv256L[r0 / 256] * UR (wl = min(256, ni[f] - r0); Float64) of a level through the
 * launch path of a factorization (Sched::trsm_rec), for `count` fronts with their own ni[f] and nb[f]: one launch of `trsm_strip_kernel`
 * (kernels_trsm.hip) while the strip kernel is on, the two half products on the GEMM tile (`trsm_inv_kernel`, enveloped:
 * `trsm_inv_env_kernel`) otherwise -- the stored values have the same bits either way.  X: the whole ni[f] x nb[f] UR of every front,
 * column-major with leading dimension ni[f], front after front, overwritten with what the device holds afterwards; inv: one 256 x 256
 * block per front.  r0 a multiple of 256; a front with ni[f] <= r0 is left untouched.  On the device UR has the leading dimension
 * ni[f] + ldpad and starts `shift` (0 or 1) doubles past a 16-byte boundary.  env != 0: an enveloped launch, every front with the firstU
 * of the leading zeros its columns really have.  *strips (may be null): launches that took the strip kernel.
 *   hsk_trsm_strip_enable   : 0 sends the base case to the two half products again (default: on unless HS_TRSM_STRIP=0); returns the
 *                             previous setting.
 *   hsk_trsm_strip_launches : launches of trsm_strip_kernel since the last call with reset != 0 (each replaces a pair of half products).
 *   hsk_trsm_half_launches  : the same for the Float64 lower half products (GemmOp::ainv 3 and 4, one count per launch). */
int hsk_trsm_inv_d(int64_t count, const int64_t* ni, const int64_t* nb, int64_t r0, int64_t c0, int64_t c1, int64_t ldpad, int64_t shift,
                   const double* inv, double* X, int env, int64_t* strips);
int hsk_trsm_strip_enable(int on);
long long hsk_trsm_strip_launches(int reset);
long long hsk_trsm_half_launches(int reset);

/* The kernels of hs_mod_* (kernels_mod.hip) on host data; every block column-major.
 *   hsk_mod_inner:   T (k x m, ldt) = op(P)^H Y, P n x k, Y n x m; conj != 0: op = conj, i.e. T = P^T Y (ComplexF64; ignored for Float64).
 *                    k in 1..256, m in 1..64.  Row slabs of 2048, partial sums added in slab order (csrc/hs_mod.h states the order).
 *   hsk_mod_apply:   Y (n x m) -= op(Z) T, Z n x k, T k x m; conj != 0: op = conj.
 *   hsk_mod_gather:  T[j, c] = Y[J[j], c], J 0-based.
 *   hsk_mod_cap:     T (k x m, any m >= 1) = op(C)^-1 T by a partial-pivoting LU of C (k x k, not overwritten); op 0: C, 1: C^T, 2: C^H.
 *                    HS_ERR_SINGULAR on an exactly zero pivot, T untouched. */
int hsk_mod_inner_d(int64_t n, int64_t k, int64_t m, const double* P, int64_t ldp, const double* Y, int64_t ldy, int conj, double* T, int64_t ldt);
int hsk_mod_inner_z(int64_t n, int64_t k, int64_t m, const double* P, int64_t ldp, const double* Y, int64_t ldy, int conj, double* T, int64_t ldt);
int hsk_mod_apply_d(int64_t n, int64_t k, int64_t m, double* Y, int64_t ldy, const double* Z, int64_t ldz, const double* T, int64_t ldt, int conj);
int hsk_mod_apply_z(int64_t n, int64_t k, int64_t m, double* Y, int64_t ldy, const double* Z, int64_t ldz, const double* T, int64_t ldt, int conj);
int hsk_mod_gather_d(int64_t n, int64_t k, int64_t m, const double* Y, int64_t ldy, const int64_t* J, double* T, int64_t ldt);
int hsk_mod_gather_z(int64_t n, int64_t k, int64_t m, const double* Y, int64_t ldy, const int64_t* J, double* T, int64_t ldt);
int hsk_mod_cap_d(int64_t k, int64_t m, const double* C, int64_t ldc, int op, double* T, int64_t ldt);
int hsk_mod_cap_z(int64_t k, int64_t m, const double* C, int64_t ldc, int op, double* T, int64_t ldt);

/* The pieces of hs_eigs_* (kernels_eigs.hip, csrc/hs_small_eig.h) on host data; every block column-major.
 *   hsk_eigs_rotate:    Out (n x N, ldo) = V (n x K, ldv) Q (K x N, ldq), K in 1..256, N in 1..K, on v_mfma_f64_16x16x4_f64.  inplace != 0: the
 *                       kernel runs with Out = V on the device (the first N columns of V are overwritten there) and Out receives them.
 *   hsk_eigs_chol_inv:  G (p x p Gram matrix, ldg, p in 1..64) = R^H R: R and Rinv = R^-1 (p x p, ld p, upper), *info = -1, or the first
 *                       column whose pivot is not above (64 eps)^2 times the largest diagonal entry of G (R and Rinv are then undefined).
 *   hsk_small_eig_z:    host only.  H (m x m ComplexF64, ldh, m in 1..256, not overwritten) -> eigenvalues w (m) and unit eigenvectors Y
 *                       (m x m, ldy) with H Y = Y diag(w): Hessenberg reduction, shifted QR, back substitution.  HS_ERR_SINGULAR when the QR
 *                       iteration does not converge. */
int hsk_eigs_rotate_d(int64_t n, int64_t K, int64_t N, const double* V, int64_t ldv, const double* Q, int64_t ldq, int inplace, double* Out, int64_t ldo);
int hsk_eigs_rotate_z(int64_t n, int64_t K, int64_t N, const double* V, int64_t ldv, const double* Q, int64_t ldq, int inplace, double* Out, int64_t ldo);
int hsk_eigs_chol_inv_d(int64_t p, const double* G, int64_t ldg, double* R, double* Rinv, int* info);
int hsk_eigs_chol_inv_z(int64_t p, const double* G, int64_t ldg, double* R, double* Rinv, int* info);
int hsk_small_eig_z(int64_t m, const double* H, int64_t ldh, double* w, double* Y, int64_t ldy);
/* hsk_eigs_coldot: d[c] = Re sum_i conj(X[i, c]) Y[i, c] for the nc columns of two n x nc blocks (launch_eigs_coldot, the x^H op(M) x of
 * hs_eigs_gen_*): row slabs of 2048, a thread adds its rows in order, partials fold by halves, slabs are added in slab order -- the bits of
 * a slab do not depend on the rows behind it.  pair (nc ints, or NULL): 0 a column of its own; +1 / -1 the two columns of a Float64
 * conjugate pair, which share one figure, the sum over both columns. */
int hsk_eigs_coldot_d(int64_t n, int64_t nc, const double* X, int64_t ldx, const double* Y, int64_t ldy, const int* pair, double* d);
int hsk_eigs_coldot_z(int64_t n, int64_t nc, const double* X, int64_t ldx, const double* Y, int64_t ldy, const int* pair, double* d);
/* Host-clock seconds of this thread's last hs_eigs_* call by phase: out4 = {block solves, orthogonalisation, restarts (host eigenproblem
 * and basis rotation), Ritz vectors and residuals}.  The block solve is timed apart only while hsk_eigs_phase_timing is on (it adds one
 * stream synchronisation per block solve and changes no result; returns the previous setting); otherwise its time is counted with the
 * orthogonalisation that follows it. */
int hsk_eigs_phase_timing(int on);
int hsk_eigs_phases(double* out4);
/* Host-clock seconds of the products with op(M) of this thread's last hs_eigs_gen_* call, taken only while hsk_eigs_phase_timing is on (it
 * then puts a stream synchronisation before and behind every product); 0 otherwise.  They are part of the phases above they occur in. */
double hsk_eigs_gen_mprod_seconds(void);

/* hsk_ulv_det: the per-node reduction of hs_hss_logabsdet (ulv_det_kernel, one wave per node) on host data.  nnodes packed LUs, node k
 * ni[k] x ni[k] with leading dimension ld[k] >= max(ni[k], 1), one after the other in LU; their row permutations one after the other in
 * rperm (0-based; ni[k] = 0: an empty node).  out2[2k] = sum log|u_ii|, out2[2k+1] = sum arg(u_ii) (ComplexF64; 0 for Float64),
 * flags3[3k..] = {negative diagonal entries (Float64), parity of rperm, an exactly zero pivot}; res3 = {log|det|, sign_re, sign_im} of
 * the product over all nodes, folded in node order as hs_hss_logabsdet folds it. */
int hsk_ulv_det_d(int64_t nnodes, const int64_t* ni, const int64_t* ld, const double* LU, const int32_t* rperm, double* out2, int32_t* flags3, double* res3);
int hsk_ulv_det_z(int64_t nnodes, const int64_t* ni, const int64_t* ld, const double* LU, const int32_t* rperm, double* out2, int32_t* flags3, double* res3);

/* Microseconds per ROUND TRIP (two exchanges) between workgroup 0 and workgroup `peer` of one launch through agent-scope atomic stores and polled
 * loads -- the exchange primitive of the dataflow sweeps of ldiv! (kernels_solve_wide.hip).  peer = 1: another XCD, peer = 8: the same XCD. */
double hsk_flow_pingpong_us(int peer, int iters);
/* Measured TFLOP/s of back-to-back v_mfma_f64_16x16x4_f64 on every CU (roofline denominator). */
double hsk_mfma_f64_peak(int waves_per_simd, int iters);
/* The same issue loop on random operands that change while it runs: the rate at the clock the chip holds under such data (DVFS). */
double hsk_mfma_f64_peak_random(int waves_per_simd, int iters);

#ifdef __cplusplus
}
#endif
#endif
