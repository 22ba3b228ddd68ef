/*
 * hs_solver.h -- C ABI of the MI355X-native nested-dissection elimination.
 *
 * Drop-in boundary for ONE hot path of bonevbs/HierarchicalSolvers.jl:
 *
 *   factor(A::SparseMatrixCSC{T}, nd, nd_loc, opts; kw...) -> FactorNode{T}
 *                                      (reference src/factorization.jl:5-11)
 *   ldiv!(C, F, B), ldiv!(F, B)        (reference src/factornode.jl:62-74)
 *   ldiv!(C, transpose(F), B), ldiv!(C, adjoint(F), B)   (hs_ldiv_t_*, hs_ldiv_dev_t_*)
 *   gmres(transpose(A), b; Pr=transpose(F)), gmres(A', b; Pr=F')   (hs_gmres_t_*, hs_gmres_block_t_*)
 *   opnorm(A, p), opnormestinv(A), cond(A, p), refined solves (xGERFS)   (hs_opnorm, hs_normestinv, hs_condest, hs_ldiv_refine_*, hs_ldiv_refine_block_*)
 *   logabsdet(F), logdet(F), det(F), selected inverse (diag(A^-1), A^-1 on A's pattern)   (hs_logabsdet, hs_selinv)
 *   maxrank(F)                         (reference src/factornode.jl:49-57)
 *
 * The reference has no FFI of its own (it is pure Julia); these entry points
 * are what a Julia `ccall` shim for that path binds (INTEGRATION.md shows the
 * shim).  Plain pointers and sizes only; all index arrays are 1-based int64
 * exactly as the Julia host holds them (SparseMatrixCSC.colptr/rowval, the
 * index vectors of the NestedDissection trees), converted inside the library.
 *
 * Threading: a call blocks the calling thread.  One handle must not be used
 * from two threads at once; distinct handles may.  hs_free is idempotent per
 * handle pointer value being NULL-safe and may be called from any thread
 * (Julia finalizer).  Errors: every int-returning function returns HS_OK (0)
 * or a negative hs_status; hs_last_error() returns the thread-local message.
 */
#ifndef HS_SOLVER_H
#define HS_SOLVER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum hs_status {
  HS_OK = 0,
  HS_ERR_ARGUMENT = -1,  /* Julia ArgumentError   (HierarchicalSolvers.jl:74-78, nesteddissection.jl:111) */
  HS_ERR_DIMENSION = -2, /* Julia DimensionMismatch (blockmatrix.jl:13-16,116-117; nesteddissection.jl:107) */
  HS_ERR_TREE = -3,      /* ErrorException "Expected nested dissection to be a binary tree..." (factorization.jl:25) */
  HS_ERR_SINGULAR = -4,  /* LinearAlgebra.SingularException raised by `\` in the reference; info = node id */
  HS_ERR_HSS_LEAF = -5,  /* error("One of the Schur complements turned into a leaf. Aborting.") (factorization.jl:164) */
  HS_ERR_DEVICE = -6,    /* HIP runtime failure / no gfx950 device: the library never falls back to the CPU */
  HS_ERR_NOMEM = -7,     /* device or host allocation failed */
  HS_ERR_UNSUPPORTED = -8
} hs_status;

/* POD mirror of `mutable struct SolverOptions` (HierarchicalSolvers.jl:30-40), same order,
 * followed by extension fields (zero = default). */
typedef struct hs_options {
  int64_t swlevel;  /* compress the top `swlevel` levels; <0 counts from the leaves (factorization.jl:8) */
  int64_t swsize;   /* minimum |bnd| for compression */
  double atol;
  double rtol;
  double c_tol;     /* validated, never consumed by the reference (factorization.jl:97-100) */
  int64_t leafsize; /* HSS leaf size */
  int64_t kest;     /* rank estimate for randomized compression; <0 => ceil(rank(L)/2) (factorization.jl:102-104) */
  int64_t stepsize; /* validated, never consumed by the reference */
  uint8_t verbose;
  /* ---- extensions ---- */
  uint8_t keep_schur; /* debug: retain every node's Schur complement S for hs_node_export */
  uint8_t profile;    /* time every kernel launch with HIP events (fills hs_stats.t_gemm etc.; adds launch gaps) */
  uint8_t split;      /* slice width, in units of 256 columns, in which the interior block of a compressed front (level <=
                         swlevel, ni >= 2 slices) is eliminated: the role of the 2x2 BlockFactorization of D (blockmatrix.jl:106-130);
                         0 = off; single-rank factorizations only */
  uint8_t hss_d;      /* > 0: a front at a level <= swlevel whose interior block has at least hss_d*1024 DOFs keeps D = Aii as an HSS
                         matrix (include/hs_hss.h) instead of a dense LU -- the role of `D::BlockFactorization` over HssMatrix blocks
                         (blockmatrix.jl:121-130, factorization.jl:86-96); the root included, which in the reference receives its
                         children's HSS blocks although it is never flagged (factorization.jl:15,67,126).  Single rank only.  With such fronts
                         hs_ldiv_dev_* and hs_solve_*_levels return only after the HSS solves on the given stream have completed
                         (the HSS module recycles its workspaces per call). */
  uint8_t hss_dexp;   /* tolerance of that HSS form: atol, rtol * 10^-e with e = 2 for hss_dexp = 0 (default) and e = hss_dexp - 1
                         otherwise (1: the tolerance of the fronts, as the reference does).  D^-1 inherits cond(D) * tol, the low-rank
                         couplings only tol: measured on Poisson 128^3 the same tolerance for both leaves GMRES unconverged */
  uint8_t mf;         /* 1 or 2: the compressed branch with the reference's data flow (src/factorization.jl:78-112,126-140): the Schur complement of a
                         flagged front leaves as an HSS matrix compressed from the operator Abb - Abi*R (never formed where the children are HSS),
                         a parent with two such children is assembled matrix-free from their generators and the sparse couplings of A: Aib, Abi
                         and Abb are never dense, L / R come from the children's generators (hs_mffront.h).
                         3: D = Aii of such a parent is the reference's `blockfactor` over HSS blocks (src/blockmatrix.jl:121-130): A11 is the left
                            child's own HSS block, A12 / A21 the sparse couplings, S22 = A22 - A21*A11^-1*A12 recompressed from its operator
                            (hss_dexp sets its tolerance); `ldiv!` runs `blockldiv!` (two HSS solves).
                         2: D is ONE HSS matrix over a bisection order of the interior, compressed from the operator [A11 A12; A21 A22].
                         1: D is expanded from the generators and eliminated densely by the front kernels (ni x ni, the one dense block of the
                            front), except on the fronts hss_d selects: the dense LU of a 32,768 block takes 0.5 s, its HSS compression +
                            elimination at 1e-4 1.8 s.
                         With nranks > 1 (dist_top = 0) the joins ship the children's HSS matrices packed into one buffer (hs_exchange_kind,
                         hs_schur_pack / hs_schur_unpack); refused together with dist_top or split.  hs_maxrank includes hssrank(S). */
  uint8_t dist_top;   /* multi-rank factorizations (nranks > 1): 1 = every front ABOVE the rank cut is eliminated by all ranks of its group instead of
                         the group's first rank (the reference factors the two subtrees of a node one after the other although they are independent,
                         src/factorization.jl:20-21; above the cut the independent units are the block columns of one front): block columns of
                         HS_DIST_NB (512) interior DOFs dealt over the group in runs of HS_DIST_PERIOD (2), each factored by its owner and fanned out to the group,
                         every rank updating its own block columns and its slice of the boundary columns; the group ends holding the complete
                         factors and Schur complement, sibling groups swap Schur complements pairwise at the join.  Needs a communicator
                         (hs_set_comm).  Fronts above the cut are eliminated exactly in this mode (no compression there). */
  int64_t seed;       /* RNG seed of the randomized compression (reference: Random.seed!(123), test/rungmres.jl:7) */
  uint8_t symmetric;  /* 1: the caller states A == transpose(A), entry for entry and bit for bit: real symmetric and COMPLEX SYMMETRIC matrices
                         (plain transpose).  Hermitian matrices are not served by this option (A != transpose(A) unless real).  The fronts a level
                         eliminates densely then update only the lower triangle of their trailing blocks and of the Schur complement, in column
                         strips (multiples of 256 wide), and rebuild the upper blocks by transposition: same pivots, the same P, L, U, Lbi, Uib, S up
                         to rounding, in the same layout -- every solve-phase entry point works on such a handle unchanged.  Compressed, HSS and
                         matrix-free fronts, dense fronts fed by compressed children, tournament-pivoted and redone levels keep the general
                         path (hs_sym_info reports the counts).  hs_numeric_begin checks the claim on the device and returns HS_ERR_ARGUMENT
                         naming the first offending (row, column) before any front is touched; with nranks > 1 hs_analyze / hs_plan return
                         HS_ERR_UNSUPPORTED.  Appended after `seed`: the offsets of the older fields do not move.  Default 0. */
  uint8_t equilibrate; /* 1: hs_numeric_begin scales the rows and columns of A by powers of two before any front is assembled: integer exponents
                         er, ec (hs_equil_scales) with A_s = 2^er A 2^ec, found on the device by Ruiz sweeps in the infinity norm (|a| = fabs,
                         |re| + |im| for complex; per sweep every exponent moves by -floor((floor(log2 max) + 1) / 2) of its row / column maximum,
                         rows and columns together; the first sweep that moves nothing ends them, 16 at most; at a fixed point every maximum
                         lies in [0.5, 2) -- except one that is not finite: a magnitude that overflows, which takes an entry near the
                         largest Float64 (|re| + |im| of a complex entry can reach it unscaled), or an infinite entry, moves nothing: its row and
                         column keep the exponents they have and may end outside that range; a NaN entry enters no maximum).  Scaling by 2^e is exact, so the handle is a plain handle of A_s between two exact scalings: the
                         fronts, the pivoting decisions and the compression tolerances atol / rtol act on A_s, and hs_ldiv_*, hs_ldiv_t_*,
                         hs_ldiv_block_*, hs_ldiv_block_t_*, hs_ldiv_ulv_* (and every driver built on them) return
                         2^ec (F_s^-1 (2^er B)) for trans = 0 and 2^er (F_s^-T (2^ec B)) for trans = 1, 2 -- bit for bit what a handle of the
                         prescaled matrix returns for the prescaled block.  hs_logabsdet subtracts ln 2 (sum er + sum ec).  The handle's own A
                         (residuals, hs_opnorm, GMRES, sensitivities) stays the caller's unscaled matrix.  Entry points that read the stored
                         factors directly (hs_mul_*, hs_factor_error_*, hs_selinv, hs_selinv_lr, hs_f32_create, hs_interface_*,
                         hs_ldiv_sparse_* and the calls that solve on its pruned paths -- sparse blocks of hs_sens_* / hs_tangent_* / hs_gn_*,
                         hs_gn_hessvec_* / hs_gn_diag_* with itmax = 0, hs_mod_create_sparse_* --, hs_solve_fwd_levels / hs_solve_bwd_levels)
                         return HS_ERR_UNSUPPORTED on such a handle;
                         hs_node_export returns blocks of A_s.  A non-zero entry whose scaled value would be subnormal or infinite makes
                         hs_numeric_begin return HS_ERR_UNSUPPORTED naming it; with nranks > 1 hs_analyze / hs_plan return HS_ERR_UNSUPPORTED.
                         With symmetric, the claim is checked on the caller's values; er == ec then, so A_s is symmetric bit for bit.
                         Every hs_numeric_begin finds the exponents anew.  Appended after `symmetric`.  Default 0: nothing is launched or allocated. */
} hs_options;

/* Defaults of the reference's kw-constructor (HierarchicalSolvers.jl:43-54): 5,1,1e-6,1e-6,0.5,32,-1,10,false */
void hs_options_default(hs_options* opts);

/* Flat post-ordered form of the two trees `symfact!` returns (nesteddissection.jl:29-69).
 * Node ids are 0-based post-order positions (children before parents, root = nnodes-1), -1 = no child.
 * *_idx hold 1-based values as Julia holds them; *_ptr are 0-based offsets, length nnodes+1.
 *   int_idx  : nd.int      (global DOF ids eliminated at the node)
 *   bnd_idx  : nd.bnd      (global DOF ids of the node's boundary)
 *   iloc_idx : nd_loc.int  (positions in the node's OWN bnd that land in the parent's int)
 *   bloc_idx : nd_loc.bnd  (positions in the node's OWN bnd that land in the parent's bnd)
 */
typedef struct hs_tree {
  int64_t nnodes;
  const int64_t* left;
  const int64_t* right;
  const int64_t* int_ptr;
  const int64_t* int_idx;
  const int64_t* bnd_ptr;
  const int64_t* bnd_idx;
  const int64_t* iloc_ptr;
  const int64_t* iloc_idx;
  const int64_t* bloc_ptr;
  const int64_t* bloc_idx;
} hs_tree;

typedef struct hs_handle hs_handle; /* opaque: owns every device allocation of one factorization */

/* factor(A, nd, nd_loc, opts) for T = Float64 / ComplexF64 (factorization.jl:5).
 * A is n x n CSC with 1-based colptr[n+1], rowval[nnz]; nzval_z is interleaved (re,im) = Julia ComplexF64.
 * Inputs are borrowed for the duration of the call.  On success *out owns the device-resident factors. */
int hs_factor_d(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                const hs_tree* tree, const hs_options* opts, hs_handle** out);
int hs_factor_z(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval_z,
                const hs_tree* tree, const hs_options* opts, hs_handle** out);

/* ldiv!(C, F, B): C = F^{-1} B for n x nrhs column-major host arrays (factornode.jl:62-74).
 * C may alias B (true in-place semantics; the reference's 2-arg form allocates). */
int hs_ldiv_d(hs_handle* F, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_ldiv_z(hs_handle* F, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);

/* Same with DEVICE pointers on HIP stream `stream` (hipStream_t, NULL = default), asynchronous:
 * for an on-device Krylov caller (gmres(...; Pr=F), test/rungmres.jl:47-48). */
int hs_ldiv_dev_d(hs_handle* F, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
int hs_ldiv_dev_z(hs_handle* F, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);

/* ldiv!(C, transpose(F), B) (trans = 1) and ldiv!(C, adjoint(F), B) (trans = 2; = 1 for Float64); trans = 0: hs_ldiv_*.
 * Same factors, no refactorization; single-rank factorizations whose fronts all keep a dense LU of D (else HS_ERR_UNSUPPORTED).
 * Limits, refused with HS_ERR_UNSUPPORTED before any device work: fronts that keep D as an HSS matrix (hs_options.hss_d, mf = 2, 3:
 * no transposed ULV solve) and factorizations over more than one rank (whatever dist_top is).  Other trans: HS_ERR_ARGUMENT.
 * The _dev_ forms take device pointers on `stream` like hs_ldiv_dev_*; C may alias B in both.  The host forms set stats.t_solve. */
int hs_ldiv_t_d(hs_handle* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_ldiv_t_z(hs_handle* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_ldiv_dev_t_d(hs_handle* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
int hs_ldiv_dev_t_z(hs_handle* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);

/* ldiv!(C, F, B) for an n x nrhs block, the factors read once per chunk of columns (hs_solve_multi.hip). Same arguments as hs_ldiv_t_*;
 * trans must be 0. C may alias B.  The block travels through the elimination tree in chunks of HS_LDIV_BLOCK_COLS columns (16 / 32 / 48 / 64,
 * default 32; read once per process); every step is a tall-skinny product on the FP64 matrix pipe.  No atomics and a fixed summation order:
 * two calls return the same bits, and a column of C does not depend on the values, the number or the position of the other columns.
 * The results agree with hs_ldiv_* to rounding, not bit for bit.  Served: what hs_ldiv_t_* serves (single-rank handles whose fronts all
 * keep a dense LU of D, low-rank L / R included).  Refused with HS_ERR_UNSUPPORTED before any device work and before C is written: fronts
 * that keep D as an HSS matrix (hs_options.hss_d, mf = 2, 3), more than one rank, trans = 1, 2 (served by hs_ldiv_block_t_*; other trans:
 * HS_ERR_ARGUMENT).  nrhs = 0
 * touches nothing.  The host forms move the whole block once and set stats.t_solve; the _dev_ forms are asynchronous on `stream`.  The work
 * blocks ((sum of ni + the largest level's sum of ni and of nb) x chunk columns) are taken on first use, kept in the handle and freed by hs_free; the
 * workspaces of hs_ldiv_* / hs_ldiv_t_* are not touched, so the calls may alternate freely. */
int hs_ldiv_block_d(hs_handle* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_ldiv_block_z(hs_handle* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_ldiv_block_dev_d(hs_handle* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
int hs_ldiv_block_dev_z(hs_handle* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
/* ldiv!(C, transpose(F), B) (trans = 1) and ldiv!(C, adjoint(F), B) (trans = 2; = 1 for Float64) for an n x nrhs block, the factors read
 * once per chunk of columns: hs_ldiv_block_* for op(F).  trans = 0 goes through hs_ldiv_block_* and returns its bits.  Everything else as
 * there: C may alias B, nrhs = 0 touches nothing, chunks of HS_LDIV_BLOCK_COLS columns, the same work blocks (the workspace does not grow),
 * the same determinism (no atomics, one summation order, a column independent of its neighbours and of its position), the same handles
 * served and the same ones refused with HS_ERR_UNSUPPORTED before any device work and before C is written (HSS interior blocks, more than
 * one rank); trans outside 0..2, null blocks, a mismatched element type: HS_ERR_ARGUMENT; bad sizes: HS_ERR_DIMENSION.  The stored blocks
 * serve both directions (the 256 x 256 inverse diagonal blocks are applied transposed): no factor memory is added.  The results agree
 * with hs_ldiv_t_* to rounding, not bit for bit.  The host forms move the whole block once and set stats.t_solve; the _dev_ forms are
 * asynchronous on `stream`. */
int hs_ldiv_block_t_d(hs_handle* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_ldiv_block_t_z(hs_handle* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_ldiv_block_dev_t_d(hs_handle* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
int hs_ldiv_block_dev_t_z(hs_handle* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
/* C = op(F)^-1 B for an n x nrhs block (trans = 0: F, 1: transpose(F), 2: adjoint(F)) on ANY complete single-rank handle, the ones whose fronts
 * keep their interior block D as an HSS matrix included (hs_options.hss_d, mf = 2, 3): what hs_ldiv_block_* / hs_ldiv_block_t_* refuse.  Such a
 * front is served per chunk of HS_LDIV_BLOCK_COLS columns on the caller's block, between the grouped launches of its level's other fronts.
 * With t = B[int], Abi ~ C_L Z_L, Aib ~ C_R Z_R, W = D^-1 C_R:
 *   trans = 0:     forward  t = D^-1 t, B[bnd] -= C_L (Z_L t);                backward  B[int] = t - W (Z_R B[bnd])
 *   trans = 1, 2:  forward  B[bnd] -= op(Z_R)^T (op(W)^T t) (no solve with D); backward  B[int] = op(D)^-T (t - op(Z_L)^T (op(C_L)^T B[bnd]))
 * op(D)^-T is one transposed ULV solve from the stored factors (hs_hss_ldiv_t, include/hs_hss.h; the 2 x 2 block form of mf = 3: two, around
 * its stored couplings).  No factor memory is added; the scratch of a call (the largest such front x one chunk) comes from the library's
 * scratch cache and goes back to it.  A handle WITHOUT such fronts goes through hs_ldiv_block_t_* and returns its bits.  Two calls return equal
 * bits.  Refused before any device work and with C untouched: more than one rank (HS_ERR_UNSUPPORTED), trans outside 0..2, null blocks, a
 * mismatched element type (HS_ERR_ARGUMENT), bad sizes (HS_ERR_DIMENSION), a low-rank transform that does not keep its dense C
 * (HS_ERR_UNSUPPORTED).  C may alias B.  Both forms return when the result is complete (the ULV solves of the fronts synchronise `stream`). */
int hs_ldiv_ulv_d(hs_handle* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_ldiv_ulv_z(hs_handle* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_ldiv_ulv_dev_d(hs_handle* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
int hs_ldiv_ulv_dev_z(hs_handle* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
/* Per-handle switch: who applies op(F)^-1 inside the lockstep drivers and hs_logabsdet on a handle whose fronts keep their interior block D
 * as an HSS matrix (hs_options.hss_d, mf = 2, 3).
 *   mode = 0 (default): today's routing and today's refusals, bit for bit.
 *   mode = 1: on such a handle hs_gmres_*, hs_gmres_t_*, hs_gmres_block_*, hs_gmres_block_t_*, hs_ldiv_refine_* (any trans, ferr),
 *             hs_ldiv_refine_block_*, hs_normestinv, hs_condest and hs_sens_* / hs_misfit_* (dense B and W; sparse ones stay refused)
 *             apply op(F)^-1 through hs_ldiv_ulv_dev_*, and what that entry point refuses is refused with its words; hs_logabsdet adds
 *             det D of every such front from its ULV factors (hs_hss_logabsdet).  A handle WITHOUT such fronts keeps its routing and
 *             returns the bits of mode 0.  Everything else keeps its refusals in either mode (hs_ldiv_block_*, hs_ldiv_t_*, hs_ldiv_sparse_*,
 *             hs_selinv*, hs_tangent_*, hs_gn_*, hs_mod_*, hs_eigs_*, hs_f32_*, hs_mul_*, hs_interface_*).
 *   mode = -1: query only.
 * Returns the previous mode (0 or 1), or HS_ERR_ARGUMENT (negative) for a null handle or another mode.  The mode is host state of the
 * handle: a plan-only handle (hs_plan) and a handle over several ranks accept the call (the drivers' own refusals then speak), and it
 * survives hs_numeric_begin and every refactorization.  Do not change it while another thread is inside a call on the same handle. */
int hs_ulv_mode(hs_handle* F, int mode);
/* last block solve of the handle, whichever direction it had (waits for it): out6 = {seconds on the device, factor bytes read by the model (column chunks x sum over
 * fronts of (ni^2 + 2 ni nb) sizeof(T), the factor term of hs_stats.bytes_solve), flops executed on the matrix pipe (padding included),
 * useful flops, column chunks, workspace bytes} */
int hs_ldiv_block_info(const hs_handle* F, double* out6);

/* ---- the stored factorization as an operator (hs_mul.hip; the schedule: hs_solve_multi.hip) ------------------------------------------
 * C = op(F) B for an n x nrhs block (trans = 0: F, 1: transpose(F), 2: adjoint(F)), where F = P' L U front by front is what the handle
 * stores -- A itself for an exact factorization, the compressed approximation otherwise: lmul!-style, the counterpart of
 * hs_ldiv_block_t_* with the same arguments, status codes and chunks of HS_LDIV_BLOCK_COLS columns, on the same work blocks (no workspace
 * and no factor memory is added).  Two passes over the tree per chunk and no triangular solve: every front forms Y = triu(U11) B[int] +
 * Uib B[bnd] on its own, then, root first, C[int[rperm]] = unit-tril(L11) Y and C[bnd] += Lbi Y (low-rank Gauss transforms through their
 * factors; trans = 1, 2: the transposed / conjugated products with L and U changing places).  The triangles are read in place, each
 * workgroup only the 16-column chunks that meet its rows.  No atomics and one summation order: two calls return the same bits and a column
 * of C depends neither on the other columns nor on its position.  C may alias B; nrhs = 0 touches nothing; the _dev_ forms are
 * asynchronous on `stream`.  Refused before any device work with C untouched, under the name hs_mul_* / hs_mul_dev_*, what
 * hs_ldiv_block_t_* refuses and in its order: a null handle, trans outside 0..2, a plan-only or unfinished handle, a mismatched element
 * type (HS_ERR_ARGUMENT), bad sizes (HS_ERR_DIMENSION), more than one rank, fronts that keep D as an HSS matrix (HS_ERR_UNSUPPORTED). */
int hs_mul_d(hs_handle* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_mul_z(hs_handle* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_mul_dev_d(hs_handle* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
int hs_mul_dev_z(hs_handle* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
/* last product of the handle (waits for it): out6 as hs_ldiv_block_info's.  A product never shows as the handle's last block solve. */
int hs_mul_info(const hs_handle* F, double* out6);
/* How far the stored factorization is from A, a property of the handle alone: R = op(A) W - op(F) W on the device for k probe columns W
 * (the handle's own A, one product with the factors, the ordered column sums of squares) and
 *   out4 = {||R||_F / ||op(A) W||_F, ||R||_F, ||op(A) W||_F, seconds on the device}.
 * Omega (n x k, ld ldo; where = 0: host, 1: device pointer) gives the probes; Omega == NULL: column j is the +-1 column
 * pm1(col_key(seed, j, 0), i) of the library's estimators -- no generator state, two calls return the same bits.  With +-1 probes
 * ||R||_F^2 / k is the Hutchinson estimate of ||op(A) - op(F)||_F^2.  Refused like hs_mul_*, under the name hs_factor_error_*; k < 1, a
 * null out4, another `where`: HS_ERR_ARGUMENT. */
int hs_factor_error_d(hs_handle* F, int trans, const double* Omega, int64_t ldo, int64_t k, int64_t seed, int where, double* out4);
int hs_factor_error_z(hs_handle* F, int trans, const double* Omega, int64_t ldo, int64_t k, int64_t seed, int where, double* out4);

/* ---- sparse right-hand sides, selected rows of the solution (hs_solve_sparse.hip) ---------------------------------------------------
 * X[r, j] = (op(F)^-1 B)[rows[r], j] for a sparse B and a list of wanted rows.  B is n x nrhs in CSC form, 1-based like A, rows strictly
 * increasing within a column (stored zeros count as entries); rows: 1-based, any order, repeats allowed; rows == NULL: all n rows (nrows is
 * ignored, X is n x nrhs).  X is column-major with leading dimension ldx.  trans = 0 / 1 / 2: F, transpose(F), adjoint(F) -- trans acts
 * on F, never on B.
 * The columns travel through the tree in chunks of HS_LDIV_BLOCK_COLS like hs_ldiv_block_t_*, but a chunk's forward sweep visits only the
 * fronts that own a stored row of its columns and their ancestors, and its backward sweep only the fronts that own a wanted row and their
 * ancestors (closed on the handle's internal front graph: slices of hs_options.split, the pseudo-root).  Columns are processed in a stable
 * sort by the node id of the front that owns their first stored row, empty columns last; results return to the caller's positions.  The
 * per-front arithmetic is that of the block solve and what is skipped is exactly zero there: X equals the wanted rows of hs_ldiv_block_t_*
 * on the expanded block bit for bit, with its determinism.  A chunk of empty columns launches nothing and returns zeros.
 * The host forms move nnz values up and nrows x nrhs values down; the _dev_ forms take bnzval and X on the device and the index arrays on
 * the host (the closure is host work), run on `stream` and return when X is complete.
 * Refused before any device work, X untouched: what hs_ldiv_block_t_* refuses (HSS interior blocks, more than one rank) with
 * HS_ERR_UNSUPPORTED; a null handle, trans outside 0..2, a plan-only or unfactored handle, a mismatched element type, null pointers with
 * nonzero sizes, bcolptr not 1-based or decreasing, rows of a column of B not strictly increasing: HS_ERR_ARGUMENT; n != size(F), a row
 * index outside 1..n, ldx too small, negative sizes: HS_ERR_DIMENSION.  nrhs == 0, or nrows == 0 with rows != NULL: HS_OK, nothing written. */
int hs_ldiv_sparse_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const int64_t* bcolptr, const int64_t* browval, const double* bnzval,
                     const int64_t* rows, int64_t nrows, double* X, int64_t ldx);
int hs_ldiv_sparse_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const int64_t* bcolptr, const int64_t* browval, const double* bnzval,
                     const int64_t* rows, int64_t nrows, double* X, int64_t ldx); /* bnzval, X: interleaved (re, im) */
int hs_ldiv_sparse_dev_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const int64_t* bcolptr, const int64_t* browval, const double* d_bnzval,
                         const int64_t* rows, int64_t nrows, double* dX, int64_t ldx, void* stream);
int hs_ldiv_sparse_dev_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const int64_t* bcolptr, const int64_t* browval, const double* d_bnzval,
                         const int64_t* rows, int64_t nrows, double* dX, int64_t ldx, void* stream);
/* what such a call would visit; host only, also on an hs_plan handle.  order[nrhs]: the processing order (0-based column ids); *nchunks;
 * active[chunk * nnodes + node]: bit 0 = the forward sweep of the chunk visits the node, bit 1 = the backward sweep does, node ids as in
 * hs_node_info (the user's tree; a split front is visited when any of its slices is).  Any of the three may be NULL (ask for *nchunks first
 * to size active).  Refusals as above. */
int hs_ldiv_sparse_plan(const hs_handle* F, int trans, int64_t n, int64_t nrhs, const int64_t* bcolptr, const int64_t* browval,
                        const int64_t* rows, int64_t nrows, int64_t* order, int64_t* nchunks, uint8_t* active);
/* the last hs_ldiv_sparse_* call of the handle: out8 = {seconds on the device, factor bytes read by the model (sizeof(T) x sum over chunks of
 * the sum of ni^2 / 2 + ni nb over the forward-visited fronts plus the same over the backward-visited ones; with every front visited this is
 * hs_ldiv_block_info's figure), front visits forward, front visits backward, fronts x chunks (what a dense block solve visits per sweep),
 * chunks, values moved between host and device (nnz + nrows x nrhs; 0 for the _dev_ forms), workspace bytes}.  The call runs through the
 * block-solve driver, so hs_ldiv_block_info then reports that driver's figures of it. */
int hs_ldiv_sparse_info(const hs_handle* F, double* out8);

/* ---- adjoint-state sensitivities on A's pattern for a block of sources (hs_sens.hip) ---------------------------------------------------
 * op(A) = A, transpose(A), adjoint(A) for trans = 0 / 1 / 2; X = op(A)^-1 B with B n x nrhs; W (n x nrhs) is the cotangent of a real
 * objective, dJ = Re<W, dX> = Re sum conj(W) .* dX.  With Lam = op(A)^-H W the sensitivity on the pattern of A is, for every stored (i, j):
 *   trans 0:  Lam = adjoint(F) \ W       (Float64: transpose(F) \ W)   G_ij = -sum_c Lam_ic conj(X_jc)
 *   trans 1:  Lam = conj(F \ conj(W))    (Float64: F \ W)              G_ij = -sum_c Lam_jc conj(X_ic)
 *   trans 2:  Lam = F \ W                                              G_ij = -sum_c conj(Lam_jc) X_ic
 * so that for any E on the pattern of A:  d/ds Re<W, op(A + sE)^-1 B> at s = 0  =  Re sum_p E_p conj(G_p).  Float64: no conj, G real.
 * hs_misfit_* is the common objective: distinct receiver rows `rows` (1-based, any order), data D (nrows x nrhs, ldd); R = X[rows, :] - D,
 * J[c] = 0.5 ||R[:, c]||^2, W = R scattered to the rows `rows`; R (may be NULL) is returned in the order of `rows`.
 * A block (hs_block_arg) is dense (column-major, ld >= n) or, with dense == NULL, CSC with the rules of hs_ldiv_sparse_* (1-based, rows
 * strictly increasing within a column).  pattern 0: G has nnz(A) values in the order of the nzval given to the factorization; 1: G has n
 * values, G[j] for the stored (j, j) and 0 where A stores no diagonal entry.  X, Lam (may be NULL): the blocks, n x nrhs.
 * The columns are processed in groups of Gc, a multiple of HS_LDIV_BLOCK_COLS: the widest group whose X and Lam blocks plus staging take at
 * most half of the free device memory (HS_ERR_NOMEM when not even one chunk fits; HS_SENS_GROUP in the environment overrides Gc, read per
 * call).  Per group: the forward solve (dense B: hs_ldiv_block_dev_t_*; sparse B: hs_ldiv_sparse_dev_* with all rows, i.e. the pruned forward
 * sweep; itmax > 0: hs_ldiv_refine_block_dev_* without ferr, a sparse block expanded on the device first -- for compressed handles), W of the
 * misfit form built on the device (sparse by construction: the pruned path when itmax = 0), the adjoint solve by the same choice of paths,
 * and one reduction kernel that continues the sum of every stored entry.  X and Lam never leave the device unless asked for.  For
 * ComplexF64 with trans = 1 the conjugation of W is folded into its copy and the one of the solution into the kernel.
 * Determinism: X and Lam carry the bits of the entry points named above (X = hs_ldiv_block_t_*(op(F), B) for itmax = 0, dense or sparse);
 * the sum of an entry is one chain over the columns in order, every step the same unfused products and sums, no atomics: two calls return
 * the same bits, G does not depend on Gc, a sparse block gives the bits of its dense expansion, and pattern 1 returns the diagonal entries
 * of pattern 0 bit for bit.  G is zero-filled first: nrhs = 0 returns G = 0 and HS_OK.
 * Refused before any device work, every output untouched: what hs_ldiv_block_t_* refuses (HSS interior blocks, more than one rank), by its
 * own check: HS_ERR_UNSUPPORTED; a null, plan-only or unfactored handle, a mismatched element type, trans outside 0..2, pattern outside 0..1,
 * itmax < 0, null pointers with nonzero sizes, a CSC block hs_ldiv_sparse_* would refuse, repeated rows in the misfit form: HS_ERR_ARGUMENT;
 * n != size(F), negative sizes, row indices outside 1..n, leading dimensions too small: HS_ERR_DIMENSION.
 * The host forms move the blocks (or their stored values) up and G, J, R and the requested blocks down; in the _dev_ forms the values and
 * the outputs are on the device, the index arrays (colptr, rowval, rows) on the host, and the call returns when the outputs are complete. */
typedef struct {            /* an n x nrhs block, dense or CSC */
  const double* dense; int64_t ld;                                     /* dense != NULL: column-major */
  const int64_t* colptr; const int64_t* rowval; const double* nzval;   /* else CSC, 1-based, as hs_ldiv_sparse_* */
} hs_block_arg;
int hs_sens_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const hs_block_arg* W, int64_t itmax, int pattern, double* G, double* X, int64_t ldx,
              double* Lam, int64_t ldl);
int hs_sens_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const hs_block_arg* W, int64_t itmax, int pattern, double* G, double* X, int64_t ldx,
              double* Lam, int64_t ldl); /* interleaved (re, im) */
int hs_sens_dev_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const hs_block_arg* W, int64_t itmax, int pattern, double* dG, double* dX,
                  int64_t ldx, double* dLam, int64_t ldl, void* stream);
int hs_sens_dev_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const hs_block_arg* W, int64_t itmax, int pattern, double* dG, double* dX,
                  int64_t ldx, double* dLam, int64_t ldl, void* stream);
int hs_misfit_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const int64_t* rows, int64_t nrows, const double* D, int64_t ldd, int64_t itmax,
                int pattern, double* J, double* R, int64_t ldr, double* G);
int hs_misfit_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const int64_t* rows, int64_t nrows, const double* D, int64_t ldd, int64_t itmax,
                int pattern, double* J, double* R, int64_t ldr, double* G);
int hs_misfit_dev_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const int64_t* rows, int64_t nrows, const double* dD, int64_t ldd,
                    int64_t itmax, int pattern, double* dJ, double* dR, int64_t ldr, double* dG, void* stream);
int hs_misfit_dev_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const int64_t* rows, int64_t nrows, const double* dD, int64_t ldd,
                    int64_t itmax, int pattern, double* dJ, double* dR, int64_t ldr, double* dG, void* stream);
/* the last hs_sens_* / hs_misfit_* call of the handle: out8 = {seconds on the device in total, of the forward solves, of the adjoint solves,
 * of the reduction (staging, the misfit kernel and the copies of requested blocks included), column groups, stored entries x columns
 * reduced, values moved between host and device (0 for the _dev_ forms), workspace bytes} */
int hs_sens_info(const hs_handle* F, double* out8);

/* ---- tangent-linear solves and Gauss-Newton Hessian products on A's pattern (hs_gn.hip) --------------------------------------------------
 * The forward mode next to hs_sens_*.  op(A), X = op(A)^-1 B and hs_block_arg as above.  E is a perturbation on the stored pattern of A:
 * pattern 0: nnz(A) values in the order of the nzval given to the factorization; pattern 1: n diagonal values (a value at a j whose (j, j) is
 * not stored counts as 0).  op(E) = E, E^T, E^H for trans = 0 / 1 / 2.
 *   tangent       dX(E) = d/ds op(A + sE)^-1 B at s = 0 = -op(A)^-1 op(E) X      (real-linear in E; antilinear for trans = 2)
 *   identity      Re<W, dX(E)> = Re sum_p E_p conj(G_p) for the G of hs_sens_* with cotangent W
 *   Gauss-Newton  J E = dX(E)[rows, :] for distinct receiver rows; H E = J* J E with the adjoint in the real inner product: the G of
 *                 hs_sens_* for W = J E scattered to `rows`, so Re<E1, H E2> = Re<J E1, J E2>
 *   diagonal      Z = op(A)^-H S, S the unit columns of `rows`; z2[q] = sum_r |Z[q, r]|^2, x2[q] = sum_c |X[q, c]|^2; the diagonal of H at
 *                 the stored (i, j) is z2[i] x2[j] (trans 0) or z2[j] x2[i] (trans 1, 2): real, the same for the directions e_p and i e_p
 * hs_tangent_*: dX is n x nrhs (rows == NULL; nrows is ignored) or nrows x nrhs in the order of `rows` (1-based, distinct), leading
 * dimension lddx; X (may be NULL) receives the fields.  hs_gn_hessvec_*: HE has nnz(A) or n values like the G of hs_sens_* and is
 * zero-filled first; JE (nrows x nrhs, ldje) and X may be NULL.  hs_gn_diag_*: Hd is a REAL array of nnz(A) or n doubles (pattern 1:
 * z2[j] x2[j] where (j, j) is stored, 0 elsewhere); z2, x2 (n doubles each) may be NULL.
 * Xin (n x nrhs, ldxin) is the X of an earlier call on the same A and B: when it is given the forward solve is skipped -- a product then
 * costs two block solves instead of three -- and B is not read and may be NULL.
 * The columns go in groups of Gc sized as hs_sens_* sizes them (HS_GN_GROUP in the environment overrides Gc, read per call).  Per group: the
 * forward solve, P = -op(E) X (one lane per row of op(E), E read in place through the handle's CSR map for trans = 0 and in CSC order
 * otherwise), the tangent solve, the receiver rows (returned, or made the sparse cotangent on the device), the adjoint solve on the pruned
 * path and the reduction kernel of hs_sens_*; every solve is chosen as hs_sens_* chooses it (dense block: hs_ldiv_block_dev_t_*; sparse B:
 * hs_ldiv_sparse_dev_* with all rows; itmax > 0: hs_ldiv_refine_block_dev_* without ferr).  hs_gn_diag_* accumulates x2 over the forward
 * groups, then sends the unit columns of `rows` in groups through the adjoint path and accumulates z2.  Nothing of size n x nrhs leaves
 * the device unless asked for.
 * Determinism: X carries the bits of the entry points named above, P the bits of one chain per (row, column) over the row's entries by
 * ascending column of op(E), every step the unfused acc - e * x, and dX = hs_ldiv_block_t_*(op(F), P) bit for bit (itmax = 0); JE are rows
 * of dX; HE has the bits of hs_sens_*(op(F), B, W = scatter(JE)); z2 and x2 are one chain per row over the columns in order
 * (acc + (re^2 + im^2), unfused) and Hd their rounded product.  So two calls return the same bits, no result depends on Gc, a sparse B
 * gives the bits of its dense expansion, a supplied Xin the bits of the computed X, and pattern 1 the diagonal entries of pattern 0 (HE,
 * Hd).  NOT guaranteed bitwise: agreement with any host composition that forms op(E) X in another order, and of Hd[p] with
 * (H e_p)_p, which sums the same terms in another order.
 * Refused before any device work, every output untouched: what hs_ldiv_block_t_* refuses (HSS interior blocks, more than one rank), by its
 * own check: HS_ERR_UNSUPPORTED; a null, plan-only or unfactored handle, a mismatched element type, trans outside 0..2, pattern outside 0..1,
 * itmax < 0, null pointers with nonzero sizes, B and Xin both NULL, repeated rows, a CSC block hs_ldiv_sparse_* would refuse:
 * HS_ERR_ARGUMENT; n != size(F), negative sizes, rows outside 1..n, leading dimensions too small: HS_ERR_DIMENSION.  nrhs = 0, or nrows = 0
 * where rows are given, returns zero-filled outputs and HS_OK.
 * The host forms move B (or its stored values, or Xin) and E up and the outputs down; in the _dev_ forms the values, E and the outputs are
 * on the device, the index arrays (colptr, rowval, rows) on the host, and the call returns when the outputs are complete. */
int hs_tangent_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* Xin, int64_t ldxin, const double* E, int pattern, int64_t itmax,
                 const int64_t* rows, int64_t nrows, double* dX, int64_t lddx, double* X, int64_t ldx);
int hs_tangent_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* Xin, int64_t ldxin, const double* E, int pattern, int64_t itmax,
                 const int64_t* rows, int64_t nrows, double* dX, int64_t lddx, double* X, int64_t ldx); /* interleaved (re, im) */
int hs_tangent_dev_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* dXin, int64_t ldxin, const double* dE, int pattern,
                     int64_t itmax, const int64_t* rows, int64_t nrows, double* ddX, int64_t lddx, double* dX, int64_t ldx, void* stream);
int hs_tangent_dev_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* dXin, int64_t ldxin, const double* dE, int pattern,
                     int64_t itmax, const int64_t* rows, int64_t nrows, double* ddX, int64_t lddx, double* dX, int64_t ldx, void* stream);
int hs_gn_hessvec_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* Xin, int64_t ldxin, const double* E, int pattern, int64_t itmax,
                    const int64_t* rows, int64_t nrows, double* HE, double* JE, int64_t ldje, double* X, int64_t ldx);
int hs_gn_hessvec_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* Xin, int64_t ldxin, const double* E, int pattern, int64_t itmax,
                    const int64_t* rows, int64_t nrows, double* HE, double* JE, int64_t ldje, double* X, int64_t ldx);
int hs_gn_hessvec_dev_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* dXin, int64_t ldxin, const double* dE, int pattern,
                        int64_t itmax, const int64_t* rows, int64_t nrows, double* dHE, double* dJE, int64_t ldje, double* dX, int64_t ldx, void* stream);
int hs_gn_hessvec_dev_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* dXin, int64_t ldxin, const double* dE, int pattern,
                        int64_t itmax, const int64_t* rows, int64_t nrows, double* dHE, double* dJE, int64_t ldje, double* dX, int64_t ldx, void* stream);
int hs_gn_diag_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* Xin, int64_t ldxin, const int64_t* rows, int64_t nrows, int pattern,
                 int64_t itmax, double* Hd, double* z2, double* x2);
int hs_gn_diag_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* Xin, int64_t ldxin, const int64_t* rows, int64_t nrows, int pattern,
                 int64_t itmax, double* Hd, double* z2, double* x2);
int hs_gn_diag_dev_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* dXin, int64_t ldxin, const int64_t* rows, int64_t nrows,
                     int pattern, int64_t itmax, double* dHd, double* dz2, double* dx2, void* stream);
int hs_gn_diag_dev_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const double* dXin, int64_t ldxin, const int64_t* rows, int64_t nrows,
                     int pattern, int64_t itmax, double* dHd, double* dz2, double* dx2, void* stream);
/* the last hs_tangent_* / hs_gn_* call of the handle: out8 = {seconds on the device in total, of the forward solves, of the tangent solves,
 * of the adjoint solves, of the products and reductions (the copies of requested blocks included), column groups, block solves issued,
 * workspace bytes} */
int hs_gn_info(const hs_handle* F, double* out8);

/* ---- solves with a low-rank or entry modification of A, without refactoring (hs_mod.hip) ------------------------------------------------
 * A1 = A + U V^H with U, V n x k (Float64: V^T), k <= HS_MOD_MAXRANK = 256.  With Z = F^-1 U, W = F^-H V and the capacitance matrix
 * C = I_k + V^H Z (Sherman-Morrison-Woodbury):
 *   trans 0:  A1^-1 B = Y - Z C^-1 (V^H Y),              Y = F^-1 B
 *   trans 2:  A1^-H B = Y - W C^-H (U^H Y),              Y = F^-H B
 *   trans 1:  A1^-T B = Y - conj(W) C^-T (U^T Y),        Y = F^-T B
 * hs_mod_create_* builds Z with the library's own solves (dense U: hs_ldiv_block_dev_t_*; the sparse form: hs_ldiv_sparse_dev_* with all rows,
 * i.e. the pruned forward sweep), C with the inner-product kernel (the sparse form: a gather of Z[J, :]), factors C with partial pivoting
 * (an exactly zero pivot: HS_ERR_SINGULAR) and records rcond_1(C) from C^-1 applied to the identity.  It keeps copies of U, V (or J), Z and
 * LU(C) on the device; W (and, in the sparse form, the dense expansion of U) is built by the first call with trans = 1 or 2 and serves both.
 * The sparse form takes dA (n x n) as 1-based CSC with the rows strictly increasing within a column (SparseMatrixCSC): k = its nonempty
 * columns J, U = dA[:, J], V = I[:, J], so A1 = A + dA.
 * hs_mod_ldiv_* solves op(A1) X = B chunk by chunk of HS_LDIV_BLOCK_COLS columns: per chunk one block solve with F (hs_ldiv_block_dev_t_*),
 * one inner product (or gather), one solve with LU(C) and one rank-k correction.
 * The object holds a pointer to F and never changes its factors; F must outlive it (freeing F first is the caller's error).  Calls on one
 * object must not overlap (it owns one set of work blocks); the solve figures of F (hs_ldiv_block_info, hs_ldiv_sparse_info) are those of
 * the solves run here.
 * Properties: k = 0 returns the bits of hs_ldiv_block_t_*; two calls return the same bits; X[:, c] depends neither on the other columns
 * nor on their number (no atomics, one summation order per element); C may alias B; nrhs = 0 touches nothing.
 * Refused before any device work, with C unwritten: what hs_ldiv_block_t_* refuses (HSS interior blocks, more than one rank), found by a
 * zero-column solve and reported with its message: HS_ERR_UNSUPPORTED; k > HS_MOD_MAXRANK: HS_ERR_UNSUPPORTED (refactor instead); null
 * pointers, trans outside 0..2, a mismatched element type, a plan-only or unfactored handle, a malformed CSC: HS_ERR_ARGUMENT; n != size(F),
 * leading dimensions below n, negative sizes, indices outside 1..n: HS_ERR_DIMENSION.  A singular C: HS_ERR_SINGULAR (no object is made).
 * The _dev_ forms take device blocks and a stream and return when the object is built (create) or with the solve queued on the stream
 * (ldiv): hs_mod_ldiv_dev_* itself waits for nothing on the host (a call on another stream than the last one waits for it on the device);
 * the block solve inside it waits, as every hs_ldiv_block_dev_* call does, until the handle's previous block solve has left its work blocks. */
#define HS_MOD_MAXRANK 256
typedef struct hs_mod hs_mod;
int hs_mod_create_d(hs_handle* F, int64_t n, int64_t k, const double* U, int64_t ldu, const double* V, int64_t ldv, hs_mod** M);
int hs_mod_create_z(hs_handle* F, int64_t n, int64_t k, const double* U, int64_t ldu, const double* V, int64_t ldv, hs_mod** M);
int hs_mod_create_dev_d(hs_handle* F, int64_t n, int64_t k, const double* dU, int64_t ldu, const double* dV, int64_t ldv, void* stream, hs_mod** M);
int hs_mod_create_dev_z(hs_handle* F, int64_t n, int64_t k, const double* dU, int64_t ldu, const double* dV, int64_t ldv, void* stream, hs_mod** M);
int hs_mod_create_sparse_d(hs_handle* F, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, hs_mod** M);
int hs_mod_create_sparse_z(hs_handle* F, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, hs_mod** M);
int hs_mod_ldiv_d(hs_mod* M, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_mod_ldiv_z(hs_mod* M, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_mod_ldiv_dev_d(hs_mod* M, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
int hs_mod_ldiv_dev_z(hs_mod* M, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
/* out8 = {k, rcond_1(C) (1 for k = 0), seconds to build, device seconds of the last hs_mod_ldiv_* (the block solves included), device bytes
 * held, 1 when W exists, block-solve calls issued so far (create included), 0} */
int hs_mod_info(hs_mod* M, double* out8);
void hs_mod_free(hs_mod* M);

/* ---- a factorization with its stored factors in Float32 (hs_f32.hip) ----------------------------------------------------------------------
 * hs_f32_create makes a stand-alone DEMOTED COPY G of a factorization F: everything the block solve reads, stored in Float32 (ComplexF32
 * for a ComplexF64 handle) -- per front the packed LU of the interior block with the boundary rows of L below it, the boundary columns of
 * U (where the Gauss transforms are dense), the inverted 256 x 256 diagonal blocks of L and U; per low-rank Gauss transform its two
 * generators; the row permutations and index lists as they are.  Every element is rounded once, to nearest even.  G keeps no pointer into
 * F: F may be freed (hs_free, hs_trim) and G goes on solving, with the same bits.  F itself is not changed.
 * hs_f32_ldiv_* solves op(F) X = B (trans 0: F, 1: transpose(F), 2: adjoint(F)) with the schedule of hs_ldiv_block_t_*: chunks of
 * HS_LDIV_BLOCK_COLS columns, the same work blocks, the same products.  Right-hand sides, work blocks, accumulators and results are
 * Float64 / ComplexF64; a factor element is widened in a register on its way into v_mfma_f64_16x16x4_f64, which is exact.  What is lost is
 * the rounding of the factors: one solve carries a relative error of about cond(A) 2^-24.  hs_gmres_block_f32_* puts a full-precision
 * Krylov solver on top.
 * Bitwise statements: the summation order of every output element is that of hs_ldiv_block_t_*, so G returns the bits hs_ldiv_block_t_*
 * returns on a handle whose stored factors hold the rounded values (hsk_round_factors_f32, include/hs_kernels.h, makes one); two calls
 * return the same bits; X[:, c] depends neither on the other columns nor on their number; C may alias B; nrhs = 0 touches nothing.
 * Refused, with *G = NULL: what hs_ldiv_block_dev_t_* refuses (HSS interior blocks, more than one rank, an unfactored or plan-only handle),
 * found by a zero-column solve and reported with its status and message; a stored element that is finite in Float64 and overflows Float32:
 * HS_ERR_UNSUPPORTED, the count in the message and in hs_last_error_info (scale the matrix).  Elements that become zero or subnormal are
 * counted and reported (hs_f32_info), not refused.  The solves refuse a null object, trans outside 0..2, an element type that does not
 * match the _d / _z suffix (HS_ERR_ARGUMENT) and n != size(F), leading dimensions below n, negative sizes (HS_ERR_DIMENSION), before any
 * device work and with C unwritten.  Calls on one object must not overlap (it owns one set of work blocks).
 * hs_f32_create returns when the copy is complete (stream: where the demotion runs); the _dev_ solves take device blocks and return with
 * the solve queued on their stream. */
typedef struct hs_f32 hs_f32;
int hs_f32_create(hs_handle* F, void* stream, hs_f32** G);
int hs_f32_ldiv_d(hs_f32* G, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_f32_ldiv_z(hs_f32* G, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs);
int hs_f32_ldiv_dev_d(hs_f32* G, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
int hs_f32_ldiv_dev_z(hs_f32* G, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream);
/* out8 = {device seconds of the last solve, Float32 value bytes held (the demoted elements, 4 bytes per real scalar), the Float64 bytes of
 * the same elements in F (exactly twice that), index, descriptor and alignment-padding bytes, work-block bytes, elements flushed to zero
 * or to a subnormal, column chunks of the last solve, seconds of the demotion} */
int hs_f32_info(hs_f32* G, double* out8);
void hs_f32_free(hs_f32* G);

/* ---- eigenpairs nearest a shift from the stored factors (hs_eigs.hip) --------------------------------------------------------------
 * F factors A_s = A - sigma I (the caller subtracts the shift before factoring; sigma is bookkeeping, so that lambda comes back unshifted).
 * The call returns the nev eigenvalues of A nearest sigma -- the eigenvalues theta of op(F)^-1 of largest modulus, mu = 1 / theta,
 * lambda = sigma + mu -- with unit eigenvectors, by block Arnoldi with thick restart on op(F)^-1: per step one block solve with `block`
 * columns, two passes of classical Gram-Schmidt against the basis, CholQR twice; a restart when ncv basis columns are full, from the
 * eigenpairs of the projected matrix (computed on the host).  A column that turns out dependent on the basis (an invariant subspace, a
 * start block of eigenvectors) is replaced by a seeded random vector.
 *   trans     0: A x = lambda x.  1, 2: transpose(F) / adjoint(F), i.e. left eigenvectors (y^T A = lambda y^T, y^H A = lambda y^H); trans = 2
 *             returns the eigenvalues of A^H, conj(lambda).
 *   ncv, block  0 selects the defaults: block = 16, ncv = the multiple of block >= max(2 nev + block, 4 block), capped by ncv + block <= 256
 *             and by n.  block <= 64.
 *   tol       a Ritz pair counts as converged when est = ||B y||_2 / |theta| <= tol (B: the last block row of the projected relation).
 *   V0        the start block, n x block (ldv0), or NULL: a seeded random block.  where: 0 host pointers (V0, X), 1 device pointers.
 *   lam       2 (nev + 1) doubles: (re, im) per eigenvalue, nearest first.  X (n x (nev + 1), ldx; may be NULL): the vectors, unit 2-norm.
 *   _d        sigma_im must be 0; vectors in LAPACK's real convention: a conjugate pair occupies two columns, real part then imaginary part
 *             of the vector of the eigenvalue with the positive imaginary part, and shares resid and est; *nout = nev, or nev + 1 when a
 *             pair would otherwise be split.
 *   resid     nev + 1 doubles: ||op(A_s) x - mu x||_2 with the handle's own matrix (the factored one); est: the estimates above.
 *   *nconv    how many of the *nout pairs met tol; fewer than *nout after maxrestart restarts is HS_OK -- the caller decides.
 * Served: what hs_ldiv_block_dev_t_* serves, exact and compressed (a compressed handle yields the eigenpairs of its own F^-1, resid tells
 * how far they are from those of A_s); its refusals (HSS interior blocks, more than one rank) are found by a zero-column solve and passed
 * on with its message as HS_ERR_UNSUPPORTED before anything is written.  HS_ERR_ARGUMENT: nev < 1, ncv + block > 256, block > 64,
 * ncv < nev + block, n < ncv + block, null outputs, trans outside 0..2, a complex shift in hs_eigs_d, a plan-only or unfactored handle.
 * HS_ERR_DIMENSION: n != size(F) or the element type of the other entry point.  Two calls return the same bits; nothing depends on the
 * launch grid.  The call returns when the results are on the host (or in X); it owns its workspace: (ncv + block + 1 + 2 (nev + 1)) n
 * elements and the slab partials.
 * hs_eigs_info: out8 = {device seconds, block solves, column applications, restarts, Gram-Schmidt passes, replaced columns, workspace
 * bytes, ncv used} of this thread's last call. */
int hs_eigs_d(hs_handle* F, int trans, int64_t n, int64_t nev, int64_t ncv, int64_t block, double sigma_re, double sigma_im, double tol, int64_t maxrestart,
              const double* V0, int64_t ldv0, int64_t seed, int where, double* lam, double* X, int64_t ldx, double* resid, double* est, int64_t* nout, int64_t* nconv,
              void* stream);
int hs_eigs_z(hs_handle* F, int trans, int64_t n, int64_t nev, int64_t ncv, int64_t block, double sigma_re, double sigma_im, double tol, int64_t maxrestart,
              const double* V0, int64_t ldv0, int64_t seed, int where, double* lam, double* X, int64_t ldx, double* resid, double* est, int64_t* nout, int64_t* nconv,
              void* stream);
int hs_eigs_info(double* out8);
/* The generalized problem A x = lambda M x from the factors of A_s = A - sigma M (the caller forms and factors the shifted pencil; sigma is
 * bookkeeping as above).  M: host CSC arrays (SparseMatrixCSC fields, 1-based; mnzval interleaved complex in _z) in the factored ordering
 * -- the rows and columns the caller gave the factorization; it is only multiplied with, so it may be singular, non-symmetric or have
 * entries outside A's pattern.  `where` concerns V0 and X alone.  All three arrays NULL: M = I, the call is hs_eigs_* (which are this
 * call with M = NULL) bit for bit.  The call returns the nev eigenvalues of the pencil (A, M) nearest sigma: theta the eigenvalues of
 * largest modulus of op(F)^-1 op(M), mu = 1 / theta, lambda = sigma + mu; an infinite eigenvalue is theta = 0 and never selected.
 *   trans     0: A x = lambda M x.  1: the pencil (A^T, M^T), y^T A = lambda y^T M.  2: (A^H, M^H), returns conj(lambda).
 *   inner     0: the Euclidean inner product.  An expansion forms T = op(M) V[:, m:m+p] and solves from T; vectors have unit 2-norm, est and
 *             the stopping test are those of hs_eigs_*.
 *             1: the op(M) inner product, for Hermitian positive definite M: every inner product of the Gram-Schmidt and CholQR passes is
 *             taken against MW = op(M) W, recomputed by one SpMM after every correction of W (never updated: one summation order per
 *             element); the basis is M-orthonormal, a Hermitian pencil gives a Hermitian projected matrix, the vectors come back with
 *             x^H op(M) x = 1 (a Float64 pair scaled as the complex vector it stands for), est is an M-norm quantity:
 *             ||B y||_2 / |theta| is the M-norm of the residual of the Ritz pair of op(F)^-1 op(M).  The rank-deficiency rule applies to
 *             the M-Gram matrix.  A Gram diagonal entry of the start block that is not positive: M is not positive definite on it,
 *             HS_ERR_ARGUMENT.  With M = NULL inner = 1 is the Euclidean run.
 *   resid     ||op(A_s) x - mu op(M) x||_2 with the handle's own A_s, in both modes.
 * HS_ERR_ARGUMENT in addition to hs_eigs_*: inner outside 0..1; one or two of the three M arrays; mcolptr[0] != 1 or not monotone; a row
 * index outside 1..n; n beyond 32-bit indices -- all found with the other argument checks, before the handle's own refusals (which are
 * those of hs_eigs_*, in the same order and words) and before anything is written.  Workspace beyond hs_eigs_*: (block + nev + 1) n
 * elements (T and op(M) X), (2 block + nev + 1) n with inner = 1 (MW), and M on the device (CSR for trans = 0, the CSC arrays read in
 * place as rows of op(M) otherwise; uploaded once per call).
 * hs_eigs_gen_info: out4 = {products with op(M), columns multiplied, device bytes held for M, inner used} of this thread's last
 * hs_eigs_gen_* / hs_eigs_* call. */
int hs_eigs_gen_d(hs_handle* F, int trans, int64_t n, const int64_t* mcolptr, const int64_t* mrowval, const double* mnzval, int inner, int64_t nev, int64_t ncv,
                  int64_t block, double sigma_re, double sigma_im, double tol, int64_t maxrestart, const double* V0, int64_t ldv0, int64_t seed, int where, double* lam,
                  double* X, int64_t ldx, double* resid, double* est, int64_t* nout, int64_t* nconv, void* stream);
int hs_eigs_gen_z(hs_handle* F, int trans, int64_t n, const int64_t* mcolptr, const int64_t* mrowval, const double* mnzval, int inner, int64_t nev, int64_t ncv,
                  int64_t block, double sigma_re, double sigma_im, double tol, int64_t maxrestart, const double* V0, int64_t ldv0, int64_t seed, int where, double* lam,
                  double* X, int64_t ldx, double* resid, double* est, int64_t* nout, int64_t* nconv, void* stream);
int hs_eigs_gen_info(double* out4);

/* ---- accuracy tools: norm and condition estimates, refined solves with error bounds (hs_condest.hip) --------------------------
 * opnorm(A, 1), opnorm(A, Inf) of the handle's A (the values of the last hs_numeric_begin); p = 1 or 0 (= Inf).  The first call that needs
 * rows of A (p = 0, hs_condest p = 0, hs_ldiv_refine_* with trans = 0) builds a CSR map of A's pattern on the device and keeps it in the handle. */
int hs_opnorm(hs_handle* F, int p, double* norm);
/* Julia's opnormestinv: the Higham-Tisseur block 1-norm estimate (SIAM J. Matrix Anal. Appl. 21(4), 2000, Alg. 2.4) of op(F)^-1,
 * op = F (trans 0), transpose(F) (1), adjoint(F) (2), with t columns (1:min(8, n); Julia's default min(2, n)) and at most itmax iterations
 * (>= 1; Julia's 5).  A lower bound of ||op(F)^-1||_1, usually within a factor of 3; *nsolves (may be NULL) = columns solved.  Deterministic:
 * the +-1 columns come from a hash of hs_options.seed, every reduction runs in a fixed order, two calls return the same bits. */
int hs_normestinv(hs_handle* F, int trans, int64_t t, int64_t itmax, double* est, int64_t* nsolves, void* stream);
/* cond(A, p) ~ ||A||_p * ||F^-1||_p, p = 1 or 0 (= Inf; ||F^-1||_Inf = ||F^-T||_1), itmax = 5.  For a compressed factorization (swlevel > 0)
 * this estimates cond(A) only as well as F approximates A.  normA, normFinv may be NULL. */
int hs_condest(hs_handle* F, int p, int64_t t, double* cond, double* normA, double* normFinv, void* stream);
/* LAPACK xGERFS on op(A) X = B, op by trans as in hs_ldiv_t_*: X = op(F) \ B, then per column r = b - op(A) x, the componentwise backward
 * error berr = max_i |r_i| / (|b| + |op(A)| |x|)_i (cabs1 for ComplexF64), and x += op(F) \ r while berr > eps, berr at least halves and
 * fewer than itmax (>= 0; 5 as in LAPACK) corrections were made.  ferr (may be NULL) = the estimate of || |op(A)^-1| (|r| + nz eps w) ||_Inf
 * / ||x||_Inf (the hs_normestinv engine, t = min(2, n), on diag(v) op(F)^-H).  berr, ferr and steps are host arrays of nrhs entries.
 * Refused with HS_ERR_UNSUPPORTED before any device work: factorizations over more than one rank; and where transposed solves are refused
 * (fronts that keep D as an HSS matrix), trans != 0 or ferr != NULL (hs_normestinv and hs_condest too).  Bad t, p, itmax, trans or
 * dimensions: HS_ERR_ARGUMENT / HS_ERR_DIMENSION.  The _dev_ forms take device X, B on `stream`; X may not alias B. */
int hs_ldiv_refine_d(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                     double* berr, double* ferr, int64_t* steps);
int hs_ldiv_refine_z(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                     double* berr, double* ferr, int64_t* steps);
int hs_ldiv_refine_dev_d(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                         double* berr, double* ferr, int64_t* steps, void* stream);
int hs_ldiv_refine_dev_z(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                         double* berr, double* ferr, int64_t* steps, void* stream);

/* hs_ldiv_refine_* for a block of right-hand sides in lockstep (hs_refine_block.hip): column c gets the xGERFS iteration hs_ldiv_refine_*
 * runs for B[:, c] alone (the same start, residual, weights, guarded ratio, continuation rule and ferr definition), but every application of
 * op(F)^-1 is one hs_ldiv_block_dev_t_* call on all columns that are still active: the factors are read once per chunk of columns.  A
 * correction is one block solve, one fused residual pass over op(A) and one host synchronisation; a column whose test ends is frozen and the
 * columns that go on are compacted into the leading slots, so a correction runs ceil(nact / chunk) chunks.  With ferr every column runs its
 * own Higham-Tisseur estimator (t = min(2, n), 5 iterations, the +-1 keys of hs_normestinv); all active estimators share one block
 * application of op(F)^-H and one of op(F)^-1 per iteration.  Results agree with hs_ldiv_refine_* to the rounding by which block and single
 * solves differ, not bit for bit; steps may differ by one where a column sits on the stopping threshold; with rows of op(A) longer than 64
 * entries the residual's summation order differs too.  No floating-point atomics, fixed reduction orders: two calls return the same bits,
 * and X[:, c], berr[c], ferr[c], steps[c] do not depend on the values, number or order of the other columns nor on the group width.
 * Columns are processed in groups of G (a multiple of HS_LDIV_BLOCK_COLS) whose workspace (R, D, W, V of n x G; with ferr five blocks of
 * n x 2G; partials) fits half of the free device memory, else HS_ERR_NOMEM; HS_REFINE_BLOCK_GROUP overrides G (read per call).
 * Refused before any device work, X untouched: what hs_ldiv_block_t_* refuses (HSS interior blocks, more than one rank) with
 * HS_ERR_UNSUPPORTED whatever trans and ferr are (no fallback: hs_ldiv_refine_* serves those handles); null pointers, X aliasing B, trans
 * outside 0..2, itmax < 0, a plan-only or unfactored handle, a mismatched element type: HS_ERR_ARGUMENT; bad n / ldx / ldb / nrhs < 0:
 * HS_ERR_DIMENSION.  nrhs = 0 touches nothing.  berr, ferr (may be NULL) and steps are host arrays; the _dev_ forms take device X, B. */
int hs_ldiv_refine_block_d(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                           double* berr, double* ferr, int64_t* steps);
int hs_ldiv_refine_block_z(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                           double* berr, double* ferr, int64_t* steps);
int hs_ldiv_refine_block_dev_d(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                               double* berr, double* ferr, int64_t* steps, void* stream);
int hs_ldiv_refine_block_dev_z(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                               double* berr, double* ferr, int64_t* steps, void* stream);
/* the calling thread's last hs_ldiv_refine_block_* call: out8 = {seconds on the device, block-solve calls, column-applications summed over
 * them, residual launches, the largest active-column count, column groups, workspace bytes, estimator column-applications} */
int hs_ldiv_refine_block_info(double* out8);

/* ---- log-determinant and selected inversion from the stored factors (hs_selinv.hip) ----------------------------------------------
 * LinearAlgebra.logabsdet(F): *logabs = log|det F|, sign2 = {re, im} of det F / |det F| ({+-1, 0} for Float64); an exactly zero pivot gives
 * logabs = -Inf, sign = 0.  det F = prod over fronts of sign(P) prod diag(U) of the pivoted LU of every front's interior block; one grouped
 * launch reads the n diagonal entries and the n permutation entries, every reduction runs in a fixed order (two calls return the same bits).
 * Compressed factorizations (swlevel > 0) whose fronts keep a dense or compact LU of D are supported and return logabsdet(F), which
 * approximates A's only as well as F approximates A.  Refused with HS_ERR_UNSUPPORTED before any device work: fronts that keep D as an HSS
 * matrix (hs_options.hss_d, mf = 2, 3), factorizations over more than one rank.  With hs_options.equilibrate the factors are those of
 * A_s = 2^er A 2^ec: logabs is returned less ln 2 (sum er + sum ec), the sums taken exactly in int64; the sign is that of A_s, which is A's. */
int hs_logabsdet(hs_handle* F, double* logabs, double* sign2);
/* Selected inverse of an exact factorization (swlevel = 0): diag (n elements of T, or NULL) = diag(A^-1); zval (nnz(A) elements of T in A's
 * CSC order, or NULL) = (A^-1)_ij for every stored entry (i, j) of A (trans = 0) or (A^-1)_ji (trans = 1: the selected inverse of A^T on
 * A's pattern).  where: 0 host pointers, 1 device pointers.  The tree is walked from the root to the leaves; per front
 * Z[int, bnd] = -R Zbb, Z[bnd, int] = -Zbb Lm, Z[int, int] = Aii^-1 + R Zbb Lm with Zbb gathered from the parent's block, as grouped GEMMs
 * over the stored factors and the stored inverses of their 256 x 256 diagonal blocks; about three factorizations' worth of flops.  The
 * factors are only read.  budget_bytes bounds the scratch alive at a time (0: derived from hipMemGetInfo at call time): a level that does
 * not fit is processed in several batches of fronts.  The first call builds, on the host, the list of A's entries every front owns and
 * keeps it in the handle.  Work runs on `stream` (NULL: the handle's); the call returns when the results are complete.
 * Refused with HS_ERR_UNSUPPORTED before any device work: what hs_logabsdet refuses; any front with low-rank Gauss transforms L / R (see
 * hs_flow_info) or eliminated in slices (hs_options.split); a pattern with a stored entry outside every front's [int; bnd] x [int; bnd]
 * block (a tree that does not cover A's pattern -- no value is returned with a hole).  A root that keeps a boundary is an ordinary front
 * under the handle's pseudo-root and is supported.  A handle that is only planned or not yet factored, trans not in 0:1, where not in 0:1,
 * diag == zval == NULL: HS_ERR_ARGUMENT. */
int hs_selinv(hs_handle* F, int trans, void* diag, void* zval, int where, int64_t budget_bytes, void* stream);
/* the last hs_selinv call of the handle: out4 = {seconds on the device, flops executed (real), peak scratch bytes, batches of fronts} */
int hs_selinv_info(const hs_handle* F, double* out4);
/* Selected inverse of a compressed factorization (swlevel != 0): the arguments, their meanings and their checks are hs_selinv's; the result
 * is diag(F^-1) and F^-1 on A's pattern, F the operator the solves apply (trans = 1 with hs_logabsdet gives the gradient of log|det F| with
 * respect to A's entries).  A compressed front keeps Uib ~= G Z_R (ni x rR, rR x nb), Lbi ~= C_L Z_L' (nb x rL, rL x ni) and the pivoted LU
 * of Aii; with W = U^-1 G and Y = Z_L' L^-1 P the recurrence reads Z[int, bnd] = -W (Z_R Zbb), Z[bnd, int] = -(Zbb C_L) Y,
 * Z[int, int] = Aii^-1 + W (Z_R Zbb C_L) Y: the substitutions run on rR columns and ni + rL rows, the products through r-wide blocks.  Dense
 * fronts of the same handle (leaves, fronts below swsize) run hs_selinv's recurrence in the same launches; on an exact handle the call
 * issues hs_selinv's launches and returns its bits.  The factors are only read (their low-rank parts are copied before a substitution
 * overwrites them).  Served: single-rank handles whose fronts keep a dense pivoted LU of Aii and are dense or low-rank with dense factors
 * (the default compressed flow and hs_options.mf = 1).  Refused with HS_ERR_UNSUPPORTED before any device work: fronts that keep D as an
 * HSS matrix (hs_options.hss_d, mf = 2, 3), fronts eliminated in slices, factorizations over more than one rank, a low-rank transform that
 * keeps only its packed sketch (HS_LR_QR=0 diagnostics), and the two pattern / tree holes hs_selinv reports. */
int hs_selinv_lr(hs_handle* F, int trans, void* diag, void* zval, int where, int64_t budget_bytes, void* stream);
/* the last hs_selinv_lr call of the handle: out8 = {seconds on the device, flops executed (real), peak scratch bytes, batches of fronts,
 * fronts served through low-rank transforms, largest rank used, flops the dense-form recurrence of hs_selinv would execute on the same front
 * shapes (counted on the host), 0}.  hs_selinv_info and hs_selinv_lr_info keep separate figures. */
int hs_selinv_lr_info(const hs_handle* F, double* out8);

/* ---- Schur-complement mode: the interface matrix, condense and expand solves (hs_interface.hip) --------------------------------------
 * The interface b is the boundary the ROOT of the tree keeps (root.bnd; hs.problems.graph_nested_dissection(..., interface=...) builds such
 * trees), everything else (i) is eliminated.  The handle's pseudo-root -- the level-0 front whose interior is root.bnd -- holds the pivoted
 * LU of the dense Schur complement S = A_bb - A_bi A_ii^-1 A_ib; these calls open it:
 *   hs_interface_size     *nb = |root.bnd| (0 when the root keeps no boundary); also on a plan-only handle (hs_plan)
 *   hs_interface_indices  the nb ids of the interface, 1-based, in the order of S's rows and columns (= root.bnd as given); plan-only too
 *   hs_interface_matrix   S (nb x nb, column-major, lds >= nb) = P^T (L U) from the stored factors of the pseudo-root: one product on the
 *                         matrix pipe that walks only the k <= min(i, j) part of K (about a third of the flops of a full product); no second
 *                         factorization, no copy of S kept by the handle; the factors are only read; two calls return the same bits.
 *                         where: 0 S is a host array, 1 a device array; stream: NULL = the handle's.  nb = 0 touches nothing.  For a
 *                         compressed handle (swlevel > 0) S is the Schur complement of the COMPRESSED factorization: it approximates A's only
 *                         as well as F approximates A.
 * The three phases split the block solve hs_ldiv_block_t_* at the pseudo-root, in place on one n x nrhs column-major block C (ldc >= n):
 *   condense  forward sweep of tree levels nlevels .. 1: on return C[idx, :] = g = B_b - op(A)_bi op(A)_ii^-1 B_i; the interior rows of C hold
 *             every front's forward intermediate at the front's own int ids -- opaque values only expand reads; nothing stays in the handle
 *   solve     level 0 only: C[idx, :] = op(S)^-1 C[idx, :]
 *   expand    reads C[idx, :] as the interface values y, reloads the intermediates from the interior rows and runs the backward sweep of
 *             levels 1 .. nlevels: C[interior, :] = op(A)_ii^-1 (B_i - op(A)_ib y); C[idx, :] is left as it is
 * condense; solve; expand returns the bits of hs_ldiv_block_t_* for the same trans (the same chunks and launches, two exact copies per front
 * more).  Between condense and expand the caller may overwrite C[idx, :] (its own interface solve, e.g. (S + K) y = g + h).  trans: 0 F, 1
 * transpose(F), 2 adjoint(F).  The _dev_ forms take a device block and a stream and return without waiting.  Active sets (hs_ldiv_sparse_*)
 * are not served in this mode.  A phase call runs on the block solve's work blocks and files its figures as the handle's last block solve
 * (hs_ldiv_block_info) as well.
 * Refused before any device work, outputs untouched: HS_ERR_UNSUPPORTED for what hs_ldiv_block_t_* refuses (fronts that keep D as an HSS
 * matrix, more than one rank) and, for hs_interface_matrix_*, a pseudo-root eliminated in slices (hs_options.split) or not kept as one dense
 * LU; HS_ERR_ARGUMENT for null pointers, trans outside 0..2, where outside 0..1, a plan-only or unfactored handle (all but size / indices), a
 * mismatched element type; HS_ERR_DIMENSION for n != size(F), ldc < n, lds < nb, nrhs < 0.
 * hs_interface_info: out8 = {seconds and executed real flops of the last hs_interface_matrix_* call, nb, seconds of the last condense, solve
 * and expand, column chunks of the last phase call, 0}. */
int hs_interface_size(const hs_handle* F, int64_t* nb);
int hs_interface_indices(const hs_handle* F, int64_t* idx);
int hs_interface_matrix_d(hs_handle* F, double* S, int64_t lds, int where, void* stream);
int hs_interface_matrix_z(hs_handle* F, double* S, int64_t lds, int where, void* stream);
int hs_interface_condense_d(hs_handle* F, int trans, double* C, int64_t ldc, int64_t n, int64_t nrhs);
int hs_interface_condense_z(hs_handle* F, int trans, double* C, int64_t ldc, int64_t n, int64_t nrhs);
int hs_interface_solve_d(hs_handle* F, int trans, double* C, int64_t ldc, int64_t n, int64_t nrhs);
int hs_interface_solve_z(hs_handle* F, int trans, double* C, int64_t ldc, int64_t n, int64_t nrhs);
int hs_interface_expand_d(hs_handle* F, int trans, double* C, int64_t ldc, int64_t n, int64_t nrhs);
int hs_interface_expand_z(hs_handle* F, int trans, double* C, int64_t ldc, int64_t n, int64_t nrhs);
int hs_interface_condense_dev_d(hs_handle* F, int trans, double* dC, int64_t ldc, int64_t n, int64_t nrhs, void* stream);
int hs_interface_condense_dev_z(hs_handle* F, int trans, double* dC, int64_t ldc, int64_t n, int64_t nrhs, void* stream);
int hs_interface_solve_dev_d(hs_handle* F, int trans, double* dC, int64_t ldc, int64_t n, int64_t nrhs, void* stream);
int hs_interface_solve_dev_z(hs_handle* F, int trans, double* dC, int64_t ldc, int64_t n, int64_t nrhs, void* stream);
int hs_interface_expand_dev_d(hs_handle* F, int trans, double* dC, int64_t ldc, int64_t n, int64_t nrhs, void* stream);
int hs_interface_expand_dev_z(hs_handle* F, int trans, double* dC, int64_t ldc, int64_t n, int64_t nrhs, void* stream);
int hs_interface_info(const hs_handle* F, double* out8);

/* ---- phased form of factor (hs_factor_* = hs_analyze + hs_numeric_* over all levels) -------------------------
 * hs_analyze builds the plan and uploads the sparsity pattern, so a later numeric factorization starts with
 * every input resident in HBM; the pattern (colptr, rowval, tree) is reused for new values of A.
 * rank / nranks (a power of two): with nranks > 1 the 2^p subtrees rooted at tree level p+1 go one per rank
 * (factorization.jl:20-21 factors them one after the other; they are independent), and a front above the cut
 * is eliminated by the first rank of its group (hs_options.dist_top = 0) or by all ranks of its group (dist_top = 1).
 *   dist_top = 0: the library moves no data between ranks: the host layer does, with its own communication library
 *     (torch.distributed / RCCL here, MPI.jl for a Julia host), using hs_exchange_info for WHAT crosses ranks and
 *     hs_set_schur_buffer / hs_pack_bnd / hs_unpack_bnd for WHERE, and drives hs_numeric_levels / hs_solve_*_levels level by level.
 *   dist_top = 1: the library moves everything through the communicator given with hs_set_comm (below): one
 *     hs_numeric_levels(F, nlevels, 0) factors, hs_ldiv_* / hs_ldiv_dev_* solve (every rank passes the same right-hand side and
 *     receives the whole solution). */
int hs_analyze(int is_complex, int64_t n, const int64_t* colptr, const int64_t* rowval, const hs_tree* tree,
               const hs_options* opts, int64_t rank, int64_t nranks, hs_handle** out);
/* Host-side plan only (ownership, exchange list, sizes): touches no device, for schedule tests and sizing. */
int hs_plan(int is_complex, int64_t n, const hs_tree* tree, const hs_options* opts, int64_t rank, int64_t nranks,
            hs_handle** out);
int hs_numeric_begin(hs_handle* F, const void* nzval, int nzval_on_device);
int hs_numeric_levels(hs_handle* F, int64_t level_from, int64_t level_to); /* deepest-first: from >= to; root = 1 */
int hs_numeric_end(hs_handle* F); /* synchronise; HS_ERR_SINGULAR if a front hit an exactly zero pivot */

/* sweeps of ldiv! on a device vector b (n elements of T), restricted to a range of tree levels */
int hs_solve_fwd_levels(hs_handle* F, void* d_b, int64_t level_from, int64_t level_to, void* stream); /* from >= to */
int hs_solve_bwd_levels(hs_handle* F, void* d_b, int64_t level_from, int64_t level_to, void* stream); /* from <= to */

int64_t hs_nlevels(const hs_handle* F);   /* depth(nd) */
int64_t hs_cut_level(const hs_handle* F); /* levels > cut are rank-local; 1 when nranks == 1 */
int64_t hs_node_owner(const hs_handle* F, int64_t node);
int64_t hs_num_exchanges(const hs_handle* F);
/* out6 = {node, level of node, src rank, dst rank, nb, elements of T in the node's Schur buffer (lds*nb)}:
 * node's Schur complement goes src -> dst before dst eliminates node's parent; in ldiv! the vector b[bnd(node)]
 * goes src -> dst in the forward sweep and dst -> src in the backward sweep. */
int hs_exchange_info(const hs_handle* F, int64_t k, int64_t* out6);
/* Order the library's stream against a stream of the host layer without blocking the host: direction 0 = `other_stream` waits for all work
 * the library has enqueued (call before a send that reads a Schur / boundary buffer), 1 = the library's stream waits for all work enqueued on
 * `other_stream` (call after a receive into such a buffer).  NULL = the legacy default stream. */
int hs_stream_order(hs_handle* F, void* other_stream, int direction);
/* 0: exchange k moves a dense Schur complement (hs_set_schur_buffer); 1: it moves an HSS matrix packed into one buffer whose size is known
 * only after the sender compressed it (hs_options.mf with nranks > 1: src calls hs_schur_pack_size + hs_schur_pack after the node's level,
 * ships the byte count and the buffer, dst calls hs_schur_unpack before the parent's level).  This is the reference's data flow over ranks:
 * the parent reads its children's S as HssMatrix objects (src/factorization.jl:78-112,126-140); out6[5] is 0 for such an exchange. */
int64_t hs_exchange_kind(const hs_handle* F, int64_t k);
int hs_schur_pack_size(hs_handle* F, int64_t node, int64_t* bytes);
int hs_schur_pack(hs_handle* F, int64_t node, void* dev_buf, int64_t bytes, void* stream);   /* returns when the buffer is complete */
int hs_schur_unpack(hs_handle* F, int64_t node, const void* dev_buf, int64_t bytes, void* stream);
/* What a factorization does with its options on THIS rank: out8 = {hs_options.mf in effect (0 = the dense-S flow), matrix-free fronts, fronts whose S
 * leaves as an HSS matrix, fronts with low-rank L / R, fronts with an HSS D (hss_d), group fronts (dist_top), ranks, fronts eliminated in slices}. */
int hs_flow_info(const hs_handle* F, int64_t* out8);
/* What hs_options.symmetric did: out4 = {the option in effect, dense fronts of the last factorization eliminated on their lower triangle,
 * fronts eliminated as before (dense ones of a tournament-pivoted or redone level or with compressed children; compressed, HSS and matrix-free
 * fronts), 0}.  Counts are of the last hs_numeric_begin .. hs_numeric_end on this rank. */
int hs_sym_info(const hs_handle* F, int64_t* out4);
/* What hs_options.equilibrate did in the last hs_numeric_begin: out6 = {the option in effect, sweeps run (the one that moved nothing
 * included), min er, max er, min ec, max ec}; all 0 with the option off.  hs_equil_scales copies the exponents to host arrays of n int32
 * each (either may be NULL); with the option off it returns HS_ERR_ARGUMENT. */
int hs_equil_info(const hs_handle* F, int64_t* out6);
int hs_equil_scales(const hs_handle* F, int32_t* er, int32_t* ec);
/* make `dptr` (device memory owned by the caller, hs_exchange_info's element count) the node's Schur buffer */
int hs_set_schur_buffer(hs_handle* F, int64_t node, void* dptr);
int hs_pack_bnd(const hs_handle* F, int64_t node, const void* d_b, void* d_buf, void* stream);   /* buf[j] = b[bnd_j] */
int hs_unpack_bnd(const hs_handle* F, int64_t node, void* d_b, const void* d_buf, void* stream); /* b[bnd_j] = buf[j] */
int hs_extract_owned(const hs_handle* F, const void* d_b, void* d_out, void* stream); /* out[int(mine)] = b[int(mine)] */

/* ---- communicator: the one data-movement primitive of a multi-rank factorization (hs_options.dist_top) -------------------------
 * Every exchange is a set of point-to-point pieces ("send these device ranges to those ranks, receive those from these"), ordered on a
 * HIP stream.  Two transports:
 *   hs_comm_create_rccl : RCCL over xGMI (grouped ncclSend / ncclRecv on one world communicator the library creates; librccl is opened
 *                         with dlopen at this call).  Rank 0 obtains an id with hs_comm_unique_id and the host distributes its 128 bytes
 *                         with whatever it has (MPI.bcast in a Julia host, torch.distributed here), then every rank calls create.
 *   hs_comm_create_host : the same operation staged through host memory and moved by a callback of the host layer (MPI.jl; gloo in
 *                         the single-GPU rehearsals of this repository, where RCCL refuses several ranks on one device).
 * The callback receives one message per peer and direction (HOST pointers), must complete all of them and return 0. */
typedef struct hs_comm hs_comm;
typedef int (*hs_transfer_fn)(void* user, int64_t nsend, const int64_t* send_peer, void* const* send_buf, const int64_t* send_bytes,
                              int64_t nrecv, const int64_t* recv_peer, void* const* recv_buf, const int64_t* recv_bytes);
int hs_comm_unique_id(void* id128);
int hs_comm_create_rccl(const void* id128, int64_t rank, int64_t nranks, hs_comm** out);
int hs_comm_create_host(hs_transfer_fn fn, void* user, int64_t rank, int64_t nranks, hs_comm** out);
void hs_comm_free(hs_comm* c);
const char* hs_comm_kind(const hs_comm* c); /* "rccl" or "host" */
int hs_comm_selftest(hs_comm* c, int64_t bytes); /* ring shift of a byte pattern (to itself when nranks == 1), checked on the host */
int hs_comm_bandwidth(hs_comm* c, int64_t bytes, int64_t reps, double* gbps); /* ring shifts timed on the transfer stream: GB/s sent per rank (0 when nranks == 1) */
/* attach a communicator (borrowed: it must outlive the handle's factorizations); rank / nranks must equal the handle's */
int hs_set_comm(hs_handle* F, hs_comm* c);

/* gmres(A, b; Pr=F, reltol, abstol, restart, maxiter, log=true) -- the call of the reference's scenario (test/rungmres.jl:47-48; IterativeSolvers.jl
 * 0.9.0, not part of the reference tree): restarted GMRES, RIGHT-preconditioned by the factorization `Pr` (NULL: none), every vector resident on
 * the device, the preconditioner applied through hs_ldiv_dev_*.  A is n x n CSC with 1-based colptr / rowval as Julia holds them (host arrays);
 * b, x: host (where = 0) or device (where = 1) vectors; use_x0 != 0: x holds the initial guess, else zero.  Defaults as in the package for
 * restart <= 0 (min(20, n)), maxiter < 0 (n), reltol < 0 (sqrt(eps)).  Convergence: ||b - A x|| <= max(reltol * ||r0||, abstol).
 * resnorm (may be NULL) receives iters + 1 residual norms (the `log=true` history, resnorm[0] = ||r0||); it must hold maxiter + 1 doubles.
 * (hs_gmres_block.hip: the lockstep driver below on one column, with hs_ldiv_dev_* in place of the block solve.) */
int hs_gmres_d(hs_handle* Pr, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where, int use_x0,
               double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream);
int hs_gmres_z(hs_handle* Pr, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where, int use_x0,
               double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream);

/* The same iteration on an n x nrhs block of right-hand sides in lockstep (hs_gmres_block.hip): nrhs independent GMRES processes share the
 * restart cycle and the Arnoldi index, so a step costs ONE block preconditioner application (hs_ldiv_block_dev_* on the active columns: the
 * factors are read once per chunk of columns), ONE sparse product with a block, batched orthogonalisations and one host synchronisation.
 * This is not block-Krylov: every column keeps its own Krylov space, Hessenberg matrix and stopping test, and column c returns what hs_gmres_*
 * returns for B[:, c] alone -- same defaults, restart limit, tolerance tol_c = max(reltol * ||r0_c||, abstol), breakdown handling -- to the
 * rounding by which hs_ldiv_block_* and hs_ldiv_* differ.  A zero column returns iters = 0, converged, X[:, c] = 0.
 * B, X: column-major blocks (ldb, ldx >= n) on the host (where = 0) or the device (where = 1); X may not alias B.  use_x0 != 0: X holds the
 * initial guesses.  resnorm (may be NULL): (maxiter + 1) x nrhs column-major, column c receives iters[c] + 1 residual norms; iters, converged:
 * nrhs entries.  nrhs = 0 touches nothing.  Pr = NULL runs unpreconditioned.
 * A column that converges, breaks down or reaches maxiter is frozen for the rest of the cycle; at cycle boundaries the columns that go on are
 * compacted, so the block solve runs ceil(nact / chunk) chunks.  Columns are processed in groups of G (a multiple of the block solve's chunk
 * width, chosen per call so that the workspace of (restart + 5) G n elements takes at most half of the free device memory; HS_ERR_NOMEM when
 * not even one chunk fits; HS_GMRES_BLOCK_GROUP in the environment overrides G, read per call).  No atomics, fixed summation orders: two calls
 * return the same bits, and X[:, c], resnorm[:, c], iters[c] do not depend on the values, number or order of the other columns, nor on G.
 * Refused before any device work, X untouched: HS_ERR_UNSUPPORTED for a Pr that hs_ldiv_block_* refuses (HSS interior blocks, more than one
 * rank: hs_gmres_* serves those, one right-hand side at a time); HS_ERR_ARGUMENT for null pointers, X aliasing B, restart above the limit, ldb
 * or ldx < n, where outside 0:1; HS_ERR_DIMENSION for a handle of another size or element type. */
int hs_gmres_block_d(hs_handle* Pr, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb, double* X, int64_t ldx,
                     int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged,
                     void* stream);
int hs_gmres_block_z(hs_handle* Pr, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb, double* X, int64_t ldx,
                     int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged,
                     void* stream);
/* hs_gmres_* / hs_gmres_block_* on op(A) x = b, right-preconditioned by op(Pr): x = x0 + op(Pr)^-1 V y, with op the identity (trans = 0), the
 * transpose (1) or the adjoint (2; = 1 for Float64) -- the solve of adjoint-state and sensitivity computations, with the SAME factorization
 * (compressed or exact) as preconditioner.  The preconditioner goes through hs_ldiv_dev_t_* (single vector) / hs_ldiv_block_dev_t_* (block).
 * Everything else is what hs_gmres_* / hs_gmres_block_* document: defaults, tol_c, breakdown, zero columns, the resnorm layout, use_x0, where,
 * groups, HS_GMRES_BLOCK_GROUP, compaction, freezing; hs_gmres_block_info reports the block calls.
 * colptr, rowval, nzval hold A itself, never op(A).  All three NULL: the handle's own A with the values of the last hs_numeric_begin; this
 * needs Pr != NULL with a completed numeric factorization (else HS_ERR_ARGUMENT) and n == hs_size(Pr) (else HS_ERR_DIMENSION); no host pass
 * over A and no upload happens: trans = 0 reads the CSR map of A that the handle keeps (built on the device at the first use by any call that
 * needs rows of A, see hs_opnorm; its values are gathered from the CSC values per call), trans = 1, 2 read the handle's CSC arrays in place.
 * Some but not all of the three NULL: HS_ERR_ARGUMENT.  trans = 0 with an explicit A goes through hs_gmres_* / hs_gmres_block_* and returns
 * their bits.  For trans = 1, 2 the rows of op(A) are the CSC columns of A: the kernels walk colptr / rowval directly, the adjoint conjugates a
 * value as it is loaded, no transposed or conjugated copy is stored, and with an explicit A the host only rebases the indices (0-based,
 * 32-bit rows).
 * Refused before any device work, x / X untouched: trans outside 0..2: HS_ERR_ARGUMENT; a single-vector call with trans != 0 on a handle
 * hs_ldiv_t_* refuses (fronts that keep D as an HSS matrix; more than one rank): HS_ERR_UNSUPPORTED with its message; a block call on a handle
 * hs_ldiv_block_t_* refuses, whatever trans: HS_ERR_UNSUPPORTED with its message; the handle's own A on a handle over more than one rank:
 * HS_ERR_UNSUPPORTED.  Pr = NULL with an explicit A is not refused: the iteration runs unpreconditioned on op(A).
 * Determinism as hs_gmres_block_*: no floating-point atomics, fixed summation orders (per row of op(A) the stored entries in order), two calls
 * return the same bits, a column does not depend on its neighbours, their number or order, or on G.  An own-A call and an explicit-A call
 * with the same matrix and trans return the same bits, where "the same matrix" means the arrays the handle was given (hs_analyze,
 * hs_numeric_begin): the same entries in the same stored order, no (row, column) stored twice.  trans = 0: a row of the CSR map is in column
 * order, the order of the host conversion, whether the map was built on the device or, for hs_options.mf, on the host with the pattern of the
 * matrix-free fronts; among duplicates of one (row, column) the two orders may differ.  trans = 1, 2: a row of op(A) is a CSC column in its
 * stored order, so an explicit A whose columns are ordered differently from the handle's copy sums in another order. */
int hs_gmres_t_d(hs_handle* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where, int use_x0,
                 double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream);
int hs_gmres_t_z(hs_handle* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where, int use_x0,
                 double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream);
int hs_gmres_block_t_d(hs_handle* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb, double* X,
                       int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters,
                       int* converged, void* stream);
int hs_gmres_block_t_z(hs_handle* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb, double* X,
                       int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters,
                       int* converged, void* stream);
/* hs_gmres_block_t_* on the MODIFIED system: op(A1) X = B with A1 = A + U V^H given as CSC (1-based, as above), right-preconditioned by
 * op(A1)^-1 as hs_mod_ldiv_dev_* applies it from the factors of A (hs_mod_*).  With a compressed (approximate) factorization this is how
 * solutions of the modified system reach a residual tolerance.  colptr / rowval / nzval == NULL is refused (HS_ERR_ARGUMENT): the handle
 * behind Pr holds the unmodified A.  Everything else as hs_gmres_block_t_*; hs_gmres_block_info reports the call. */
int hs_gmres_block_mod_d(hs_mod* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb, double* X,
                         int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters,
                         int* converged, void* stream);
int hs_gmres_block_mod_z(hs_mod* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb, double* X,
                         int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters,
                         int* converged, void* stream);
/* hs_gmres_block_t_* right-preconditioned by a demoted copy of the factorization: op(A) X = B with op(F)^-1 applied by hs_f32_ldiv_dev_*
 * from Float32 factors, the Krylov spaces, residuals and the solution in Float64 / ComplexF64.  A must be given (CSC, 1-based, as above): the
 * object holds no matrix, and colptr / rowval / nzval == NULL is HS_ERR_ARGUMENT.  A size or element type of A and B that is not the
 * object's: HS_ERR_DIMENSION.  Everything else as hs_gmres_block_t_*; hs_gmres_block_info reports the call. */
int hs_gmres_block_f32_d(hs_f32* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb, double* X,
                         int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters,
                         int* converged, void* stream);
int hs_gmres_block_f32_z(hs_f32* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb, double* X,
                         int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters,
                         int* converged, void* stream);
/* the calling thread's last hs_gmres_block_* / hs_gmres_block_t_* call: out8 = {seconds on the device, block preconditioner calls, column-applications summed over
 * those calls, SpMM launches, restart cycles (summed over the groups), column groups, workspace bytes, the largest active-column count} */
int hs_gmres_block_info(double* out8);

int64_t hs_maxrank(const hs_handle* F); /* factornode.jl:49-57: largest of rank(L), rank(R) and the HSS ranks the factorization
                                           holds (hssrank of the interior blocks kept as HSS, hs_options.hss_d); 0 for the dense path */
/* ranks of one front's Gauss transforms (0 = dense); returns 1 if the front is compressed, 0 if not, <0 on error */
int hs_node_ranks(const hs_handle* F, int64_t node, int64_t* rank_L, int64_t* rank_R);
int hs_is_complex(const hs_handle* F);  /* eltype(F) == ComplexF64 */
int64_t hs_size(const hs_handle* F);    /* n */
void hs_free(hs_handle* F);
/* hs_free parks the three big device blocks of a factorization (factor arena, inverse blocks, Schur scratch; blocks >= 256 MiB, at most four)
 * in a process-wide cache, and the next hs_analyze / hs_factor_* of about the same size takes them over: the driver hands out 139 GiB in
 * 1.4 s in a fresh process but needs 4.9 s once memory of that size has been freed before (measured, MI355X / ROCm 7.2).  hs_trim gives the
 * parked blocks and the recycled blocks of the HSS / low-rank modules back to the driver and returns their bytes (call it with nothing in
 * flight; a failing allocation inside the library does it by itself).  HS_ARENA_CACHE=0 in the environment turns the parking off. */
int64_t hs_trim(void);
const char* hs_last_error(void);
int64_t hs_last_error_info(void); /* e.g. node id of a singular front */

/* ---- introspection (metrics the reference lacks) ---- */
typedef struct hs_stats {
  int64_t n, nnodes, nlevels;
  int64_t max_ni, max_nb;
  double flops_factor;   /* sum of F(ni,nb) = 2/3 ni^3 + 2 ni^2 nb + 2 ni nb^2 (x4 for complex), SURVEY.md 8(d) */
  double bytes_factors;  /* device bytes held by the factors */
  double bytes_solve;    /* algorithmic bytes one ldiv! with nrhs=1 must read */
  double t_symbolic, t_upload, t_assemble, t_panel, t_trsm, t_gemm, t_total; /* seconds, device time of last hs_factor */
  double t_solve;        /* seconds, device time of last hs_ldiv */
  double gemm_flops;     /* flops executed by the MFMA GEMM kernel in the last hs_factor */
  int64_t gemm_launches;
  /* every launch of the kernel `gemm_op_kernel` in the last hs_factor (the trailing/Schur updates; the 32-row TRSM base
   * cases run the same tile code as `trsm_inv_kernel`): what a rocprofv3 --stats line of that kernel is compared with */
  double t_mfma_kernel;
  int64_t mfma_kernel_launches;
  double gemm_bytes;     /* algorithmic bytes of those launches: A and B read once, C read and written once ((M*K + K*N + 2*M*N) * sizeof(T)
                            summed over the fronts of every launch) -- what measured HBM traffic is compared with */
} hs_stats;
int hs_get_stats(const hs_handle* F, hs_stats* out);

/* per-node sizes (post-order id): ni, nb, level (root = 1) */
int hs_node_info(const hs_handle* F, int64_t node, int64_t* ni, int64_t* nb, int64_t* level);

/* Export one node's stored blocks to host (column-major, tight leading dimension), for parity tests:
 *   HS_BLK_LU  : ni x ni   packed L\U of the pivoted interior block  (P*Aii = L*U)
 *   HS_BLK_LBI : nb x ni   Abi * U^{-1}
 *   HS_BLK_UIB : ni x nb   L^{-1} * P * Aib
 *   HS_BLK_S   : nb x nb   Schur complement in the node's own bnd order (needs opts.keep_schur)
 *   HS_BLK_DLU : ni x ni   the same packed L\U wherever D has one: also for a matrix-free front (hs_options.mf = 1) whose D was expanded
 *                         and eliminated densely and which exports no other block (what hs_logabsdet reads; with hs_node_export_piv)
 * out must hold rows*cols elements of T (2 doubles per element for complex).
 *   hs_node_export_piv: ni int64 values, 0-based row permutation p with (P*x)[i] = x[p[i]].
 * From these: D = P'LU, L = Lbi*L^{-1}*P, R = U^{-1}*Uib  (FactorNode fields, factornode.jl:7-12).
 * With hs_options.equilibrate these (and the S kept by keep_schur) are blocks of the scaled matrix A_s = 2^er A 2^ec. */
enum { HS_BLK_LU = 0, HS_BLK_LBI = 1, HS_BLK_UIB = 2, HS_BLK_S = 3, HS_BLK_DLU = 4 };
int hs_node_export(const hs_handle* F, int64_t node, int which, double* out);
int hs_node_export_piv(const hs_handle* F, int64_t node, int64_t* out);

/* Library/device identification: fills name (e.g. "gfx950") and returns the CU count, or <0 if no usable device. */
int hs_device_info(char* arch_name, int64_t len, int64_t* cu_count, int64_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* HS_SOLVER_H */
