// hs_solve_multi.h -- the blocked multi-right-hand-side ldiv! (hs_ldiv_block_*): what hs_solve_multi.hip reads from a factorization handle
// and the launch API of kernels_solve_multi.hip.  hs_api.hip owns the handle and checks the arguments; hs_multi_view and the two scratch calls
// of hs_selinv.h are the whole interface between the files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "hs_common.h"

struct hs_handle;

struct HsMultiLR {            // a front whose Gauss transforms are low-rank (compressed front, or mf = 1 with dense D)
  const void* lrL = nullptr;  // LowRank<T>* of Lbi (nb x ni), null: none
  const void* lrR = nullptr;  // LowRank<T>* of Uib (ni x nb)
  long long woff = 0;         // its ni-segment in the work blocks
  int pos = 0;                // its index in the level's SolveNode array
};
struct HsMultiFront {  // host copy of what the flop count and the boundary work block need
  int ni = 0, nb = 0, dense_bnd = 0;
  long long woff = 0;  // its ni-segment in the work blocks
};
struct HsMultiLevel {
  const void* sn = nullptr;  // SolveNode<T>[] of the level's fronts (device)
  int nfronts = 0, maxni = 0, maxnb = 0;
  long long wbase = 0, wrows = 0;  // the level's range of ni-segments: [wbase, wbase + wrows)
  std::vector<HsMultiFront> fronts;
  std::vector<HsMultiLR> lr;
  std::vector<int> node;  // the handle's internal node id of every front, in the order of sn / fronts
  std::vector<int> hss;   // the level's fronts whose interior block D is an HSS matrix (internal node ids): their SolveNode carries ni = 0, so the
                          // grouped dense kernels skip them; HsMultiView::hss_front serves them (hs_ldiv_ulv_* only)
};
struct HsMultiView {
  int64_t n = 0;
  long long wtotal = 0;              // sum of ni over every front
  double sum_fac = 0.0;              // sum over fronts of ni^2 + 2 ni nb
  std::vector<HsMultiLevel> levels;  // index = level (0 = root / pseudo-root)
  void** mx = nullptr;               // cache slot of hs_solve_multi.hip (work blocks, the last call's figures), freed by hs_free through *mx_free
  void (**mx_free)(void*) = nullptr;
  // hs_ldiv_ulv_*: one sweep (0: leaves -> root, 1: root -> leaves) of one HSS front on the kc columns of the caller's column-major block B, which
  // is what carries boundary rows between levels.  Null (every other entry point refuses such handles before it builds a view): no hook.
  void (*hss_front)(void* ctx, int node, int sweep, int trans, void* B, long long ldb, int kc, hipStream_t s) = nullptr;
  void* hss_ctx = nullptr;
};
void hs_multi_view(hs_handle* h, HsMultiView* v);

// Optional active set of the driver below (hs_solve_sparse.hip builds it): which fronts each sweep of each chunk visits.  A level's
// grouped launches then run over a compacted SolveNode / MultiAux array of its active fronts (their woff / boff segments stay where they
// are), maxni / maxnb are taken over the subset, and a level without an active front launches nothing.
struct MultiAux;
struct HsMultiSubset {          // the fronts of one level that one sweep of one chunk visits
  const void* sn = nullptr;     // compacted SolveNode<T>[] (device)
  const MultiAux* aux = nullptr;  // compacted alike (device)
  int maxni = 0, maxnb = 0;
  std::vector<int> pos;         // their indices in the level's arrays, increasing
};
struct HsZeroSeg {  // rows [woff, woff + ni) of work block 2
  long long woff;
  int ni, pad;
};
struct HsMultiActive {
  int nlevels = 0;
  std::vector<HsMultiSubset> sub;    // [(chunk * nlevels + level) * 2 + sweep], sweep 0: forward, 1: backward
  // fronts the backward sweep of a chunk visits and its forward sweep did not: their y is zero, and work block 2 is cleared there before the
  // backward sweep reads it (it holds the x of an earlier chunk or call)
  const HsZeroSeg* zseg = nullptr;   // device
  std::vector<size_t> zoff;          // chunk c owns zseg[zoff[c] .. zoff[c + 1])
  std::vector<int> zmaxni;           // per chunk: the longest of them
  // every chunk lives in the same n x KC block dC: begin(c, kc, s) fills it before the sweeps of chunk c, end(c, kc, s) reads it after them
  void* ctx = nullptr;
  void (*begin)(void* ctx, int chunk, int kc, hipStream_t s) = nullptr;
  void (*end)(void* ctx, int chunk, int kc, hipStream_t s) = nullptr;
  const HsMultiSubset& at(int chunk, int level, int sweep) const { return sub[((size_t)chunk * nlevels + level) * 2 + sweep]; }
};

// C[:, 0:nrhs] = op(F)^-1 C[:, 0:nrhs] in place on the device (ld ldc), chunk by chunk, on stream s; events around the launches.  trans = 0: F
// (kernels_solve_multi.hip), 1: transpose(F), 2: adjoint(F) (kernels_solve_multi_t.hip).  act == nullptr: every front in both sweeps.
// phase (hs_interface.hip; no active set then) runs a part of every chunk's schedule, split at level 0 (the pseudo-root):
//   HS_MULTI_CONDENSE  the forward sweep of levels nlevels-1 .. 1; every front's y is then copied from work block 2 to C[int, :]
//   HS_MULTI_ROOT      both sweeps of level 0
//   HS_MULTI_EXPAND    work block 2 is reloaded from C[int, :] level by level, then the backward sweep of levels 1 .. nlevels-1
// The two copies are exact, so the three in a row leave the bits of HS_MULTI_ALL, which is the schedule without them.
enum { HS_MULTI_ALL = 0, HS_MULTI_CONDENSE, HS_MULTI_ROOT, HS_MULTI_EXPAND };
template <class T>
void hs_solve_multi_run(const HsMultiView& v, int trans, T* dC, int64_t ldc, int64_t nrhs, hipStream_t s, const HsMultiActive* act = nullptr,
                        int phase = HS_MULTI_ALL);
double hs_solve_multi_seconds(void* mx);  // waits for the last block solve and returns its device seconds
void hs_solve_multi_info(void* mx, double* out6);
int hs_ldiv_block_cols();  // KC: columns per chunk (HS_LDIV_BLOCK_COLS = 16 / 32 / 48 / 64, default 32)

// ---- hs_solve_sparse.hip: sparse right-hand sides, selected rows of the solution (hs_ldiv_sparse_*) --------------------------------------
struct HsSparseTree {         // the handle's internal front graph (host); hs_api.hip fills it, also for a plan-only handle
  int64_t n = 0;
  int nuser = 0;              // nodes the C ABI numbers (the user's tree, then the pseudo-root if there is one)
  std::vector<int> parent;    // per internal node (slices of a split front are a chain), -1: none
  std::vector<int> user;      // per internal node: the C ABI's node id
  std::vector<int> ni, nb;    // per internal node
  const int* owner = nullptr; // per row (0-based): the internal node whose int holds it, -1: none
};
void hs_sparse_tree(const hs_handle* h, HsSparseTree* t);
struct HsSparsePlan {
  int KC = 0, nchunks = 0;
  std::vector<int64_t> order;       // processing order of the columns (0-based ids)
  std::vector<unsigned char> act;   // [chunk * nnodes + internal node]: bit 0 forward, bit 1 backward
  double visits[2] = {0, 0};        // front visits, forward / backward
  double model = 0.0;               // sum over chunks and sweeps of ni^2 / 2 + ni nb over the visited fronts (elements)
};
// 0-based or 1-based indices (base); rows == nullptr: every row is wanted
void hs_sparse_plan(const HsSparseTree& t, int64_t nrhs, const int64_t* bcolptr, const int64_t* browval, int64_t base, const int64_t* rows, int64_t nrows,
                    HsSparsePlan* p);
// X[r, j] = (op(F)^-1 B)[rows[r], j]: bval / dX on the device (X column-major, ld ldx), the index arrays on the host (1-based).  Waits for s.
// out8: the figures of hs_ldiv_sparse_info but the seconds and the values moved
template <class T>
void hs_solve_sparse_run(const HsMultiView& v, const HsSparseTree& t, int trans, int64_t nrhs, const int64_t* bcolptr, const int64_t* browval, const T* d_bval,
                         const int64_t* rows, int64_t nrows, T* dX, int64_t ldx, hipStream_t s, double* out8);

// ---- kernels_solve_sparse.hip ------------------------------------------------------------------------------------------------------------
// W[row[e], col[e]] = val[src[e]] for the cnt entries of a chunk (W: n x kc column-major, ld ldw, zero before)
template <class T>
void launch_sparse_scatter(T* W, long long ldw, const T* val, const int* row, const int* col, const long long* src, long long cnt, hipStream_t s);
// X[r, xcol[c]] = W[rows[r], c] for r < nrows, c < kc (X: ld ldx; rows == nullptr: row r itself)
template <class T>
void launch_sparse_gather(T* X, long long ldx, const long long* xcol, const T* W, long long ldw, const int* rows, long long nrows, int kc, hipStream_t s);
// dst[e] = src[idx[e]] for whole SolveNode<T> entries (src: base of the handle's array, idx: element offsets from it)
template <class T>
void launch_sparse_compact(SolveNode<T>* dst, const SolveNode<T>* src, const long long* idx, long long cnt, hipStream_t s);
// rows [woff, woff + ni) x kc of the row-major work block W2 (pitch kcw) = 0 for every segment, one launch
template <class T>
void launch_sparse_zero(T* W2, int kcw, int kc, const HsZeroSeg* seg, int nseg, int maxni, hipStream_t s);

// ---- the factor scalar --------------------------------------------------------------------------------------------------------------------
// T is the element type of the work blocks (double, cplx); S that of the stored factor panels: T itself (the handle's own factors) or
// F32Of<T>::type (a copy demoted to Float32 storage, hs_f32.h).  A SolveNode<S> and a LowRank<S> have the layout of their <T> forms
// (pointers and integers only).  Every problem struct, kernel and launch below is written once over the pair; kernels_solve_multi.hip and
// kernels_solve_multi_t.hip instantiate S = T, kernels_solve_multi_f32.hip S = F32Of<T>::type.
struct cplxf {
  float re, im;
};
template <class T>
struct F32Of;
template <>
struct F32Of<double> {
  typedef float type;
};
template <>
struct F32Of<cplx> {
  typedef cplxf type;
};
static_assert(sizeof(SolveNode<float>) == sizeof(SolveNode<double>) && sizeof(SolveNode<cplxf>) == sizeof(SolveNode<cplx>), "SolveNode<S> has the layout of SolveNode<T>");

// ---- kernels_solve_multi.hip ----------------------------------------------------------------------------------------------------------
// One tall-skinny product  D = A X  or  D = Cin - A X  with A (M x K, column-major, a stored factor panel) read once and fed to
// v_mfma_f64_16x16x4_f64 from registers.  X (K x kc, kc <= 64), Cin and D are rows of row-major work blocks (one pitch for all columns).
template <class T, class S = T>
struct MultiProb {
  const S* A;
  int lda, M, K;
  int trap;  // 1: A is the unit lower trapezoid of what is stored (LowRank::Lp); 2 (the products of hs_mul_* only): its upper triangle, diagonal included
  const T* X;
  long long xrs;    // X(k, c) = X[k * xrs + c]
  const T* Cin;     // null: D = A X; else D = Cin - A X, addressed like C
  T* C;
  long long crs;    // D(i, c) -> C[(cmap ? cmap[i] : i) * crs + c]
  const int* cmap;
};
enum {
  HSM_DIAG_L = 0,  // Y_j = inv256L_j W_j                         (W: work block 1, Y: work block 2)
  HSM_BELOW_L,     // W[rows below block j] -= L[below, j] Y_j    (interior rows)
  HSM_BND_L,       // Xb -= Lbi Y                                 (Xb: the gathered boundary rows B[bnd, :])
  HSM_UR,          // W = Y - Uib Xb
  HSM_DIAG_U,      // X_j = inv256U_j W_j                         (X overwrites Y)
  HSM_ABOVE_U,     // W[rows above block j] -= U[above, j] X_j
};
struct MultiAux {   // per front, in the order of the level's SolveNode array (the driver builds and uploads it once per handle)
  long long boff;   // its nb-segment in the boundary work block
  int nb, pad;      // boundary size (the SolveNode of a matrix-free front carries 0)
};
struct MultiArgs {  // what the grouped kernels need besides the level's SolveNode array
  void* W1;         // work block of the level: (wrows x kcw), row-major, segment of a front at woff - wbase
  void* W2;         // y / x of every front: (wtotal x kcw), row-major, segment at woff
  void* XB;         // boundary rows of the level's fronts: (sum of nb x kcw), row-major, segment at boff
  const MultiAux* aux;
  long long wbase;
  int kcw;          // row pitch of the work blocks
  void* B;          // the caller's block (column-major)
  long long ldb;
  int kc;           // columns of this chunk
};
__host__ __device__ constexpr int hs_multi_rows_per_wg_c(bool is_complex) { return is_complex ? 32 : 64; }  // 4 waves split K over these rows
int hs_multi_rows_per_wg(bool is_complex);
template <class T, class S>
void launch_multi_level(const SolveNode<S>* sn, int nfronts, int mode, int blk, int maxM, const MultiArgs& a, hipStream_t s);
template <class T, class S>
void launch_multi_prob(const MultiProb<T, S>& p, int kc, hipStream_t s);
// The caller's column-major block <-> the row-major work blocks, for every front of a level:
//   what = 0: W1 = B[int, :]   1: Xb = B[bnd, :]   2: B[int, :] = W2   3: B[bnd, :] = Xb
// perm_what names the one interior move that goes through the front's row permutation (B[int[rperm[i]], :] <-> row i of the work block):
// 0 for the forward solve (W1 = (P B)[int, :]), 2 for the transposed / adjoint one (B[int, :] = P^T W2); no other value is served.
// One kernel per T whatever S is: it reads ni, woff, rperm and fidx of a descriptor, which SolveNode<S> holds where SolveNode<T> does.
template <class T, class S>
void launch_multi_move(const SolveNode<S>* sn, int nfronts, int what, int maxrows, const MultiArgs& a, hipStream_t s, int perm_what);

// ---- kernels_solve_multi_t.hip --------------------------------------------------------------------------------------------------------
// The product of the transposed / adjoint block solve:  D = op(A)^T X  or  D = Cin - op(A)^T X  with A stored K x M column-major (the
// reduction index is the contiguous one), op = identity or conj; X, Cin and D as above.
template <class T, class S = T>
struct MultiProbT {
  const S* A;
  int lda, M, K;    // M outputs = columns of A, K = rows of A
  int trap;         // 1: A is the unit lower trapezoid of what is stored (LowRank::Lp, K x M); 2 (hs_mul_* only): its upper triangle with the diagonal
  int conj;         // 1: op = conj (ComplexF64)
  const T* X;
  long long xrs;    // X(k, c) = X[(xmap ? xmap[k] : k) * xrs + c]
  const int* xmap;
  const T* Cin;     // null: D = op(A)^T X; else D = Cin - op(A)^T X, addressed like C
  T* C;
  long long crs;    // D(i, c) -> C[(cmap ? cmap[i] : i) * crs + c]
  const int* cmap;
};
enum {
  HSMT_DIAG_U = 0,  // Z_j = op(inv256U_j)^T W_j                          (W: work block 1, Z: work block 2)
  HSMT_BELOW_U,     // W[below j] -= op(U11[j, below])^T Z_j              (right-looking)
  HSMT_LEFT_U,      // W_j -= op(U11[above j, j])^T Z[above j]            (left-looking)
  HSMT_BND_U,       // Xb -= op(Uib)^T Z
  HSMT_LB,          // W = Z - op(Lbi)^T Xb
  HSMT_DIAG_L,      // X_j = op(inv256L_j)^T W_j                          (X overwrites Z)
  HSMT_ABOVE_L,     // W[above j] -= op(L11[j, above])^T X_j              (right-looking)
  HSMT_LEFT_L,      // W_j -= op(L11[below j, j])^T X[below j]            (left-looking)
};
template <class T, class S>
void launch_multi_level_t(const SolveNode<S>* sn, int nfronts, int mode, int blk, int conj, int maxM, const MultiArgs& a, hipStream_t s);
template <class T, class S>
void launch_multi_prob_t(const MultiProbT<T, S>& p, int kc, hipStream_t s);

// ---- kernels_solve_multi_mul.hip: the products of hs_mul_* (C = op(F) B, hs_mul_run) ----------------------------------------------------------
// The same tile body, sides and lane maps with what the product with F needs and the solves do not (a template argument of the sides, so the
// kernels of the solves keep their code): trap = 2; a triangular operand is read between the 16-column chunks that meet the workgroup's rows and
// nowhere else; the sign of the product is a field of its own (minus), so D = Cin + A X exists beside Cin - A X and A X; and one product may
// write (forward: C2) or read (transposed: X2) two work blocks, split at a row: the trapezoid [L11; Lbi] is ONE panel of LF.
template <class T, class S = T>
struct MultiProbMul : MultiProb<T, S> {
  int minus;   // 1: the product is subtracted (D = Cin - A X); 0: added to Cin, or stored when there is none
  int split;   // with C2: rows >= split of D are C2[(row - split) * crs + c] += (cmap does not reach them); rows below it go through C / Cin
  T* C2;       // null: no second block
};
template <class T, class S = T>
struct MultiProbMulT : MultiProbT<T, S> {
  int minus;
  int split;     // with X2: X(k, c) for k >= split is X2[(k - split) * xrs + c] (xmap does not reach them)
  const T* X2;   // null: no second block
};
enum {
  HSMM_TRIU = 0,  // Y = triu(LF[0:ni, 0:ni]) W                              (W: work block 1, Y: work block 2)
  HSMM_UR,        // Y += Uib Xb
  HSMM_TRAP,      // [W; Xb +=] = unit-trapezoid(LF[0:mrows, 0:ni]) Y        (rows < ni -> W, rows >= ni are added into Xb)
};
enum {
  HSMMT_TRAP = 0,  // Z = op(unit-trapezoid(LF[0:mrows, 0:ni]))^T [W; Xb]    (W: work block 1, Z: work block 2)
  HSMMT_TRIU,      // W = op(triu(LF[0:ni, 0:ni]))^T Z
  HSMMT_BND_U,     // Xb += op(Uib)^T Z
};
template <class T>
void launch_mul_level(const SolveNode<T>* sn, int nfronts, int mode, int maxM, const MultiArgs& a, hipStream_t s);
template <class T>
void launch_mul_prob(const MultiProbMul<T, T>& p, int kc, hipStream_t s);
template <class T>
void launch_mul_level_t(const SolveNode<T>* sn, int nfronts, int mode, int conj, int maxM, const MultiArgs& a, hipStream_t s);
template <class T>
void launch_mul_prob_t(const MultiProbMulT<T, T>& p, int kc, hipStream_t s);

// C[:, 0:nrhs] = op(F) C[:, 0:nrhs] in place on the device (ld ldc), in chunks of hs_ldiv_block_cols() columns on the work blocks of the block
// solve, on stream s (the schedule: hs_solve_multi.hip).  Its figures are hs_mul_figures', never the handle's last block solve.
template <class T>
void hs_mul_run(const HsMultiView& v, int trans, T* dC, int64_t ldc, int64_t nrhs, hipStream_t s);
// seconds (waits for the product), factor bytes read, executed flops, useful flops, chunks, work-block bytes of the last hs_mul_run
void hs_mul_figures(void* mx, double* out6);
