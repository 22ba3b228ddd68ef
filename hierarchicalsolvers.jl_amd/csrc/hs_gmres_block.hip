// hs_gmres_block.hip -- right-preconditioned restarted GMRES behind the C ABI (include/hs_solver.h), every vector on the device: one
// right-hand side (hs_gmres_*, hs_gmres_t_*) or a block of them in lockstep (hs_gmres_block_*), on one driver.
//
// Reference scenario (test/rungmres.jl:47-48):  x, ch = gmres(A, b; Pr=F, reltol=1e-9, restart=30, log=true, maxiter=30)
// IterativeSolvers.jl (0.9.0) is not part of the reference tree: the algorithm is the textbook one (Saad & Schultz 1986; Arnoldi with
// classical Gram-Schmidt + one re-orthogonalisation pass, Givens rotations on the Hessenberg matrix, right preconditioning
// x = x0 + Pr^-1 V y) and matches the Python mirror tests/gmres_mirror.py step for step (same iteration counts).
// PARITY UNPINNED against the Julia package.
//
// nrhs independent Arnoldi processes advance together: every column keeps its own Krylov space, Hessenberg matrix, rotations and stopping
// test, but a step applies the preconditioner to all active columns with ONE hs_ldiv_block_dev_* call (the factors are read
// once per 32 columns, not once per column), multiplies by A with ONE CSR SpMM, runs the orthogonalisations as batched kernels (column =
// blockIdx.y; all HBM-bound n-vector kernels, the Hessenberg / Givens recurrences and the triangular solve one thread per column on
// device-resident H, c, s, g) and reads 2 nact doubles (||w|| and the residual estimate per column) to the host with one synchronisation:
// a preconditioner application costs three orders of magnitude more than that read, and an iteration that is not needed costs a whole
// `ldiv!`.  This is not block-Krylov.  hs_gmres_* is the same driver on one column in a group of width 1, with the single-right-hand-side
// solve hs_ldiv_dev_* as the preconditioner call (which also serves the handles the block solve refuses): a column of a block returns what
// hs_gmres_* returns for it alone, to the rounding by which hs_ldiv_block_* and hs_ldiv_* differ, and the same bits without a preconditioner.
//
// Layout: every n x nact object is a column-major block with leading dimension ldv (n rounded up to an even value); the basis is
// V[(j G + c) ldv + i] (G: group width), so V_j is directly the dB argument of hs_ldiv_block_dev_*.  A column that converges, breaks down or
// exhausts maxiter is frozen for the rest of the restart cycle by a device-resident mask (its state is no longer written); at cycle boundaries
// the columns that go on are gathered into the leading columns ("slots") of the residual block, so the block solve runs ceil(nact / 32) chunks.
// X and B are never repacked: the kernels that touch them take a slot -> column map.
//
// Determinism: no atomics, every reduction in a fixed order that depends on the row index alone, so a column's results do not depend on its
// slot, on the other columns, on G or on compaction.
//
// hs_gmres_t_* / hs_gmres_block_t_* run the same schedule on op(A) X = B right-preconditioned by op(Pr): gmres_group is a template on the
// operator (the CSR SpMM below, or the SpMM over "entry ranges as rows" of hs_gmres_common.h) and on the preconditioner call (hs_ldiv_dev_* /
// hs_ldiv_dev_t_* for one column, hs_ldiv_block_dev_* / hs_ldiv_block_dev_t_* for a block); A is passed as host CSC arrays or is the
// handle's own (hs_gmres_op.h).  hs_gmres_block_mod_* is one more pair of
// instantiations: op(A1) X = B with A1 = A + U V^H as host CSC arrays, the preconditioner call hs_mod_ldiv_dev_* (hs_mod.hip).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hs_kernels.h"
#include "hs_host.h"
#include "hs_block_apply.h"
#include "hs_gmres_common.h"
#include "hs_solve_multi.h"
#include "hs_mod.h"  // hs_mod_apply_prec, hs_mod_handle
#include "hs_f32.h"  // hs_f32_apply_prec, hs_f32_size, hs_f32_is_complex

namespace {

// Y[:, c] = A X[:, xmap[c]]   or, with B,   Y[:, c] = B[:, bmap[c]] - A X[:, xmap[c]]   (CSR, 0-based; null map: identity), c < nc.
// A workgroup owns 256 rows and walks the columns CB at a time, lanes along rows: X[:, c] and Y[:, c] are read and written contiguously, and
// rowptr / colind / val of the row tile are read once per chunk of CB columns, not once per column (the chunks after the first follow it in
// the same workgroup and should find them in L2; that is not measured).  Per (row, column) the sum runs over e in
// stored order with Scal<T>::fma; with one column (hs_gmres_*) this is the one-thread-per-row product.
// The kernel is spmm_op_kernel<T, CB, false> (hs_gmres_common.h): a CSR is the plain case of its "entry ranges as rows".
template <class T>
void launch_spmm(const int64_t* rowptr, const int32_t* colind, const T* val, const T* X, int64_t ldx, const int64_t* xmap, T* Y, int64_t ldy, const T* B, int64_t ldb,
                 const int64_t* bmap, int64_t n, int nc, hipStream_t s) {
  constexpr int CB = sizeof(T) == 16 ? 4 : 8;
  hipLaunchKernelGGL((spmm_op_kernel<T, CB, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rowptr, colind, val, X, ldx, xmap, Y, ldy, B, ldb, bmap, n, nc);
}

// The kernels of the iteration: the column (slot) is blockIdx.y, a frozen column (mask[c] == 0) is skipped.
// part[(c nblk + blockIdx.x) k1 + j] = sum over the block's 1024 rows of conj(V_j[i, c]) W[i, c],  j = 0..k;  w stays in registers
template <class T>
__global__ __launch_bounds__(256) void bdot_kernel(const T* __restrict__ V, int64_t ldv, int64_t jstride, int k1, const T* __restrict__ W, T* __restrict__ part, int64_t n,
                                                   const int* __restrict__ mask) {
  __shared__ T sh[256];
  const int c = blockIdx.y;
  if (!mask[c]) return;
  const T* Vc = V + (size_t)c * ldv;
  const T* w = W + (size_t)c * ldv;
  T* pc = part + ((size_t)c * gridDim.x + blockIdx.x) * k1;
  const int64_t i0 = (int64_t)blockIdx.x * 1024;
  T wv[4];
  for (int t = 0; t < 4; ++t) {
    const int64_t i = i0 + t * 256 + threadIdx.x;
    wv[t] = i < n ? w[i] : Scal<T>::zero();
  }
  for (int j = 0; j < k1; ++j) {
    T acc = Scal<T>::zero();
    for (int t = 0; t < 4; ++t) {
      const int64_t i = i0 + t * 256 + threadIdx.x;
      if (i < n) acc = Scal<T>::fma(conj_(Vc[(size_t)j * jstride + i]), wv[t], acc);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) pc[j] = sh[0];
    __syncthreads();
  }
}
// h[c hs + j] = sum over blocks of part[(c nblk + b) k1 + j], hacc += the same   (one workgroup per column; fixed order)
template <class T>
__global__ __launch_bounds__(256) void breduce_kernel(const T* __restrict__ part, int nblk, int k1, T* __restrict__ h, T* __restrict__ hacc, int hs, const int* __restrict__ mask) {
  __shared__ T sh[256];
  const int c = blockIdx.x;
  if (!mask[c]) return;
  const T* pc = part + (size_t)c * nblk * k1;
  for (int j = 0; j < k1; ++j) {
    T acc = Scal<T>::zero();
    for (int b = threadIdx.x; b < nblk; b += 256) acc = acc + pc[(size_t)b * k1 + j];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      h[(size_t)c * hs + j] = sh[0];
      if (hacc) hacc[(size_t)c * hs + j] = hacc[(size_t)c * hs + j] + sh[0];
    }
    __syncthreads();
  }
}
// W[i, c] -= sum_j h[c hs + j] V_j[i, c]
template <class T>
__global__ __launch_bounds__(256) void baxpy_kernel(const T* __restrict__ V, int64_t ldv, int64_t jstride, int k1, const T* __restrict__ h, int hs, T* __restrict__ W, int64_t n,
                                                    const int* __restrict__ mask) {
  __shared__ T sh[GM_MAXK + 1];
  const int c = blockIdx.y;
  if (!mask[c]) return;
  if ((int)threadIdx.x < k1) sh[threadIdx.x] = h[(size_t)c * hs + threadIdx.x];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const T* Vc = V + (size_t)c * ldv;
  T acc = W[(size_t)c * ldv + i];
  for (int j = 0; j < k1; ++j) acc = Scal<T>::fnma(sh[j], Vc[(size_t)j * jstride + i], acc);
  W[(size_t)c * ldv + i] = acc;
}
// cycle end: out[:, c] = x[:, c] + sum_{j < kused[c]} y[c ys + j] V_j[:, c], every column with its own kused.  x null: out = V y (slot
// order, ld ldo); else x = out = the caller's X through the slot -> column map (the unpreconditioned update)
template <class T>
__global__ __launch_bounds__(256) void bcombine_kernel(const T* __restrict__ V, int64_t ldv, int64_t jstride, const T* __restrict__ y, int ys, const int* __restrict__ kused,
                                                       T* __restrict__ X, int64_t ldx, const int64_t* __restrict__ xmap, T* __restrict__ out, int64_t ldo, int64_t n) {
  __shared__ T sh[GM_MAXK + 1];
  const int c = blockIdx.y;
  const int k = kused[c];
  if ((int)threadIdx.x < k) sh[threadIdx.x] = y[(size_t)c * ys + threadIdx.x];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  T* dst = X ? X + (size_t)xmap[c] * ldx : out + (size_t)c * ldo;
  const T* Vc = V + (size_t)c * ldv;
  T acc = X ? dst[i] : Scal<T>::zero();
  for (int j = 0; j < k; ++j) acc = Scal<T>::fma(sh[j], Vc[(size_t)j * jstride + i], acc);
  dst[i] = acc;
}
// X[:, xmap[c]] += Z[:, c]   (the preconditioned update, as one fma with 1)
template <class T>
__global__ __launch_bounds__(256) void badd_kernel(const T* __restrict__ Z, int64_t ldz, T* __restrict__ X, int64_t ldx, const int64_t* __restrict__ xmap, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  T* x = X + (size_t)xmap[blockIdx.y] * ldx;
  x[i] = Scal<T>::fma(Scal<T>::one(), Z[(size_t)blockIdx.y * ldz + i], x[i]);
}
template <class T>
__global__ __launch_bounds__(256) void bnorm2_part_kernel(const T* __restrict__ W, int64_t ldw, double* __restrict__ part, int64_t n, const int* __restrict__ mask) {
  __shared__ double sh[256];
  const int c = blockIdx.y;
  if (mask && !mask[c]) return;
  const T* w = W + (size_t)c * ldw;
  double acc = 0.0;
  for (int t = 0; t < 4; ++t) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + t * 256 + threadIdx.x;
    if (i < n) acc += abs2_(w[i]);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)c * gridDim.x + blockIdx.x] = sh[0];
}
// out[c ostride] = sqrt(sum of the column's partial sums)
__global__ __launch_bounds__(256) void bnorm2_final_kernel(const double* __restrict__ part, int nblk, double* __restrict__ out, int ostride, const int* __restrict__ mask) {
  __shared__ double sh[256];
  const int c = blockIdx.x;
  if (mask && !mask[c]) return;
  double acc = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) acc += part[(size_t)c * nblk + b];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(size_t)c * ostride] = sqrt(sh[0]);
}
// V[i, c] = W[i, c] / nrm[c nstride]  (a zero norm copies: breakdown is handled through the residual estimate)
template <class T>
__global__ __launch_bounds__(256) void bscale_into_kernel(const T* __restrict__ W, int64_t ldw, const double* __restrict__ nrm, int nstride, T* __restrict__ V, int64_t ldv,
                                                          int64_t n, const int* __restrict__ mask) {
  const int c = blockIdx.y;
  if (mask && !mask[c]) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double a = nrm[(size_t)c * nstride];
  const T w = W[(size_t)c * ldw + i];
  V[(size_t)c * ldv + i] = a > 0.0 ? scale_(w, 1.0 / a) : w;
}
// cycle boundary: Rn[:, c] = R[:, src[c]]
template <class T>
__global__ __launch_bounds__(256) void bgather_kernel(const T* __restrict__ R, T* __restrict__ Rn, int64_t ld, const int* __restrict__ src, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Rn[(size_t)blockIdx.y * ld + i] = R[(size_t)src[blockIdx.y] * ld + i];
}

// Device-resident small state of the slots in one restart cycle, slot c at c times the stride: H ((m+1) x m, ld m+1), cs, sn, g, the new
// column h (and h2 of the second pass), y; {||w||, |g[k+1]|} adjacent in hnres; what decides freezing (tol, itleft) and its result (mask, kused)
template <class T>
struct GbSmall {
  T *H, *cs, *sn, *g, *h, *h2, *y;
  double* hnres;  // 2 per slot
  double* beta;   // ||r|| at the start of the cycle
  double* tol;
  int* itleft;    // iterations the column may still take
  int* mask;      // 1: the column advances in this cycle
  int* kused;
  int64_t* col;   // slot -> column of the caller's B / X
  int ld, sH, s1, s2;  // strides: H, (m+1)-arrays, (m+2)-arrays
};
// one thread per slot: applies the previous rotations to column k of the slot's H, creates the one that annihilates H[k+1, k] and updates g,
// then takes the freezing decision the host repeats from the same two doubles
template <class T>
__global__ __launch_bounds__(64) void bgivens_kernel(GbSmall<T> S, int k, int nact) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= nact || !S.mask[c]) return;
  T* Hc = S.H + (size_t)c * S.sH + (size_t)k * S.ld;
  const T* h = S.h + (size_t)c * S.s2;
  T* cs = S.cs + (size_t)c * S.s1;
  T* sn = S.sn + (size_t)c * S.s1;
  T* g = S.g + (size_t)c * S.s2;
  const double hn = S.hnres[2 * c];
  for (int i = 0; i <= k; ++i) Hc[i] = h[i];
  T hk1 = Scal<T>::zero();
  *((double*)&hk1) = hn;  // real part = ||w||
  Hc[k + 1] = hk1;
  for (int i = 0; i < k; ++i) {
    const T t = cs[i] * Hc[i] + sn[i] * Hc[i + 1];
    Hc[i + 1] = Scal<T>::zero() - conj_(sn[i]) * Hc[i] + cs[i] * Hc[i + 1];
    Hc[i] = t;
  }
  const T a = Hc[k], b = Hc[k + 1];
  const double aa = absT(a), den = sqrt(aa * aa + absT(b) * absT(b));
  T cc = Scal<T>::one(), s = Scal<T>::zero();
  if (den != 0.0) {
    cc = Scal<T>::zero();
    *((double*)&cc) = aa / den;
    const T ph = aa > 0.0 ? scale_(a, 1.0 / aa) : Scal<T>::one();
    s = scale_(ph * conj_(b), 1.0 / den);
  }
  cs[k] = cc;
  sn[k] = s;
  Hc[k] = cc * a + s * b;
  Hc[k + 1] = Scal<T>::zero();
  g[k + 1] = Scal<T>::zero() - conj_(s) * g[k];
  g[k] = cc * g[k];
  const double res = absT(g[k + 1]);
  S.hnres[2 * c + 1] = res;
  S.kused[c] = k + 1;
  const int left = S.itleft[c] - 1;
  S.itleft[c] = left;
  if (res <= S.tol[c] || hn == 0.0 || left <= 0) S.mask[c] = 0;
}
// y = triu(H[:k, :k]) \ g[:k] with the slot's own k = kused[c]
template <class T>
__global__ __launch_bounds__(64) void bhess_solve_kernel(GbSmall<T> S, int nact) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= nact) return;
  const int k = S.kused[c];
  const T* H = S.H + (size_t)c * S.sH;
  const T* g = S.g + (size_t)c * S.s2;
  T* y = S.y + (size_t)c * S.s1;
  for (int i = k - 1; i >= 0; --i) {
    T acc = g[i];
    for (int j = i + 1; j < k; ++j) acc = Scal<T>::fnma(H[(size_t)i + (size_t)j * S.ld], y[j], acc);
    y[i] = acc / H[(size_t)i + (size_t)i * S.ld];
  }
}
template <class T>
__global__ __launch_bounds__(64) void breset_kernel(GbSmall<T> S, int m, int nact) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= nact) return;
  T* g = S.g + (size_t)c * S.s2;
  for (int i = 0; i <= m; ++i) g[i] = Scal<T>::zero();
  T b = Scal<T>::zero();
  *((double*)&b) = S.beta[c];
  g[0] = b;
  S.kused[c] = 0;
  S.mask[c] = 1;
}

// What gmres_group is instantiated on.  The operator: Y[:, c] = A X[:, xmap[c]], or B[:, bmap[c]] - A X[:, xmap[c]] with B.  The
// preconditioner: out = Pr^-1 in on an n x nc block; F == nullptr: none.
template <class T>
struct CsrSpmm {  // hs_gmres_block_*: the CSR upload of A
  const int64_t* rowptr;
  const int32_t* colind;
  const T* val;
  void operator()(const T* X, int64_t ldx, const int64_t* xmap, T* Y, int64_t ldy, const T* B, int64_t ldb, const int64_t* bmap, int64_t n, int nc, hipStream_t s) const {
    launch_spmm<T>(rowptr, colind, val, X, ldx, xmap, Y, ldy, B, ldb, bmap, n, nc, s);
  }
};
template <class T>
struct RowsSpmm {  // hs_gmres_block_t_*: op(A) over entry ranges
  RowsOf<T> A;
  void operator()(const T* X, int64_t ldx, const int64_t* xmap, T* Y, int64_t ldy, const T* B, int64_t ldb, const int64_t* bmap, int64_t n, int nc, hipStream_t s) const {
    launch_spmm_op<T>(A, X, ldx, xmap, Y, ldy, B, ldb, bmap, n, nc, s);
  }
};
template <class T>
struct PrecBlockFwd {  // hs_ldiv_block_dev_*
  hs_handle* F;
  int operator()(T* out, const T* in, int64_t ld, int64_t n, int64_t nc, hipStream_t s) const { return hs_block_apply_dev<T>(F, HS_VIA_BLOCK, 0, out, ld, in, ld, n, nc, s); }
};
template <class T>
struct PrecBlockMod {  // hs_mod_ldiv_dev_*: op(A + U V^H)^-1 through the factors of A
  hs_handle* F;       // the handle the modification was built on: what gmres_group reads as Pr.F (non-null: there is a preconditioner)
  hs_mod* M;
  int trans;
  int operator()(T* out, const T* in, int64_t ld, int64_t n, int64_t nc, hipStream_t s) const { return hs_mod_apply_prec(M, trans, out, ld, in, ld, n, nc, s); }
};
template <class T>
struct PrecBlockF32 {  // hs_f32_ldiv_dev_*: op(F)^-1 from the Float32 copy of the factors
  hs_handle* F;        // never dereferenced: the object itself, which gmres_group reads as "there is a preconditioner"
  hs_f32* G;
  int trans;
  int operator()(T* out, const T* in, int64_t ld, int64_t n, int64_t nc, hipStream_t s) const { return hs_f32_apply_prec(G, trans, out, ld, in, ld, n, nc, s); }
};
template <class T>
struct PrecBlockOp {  // hs_ldiv_block_dev_t_*: op(F)
  hs_handle* F;
  int trans;
  int operator()(T* out, const T* in, int64_t ld, int64_t n, int64_t nc, hipStream_t s) const { return hs_block_apply_dev<T>(F, HS_VIA_BLOCK_T, trans, out, ld, in, ld, n, nc, s); }
};

// hs_gmres_* / hs_gmres_t_*: the single-right-hand-side solves, which also serve the handles the block solve refuses (their columns are
// solved one after the other: a group of width 1 hands them one)
template <class T>
struct PrecFwd {  // hs_ldiv_dev_*
  hs_handle* F;
  int operator()(T* out, const T* in, int64_t ld, int64_t n, int64_t nc, hipStream_t s) const {
    return hs_block_apply_dev<T>(F, HS_VIA_COLS, 0, out, ld, in, ld, n, nc, s);
  }
};
template <class T>
struct PrecOp {  // hs_ldiv_dev_t_*: op(F)
  hs_handle* F;
  int trans;
  int operator()(T* out, const T* in, int64_t ld, int64_t n, int64_t nc, hipStream_t s) const {
    return hs_block_apply_dev<T>(F, HS_VIA_COLS_T, trans, out, ld, in, ld, n, nc, s);
  }
};

// figures of the calling thread's last hs_gmres_block_* call (hs_gmres_block_info); a run counts into the array its caller gives it
enum { GI_SECONDS = 0, GI_PREC_CALLS, GI_COL_APPS, GI_SPMM, GI_CYCLES, GI_GROUPS, GI_WORK_BYTES, GI_MAX_ACTIVE };
thread_local double g_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};

struct Column {  // host side of one right-hand side
  int64_t col = 0;
  double beta = 0.0, tol = 0.0;
  int64_t it = 0;
  bool conv = false, frozen = false;
  std::vector<double> hist;
};

template <class T>
struct Workspace {
  int64_t ldv = 0, G = 0;
  int m = 0, nblk = 0;
  T *V = nullptr, *W = nullptr, *Z = nullptr, *R = nullptr, *R2 = nullptr, *part = nullptr;
  double *dpart = nullptr;
  int* src = nullptr;
  GbSmall<T> S;
};
template <class T>
size_t bytes_per_column(int64_t n, int m) {
  const size_t ldv = (size_t)(n + 1) / 2 * 2, nblk = (size_t)(n + 1023) / 1024;
  return ((size_t)(m + 5) * ldv + nblk * (m + 2) + (size_t)(m + 1) * m + 3 * (size_t)(m + 1) + 3 * (size_t)(m + 2)) * sizeof(T) + (nblk + 4) * sizeof(double) +
         4 * sizeof(int) + sizeof(int64_t);
}

// one group of gc <= G columns (g0 .. g0 + gc of the caller's B and X, device pointers) from start to finish
template <class T, class Op, class Prec>
void gmres_group(const Op& A, const Prec& Pr, int64_t n, const T* B, int64_t ldb, T* X, int64_t ldx, int64_t g0, int gc, int use_x0, double reltol, double abstol,
                 int64_t maxiter, Workspace<T>& ws, Column* cols, double* info, hipStream_t s) {
  hs_handle* const F = Pr.F;
  const int m = ws.m, nblk = ws.nblk;
  const int64_t ldv = ws.ldv, jstride = ws.G * ldv;
  GbSmall<T>& S = ws.S;
  const unsigned gn = (unsigned)((n + 255) / 256);
  std::vector<double> hd((size_t)2 * gc);
  std::vector<int64_t> hcol((size_t)gc);
  std::vector<double> hbeta((size_t)gc), htol((size_t)gc);
  std::vector<int> hleft((size_t)gc), hsrc((size_t)gc);
  auto read = [&](const double* d, int cnt) {
    HS_HIP(hipMemcpyAsync(hd.data(), d, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, s));
    HS_HIP(hipStreamSynchronize(s));
  };
  auto norms = [&](const T* Wb, double* out, int ostride, int nc, const int* mask) {
    hipLaunchKernelGGL(bnorm2_part_kernel<T>, dim3(nblk, nc), dim3(256), 0, s, Wb, ldv, ws.dpart, n, mask);
    hipLaunchKernelGGL(bnorm2_final_kernel, dim3(nc), dim3(256), 0, s, (const double*)ws.dpart, nblk, out, ostride, mask);
  };
  auto residual = [&](int nc) {  // R[:, c] = B[:, col[c]] - A X[:, col[c]]
    A((const T*)X, ldx, (const int64_t*)S.col, ws.R, ldv, B, ldb, (const int64_t*)S.col, n, nc, s);
    info[GI_SPMM] += 1;
  };
  // r0 = b - A x0, slots in the order of the columns
  for (int c = 0; c < gc; ++c) hcol[(size_t)c] = g0 + c;
  HS_HIP(hipMemcpyAsync(S.col, hcol.data(), sizeof(int64_t) * (size_t)gc, hipMemcpyHostToDevice, s));
  HS_HIP(hipStreamSynchronize(s));
  if (use_x0) {
    residual(gc);
  } else {
    HS_HIP(hipMemset2DAsync(X + (size_t)g0 * ldx, sizeof(T) * (size_t)ldx, 0, sizeof(T) * (size_t)n, (size_t)gc, s));
    HS_HIP(hipMemcpy2DAsync(ws.R, sizeof(T) * (size_t)ldv, B + (size_t)g0 * ldb, sizeof(T) * (size_t)ldb, sizeof(T) * (size_t)n, (size_t)gc, hipMemcpyDeviceToDevice, s));
  }
  norms(ws.R, S.beta, 1, gc, nullptr);
  read(S.beta, gc);
  std::vector<Column*> cur((size_t)gc);
  for (int c = 0; c < gc; ++c) {
    Column& q = cols[c];
    q.col = g0 + c;
    q.beta = hd[(size_t)c];
    q.tol = std::max(reltol * q.beta, abstol);
    q.hist.push_back(q.beta);
    q.conv = q.beta <= q.tol;
    cur[(size_t)c] = &q;
  }
  for (;;) {
    // the columns that go on move into the leading slots
    std::vector<Column*> next;
    bool moved = false;
    for (size_t c = 0; c < cur.size(); ++c)
      if (!cur[c]->conv && cur[c]->it < maxiter) {
        moved = moved || c != next.size();
        hsrc[next.size()] = (int)c;
        next.push_back(cur[c]);
      }
    if (next.empty()) break;
    const int nact = (int)next.size();
    if (moved) {
      HS_HIP(hipMemcpyAsync(ws.src, hsrc.data(), sizeof(int) * (size_t)nact, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(bgather_kernel<T>, dim3(gn, nact), dim3(256), 0, s, (const T*)ws.R, ws.R2, ldv, (const int*)ws.src, n);
      std::swap(ws.R, ws.R2);
    }
    cur.swap(next);
    for (int c = 0; c < nact; ++c) {
      Column& q = *cur[(size_t)c];
      hcol[(size_t)c] = q.col;
      hbeta[(size_t)c] = q.beta;
      htol[(size_t)c] = q.tol;
      hleft[(size_t)c] = (int)std::min<int64_t>(maxiter - q.it, 1 << 30);
      q.frozen = false;
    }
    HS_HIP(hipMemcpyAsync(S.col, hcol.data(), sizeof(int64_t) * (size_t)nact, hipMemcpyHostToDevice, s));
    HS_HIP(hipMemcpyAsync(S.beta, hbeta.data(), sizeof(double) * (size_t)nact, hipMemcpyHostToDevice, s));
    HS_HIP(hipMemcpyAsync(S.tol, htol.data(), sizeof(double) * (size_t)nact, hipMemcpyHostToDevice, s));
    HS_HIP(hipMemcpyAsync(S.itleft, hleft.data(), sizeof(int) * (size_t)nact, hipMemcpyHostToDevice, s));
    HS_HIP(hipStreamSynchronize(s));  // the host arrays are reused
    info[GI_CYCLES] += 1;
    info[GI_MAX_ACTIVE] = std::max(info[GI_MAX_ACTIVE], (double)nact);
    const unsigned gs = (unsigned)((nact + 63) / 64);
    hipLaunchKernelGGL(bscale_into_kernel<T>, dim3(gn, nact), dim3(256), 0, s, (const T*)ws.R, ldv, (const double*)S.beta, 1, ws.V, ldv, n, (const int*)nullptr);
    hipLaunchKernelGGL(breset_kernel<T>, dim3(gs), dim3(64), 0, s, S, m, nact);
    int running = nact;
    for (int k = 0; k < m && running > 0; ++k) {
      const T* Vk = ws.V + (size_t)k * jstride;
      const T* zz = Vk;
      if (F) {
        const int st = Pr(ws.Z, Vk, ldv, n, nact, s);
        if (st != 0) throw st;
        info[GI_PREC_CALLS] += 1;
        info[GI_COL_APPS] += nact;
        zz = ws.Z;
      }
      A(zz, ldv, (const int64_t*)nullptr, ws.W, ldv, (const T*)nullptr, (int64_t)0, (const int64_t*)nullptr, n, nact, s);
      info[GI_SPMM] += 1;
      // classical Gram-Schmidt with one re-orthogonalisation pass, per column: h = V^H w; w -= V h; h2 = V^H w; w -= V h2; H[:, k] = h + h2
      const int k1 = k + 1;
      const int* mask = S.mask;
      hipLaunchKernelGGL(bdot_kernel<T>, dim3(nblk, nact), dim3(256), 0, s, (const T*)ws.V, ldv, jstride, k1, (const T*)ws.W, ws.part, n, mask);
      hipLaunchKernelGGL(breduce_kernel<T>, dim3(nact), dim3(256), 0, s, (const T*)ws.part, nblk, k1, S.h, (T*)nullptr, S.s2, mask);
      hipLaunchKernelGGL(baxpy_kernel<T>, dim3(gn, nact), dim3(256), 0, s, (const T*)ws.V, ldv, jstride, k1, (const T*)S.h, S.s2, ws.W, n, mask);
      hipLaunchKernelGGL(bdot_kernel<T>, dim3(nblk, nact), dim3(256), 0, s, (const T*)ws.V, ldv, jstride, k1, (const T*)ws.W, ws.part, n, mask);
      hipLaunchKernelGGL(breduce_kernel<T>, dim3(nact), dim3(256), 0, s, (const T*)ws.part, nblk, k1, S.h2, S.h, S.s2, mask);
      hipLaunchKernelGGL(baxpy_kernel<T>, dim3(gn, nact), dim3(256), 0, s, (const T*)ws.V, ldv, jstride, k1, (const T*)S.h2, S.s2, ws.W, n, mask);
      norms(ws.W, S.hnres, 2, nact, mask);
      hipLaunchKernelGGL(bscale_into_kernel<T>, dim3(gn, nact), dim3(256), 0, s, (const T*)ws.W, ldv, (const double*)S.hnres, 2, ws.V + (size_t)(k + 1) * jstride, ldv, n, mask);
      hipLaunchKernelGGL(bgivens_kernel<T>, dim3(gs), dim3(64), 0, s, S, k, nact);
      read(S.hnres, 2 * nact);  // the one synchronisation of the step
      for (int c = 0; c < nact; ++c) {
        Column& q = *cur[(size_t)c];
        if (q.frozen) continue;
        const double hn = hd[(size_t)2 * c], res = hd[(size_t)2 * c + 1];
        ++q.it;
        q.hist.push_back(res);
        if (res <= q.tol || hn == 0.0 || q.it >= maxiter) {  // what bgivens_kernel decided for the mask
          q.conv = res <= q.tol;
          q.frozen = true;
          --running;
        }
      }
    }
    // x += Pr^-1 (V y), H y = g, every column with its own k_used; then the true residuals
    hipLaunchKernelGGL(bhess_solve_kernel<T>, dim3(gs), dim3(64), 0, s, S, nact);
    if (F) {
      hipLaunchKernelGGL(bcombine_kernel<T>, dim3(gn, nact), dim3(256), 0, s, (const T*)ws.V, ldv, jstride, (const T*)S.y, S.s1, (const int*)S.kused, (T*)nullptr, (int64_t)0,
                         (const int64_t*)nullptr, ws.W, ldv, n);
      const int st = Pr(ws.Z, ws.W, ldv, n, nact, s);
      if (st != 0) throw st;
      info[GI_PREC_CALLS] += 1;
      info[GI_COL_APPS] += nact;
      hipLaunchKernelGGL(badd_kernel<T>, dim3(gn, nact), dim3(256), 0, s, (const T*)ws.Z, ldv, X, ldx, (const int64_t*)S.col, n);
    } else {
      hipLaunchKernelGGL(bcombine_kernel<T>, dim3(gn, nact), dim3(256), 0, s, (const T*)ws.V, ldv, jstride, (const T*)S.y, S.s1, (const int*)S.kused, X, ldx,
                         (const int64_t*)S.col, (T*)nullptr, (int64_t)0, n);
    }
    residual(nact);
    norms(ws.R, S.beta, 1, nact, nullptr);
    read(S.beta, nact);
    for (int c = 0; c < nact; ++c) {
      Column& q = *cur[(size_t)c];
      q.beta = hd[(size_t)c];
      q.conv = q.conv || q.beta <= q.tol;
    }
  }
  HS_HIP(hipStreamSynchronize(s));
}

// G: the widest group (a multiple of the block solve's chunk width) whose workspace fits half of the free memory, HS_GMRES_BLOCK_GROUP overrides
int64_t group_width(size_t per_col, int64_t nrhs) {
  const int64_t KC = hs_ldiv_block_cols();
  const int64_t all = std::min<int64_t>((nrhs + KC - 1) / KC * KC, 32768);  // the column is blockIdx.y
  if (const char* e = getenv("HS_GMRES_BLOCK_GROUP")) {
    const long long v = atoll(e);
    if (v > 0) return std::min<int64_t>(all, (v + KC - 1) / KC * KC);
  }
  size_t fr = 0, tot = 0;
  HS_HIP(hipMemGetInfo(&fr, &tot));
  const int64_t fit = (int64_t)(fr / 2 / per_col);
  if (fit >= all) return all;
  if (fit < std::min<int64_t>(KC, nrhs))
    HS_FAIL(HS_ERR_NOMEM, 0, "OutOfMemoryError: hs_gmres_block_* needs %zu bytes for one group of %lld columns, half of the free device memory is %zu bytes",
            per_col * (size_t)std::min<int64_t>(KC, nrhs), (long long)std::min<int64_t>(KC, nrhs), fr / 2);
  return std::max<int64_t>(fit / KC * KC, std::min<int64_t>(KC, nrhs));
}

// the dimension test and the defaults every GMRES entry point applies after its own argument checks
template <class T>
void gmres_defaults(hs_handle* F, int64_t n, int64_t* restart, int64_t* maxiter, double* reltol) {
  if (F && (hs_size(F) != n || (hs_is_complex(F) != 0) != (sizeof(T) == 16)))
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: the preconditioner is %lld x %lld %s, A is %lld x %lld", (long long)hs_size(F), (long long)hs_size(F),
            hs_is_complex(F) ? "ComplexF64" : "Float64", (long long)n, (long long)n);
  // defaults of IterativeSolvers 0.9: restart = min(20, n), maxiter = n, reltol = sqrt(eps)
  if (*restart <= 0) *restart = std::min<int64_t>(20, n);
  if (*restart > GM_MAXK) HS_FAIL(HS_ERR_ARGUMENT, *restart, "ArgumentError: restart = %lld exceeds the limit of %d", (long long)*restart, GM_MAXK);
  if (*maxiter < 0) *maxiter = n;
  if (!(*reltol >= 0.0)) *reltol = 1.4901161193847656e-08;
}
// the checks and defaults hs_gmres_block_* and hs_gmres_block_t_* share (A and nrhs = 0 apart)
template <class T>
void gmres_block_check(hs_handle* F, int64_t n, const T* B, int64_t ldb, T* X, int64_t ldx, int where, int64_t* restart, int64_t* maxiter, double* reltol, int64_t* iters,
                       int* converged) {
  if (!B || !X || !iters || !converged || (const void*)B == (const void*)X)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_gmres_block needs B, X (not aliasing B) and the two result arrays");
  if (where != 0 && where != 1) HS_FAIL(HS_ERR_ARGUMENT, where, "ArgumentError: hs_gmres_block: where = %d (0: host pointers, 1: device pointers)", where);
  if (ldb < n || ldx < n)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_gmres_block: ldb = %lld, ldx = %lld below n = %lld", (long long)ldb, (long long)ldx, (long long)n);
  gmres_defaults<T>(F, n, restart, maxiter, reltol);
}
void need_device() {
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) HS_FAIL(HS_ERR_DEVICE, 0, "no HIP device available: this library has no CPU fallback");
}

// Every GMRES entry point from the device check to the results.  make_op(buf, s) puts A on the device (or finds it there) and returns the
// operator; width(bytes per column) is the group width the caller wants, asked after the device check; info receives the eight figures.
template <class T, class MakeOp, class Prec, class Width>
void gmres_run(MakeOp make_op, const Prec& Pr, Width width, double* info, int64_t n, const T* B, int64_t ldb, T* X, int64_t ldx, int64_t nrhs, int where, int use_x0,
               double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  need_device();
  hipStream_t s = (hipStream_t)stream;
  HsDevBuf buf("GMRES workspace");
  HsEvents<2> ev;
  HsDrain drain{s};  // after a throw nothing in flight outlives the workspace
  std::fill(info, info + 8, 0.0);
  const auto A = make_op(buf, s);
  const T* dB = B;
  T* dX = X;
  int64_t dldb = ldb, dldx = ldx;
  if (where == 0) {  // the whole block goes up and comes down once
    T* tb = buf.get<T>((size_t)n * nrhs);
    T* tx = buf.get<T>((size_t)n * nrhs);
    HS_HIP(hipMemcpy2D(tb, sizeof(T) * (size_t)n, B, sizeof(T) * (size_t)ldb, sizeof(T) * (size_t)n, (size_t)nrhs, hipMemcpyHostToDevice));
    if (use_x0) HS_HIP(hipMemcpy2D(tx, sizeof(T) * (size_t)n, X, sizeof(T) * (size_t)ldx, sizeof(T) * (size_t)n, (size_t)nrhs, hipMemcpyHostToDevice));
    dB = tb;
    dX = tx;
    dldb = dldx = n;
  }
  const int m = (int)restart;
  Workspace<T> ws;
  const size_t per_col = bytes_per_column<T>(n, m);
  ws.G = std::min<int64_t>(width(per_col), nrhs);
  ws.m = m;
  ws.ldv = (n + 1) / 2 * 2;
  ws.nblk = (int)((n + 1023) / 1024);
  const size_t G = (size_t)ws.G, blk = G * (size_t)ws.ldv;
  const size_t nvec = (size_t)m + (G > 1 ? 5 : 4);  // R2 serves compaction, which one column never sees
  T* big = buf.get<T>(nvec * blk);
  ws.V = big;
  ws.W = big + (size_t)(m + 1) * blk;
  ws.Z = ws.W + blk;
  ws.R = ws.Z + blk;
  ws.R2 = G > 1 ? ws.R + blk : nullptr;
  ws.part = buf.get<T>(G * ws.nblk * (m + 2));
  ws.dpart = buf.get<double>(G * ws.nblk);
  ws.src = buf.get<int>(G);
  GbSmall<T>& S = ws.S;
  S.ld = m + 1;
  S.sH = (m + 1) * m;
  S.s1 = m + 1;
  S.s2 = m + 2;
  S.H = buf.get<T>(G * S.sH);
  S.cs = buf.get<T>(G * S.s1);
  S.sn = buf.get<T>(G * S.s1);
  S.y = buf.get<T>(G * S.s1);
  S.g = buf.get<T>(G * S.s2);
  S.h = buf.get<T>(G * S.s2);
  S.h2 = buf.get<T>(G * S.s2);
  S.hnres = buf.get<double>(2 * G);
  S.beta = buf.get<double>(G);
  S.tol = buf.get<double>(G);
  S.itleft = buf.get<int>(G);
  S.mask = buf.get<int>(G);
  S.kused = buf.get<int>(G);
  S.col = buf.get<int64_t>(G);
  info[GI_WORK_BYTES] = (double)(per_col * G - ((size_t)m + 5 - nvec) * blk * sizeof(T));
  HS_HIP(hipEventRecord(ev[0], s));
  // a frozen column's basis vectors still travel through the block solve: they must be finite from the first step on
  HS_HIP(hipMemsetAsync(big, 0, sizeof(T) * nvec * blk, s));
  std::vector<Column> cols((size_t)nrhs);
  for (int64_t g0 = 0; g0 < nrhs; g0 += ws.G) {
    const int gc = (int)std::min<int64_t>(ws.G, nrhs - g0);
    gmres_group<T>(A, Pr, n, dB, dldb, dX, dldx, g0, gc, use_x0, reltol, abstol, maxiter, ws, cols.data() + g0, info, s);
    info[GI_GROUPS] += 1;
  }
  HS_HIP(hipEventRecord(ev[1], s));
  HS_HIP(hipEventSynchronize(ev[1]));
  float ms = 0.f;
  HS_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  info[GI_SECONDS] = ms * 1e-3;
  if (where == 0) HS_HIP(hipMemcpy2D(X, sizeof(T) * (size_t)ldx, dX, sizeof(T) * (size_t)n, sizeof(T) * (size_t)n, (size_t)nrhs, hipMemcpyDeviceToHost));
  for (int64_t c = 0; c < nrhs; ++c) {
    const Column& q = cols[(size_t)c];
    iters[c] = q.it;
    converged[c] = q.conv ? 1 : 0;
    if (resnorm)
      for (int64_t i = 0; i <= q.it; ++i) resnorm[(size_t)c * ((size_t)maxiter + 1) + (size_t)i] = q.hist[(size_t)i];
  }
}

// hs_gmres_block_*: groups as wide as the free device memory allows, the figures for hs_gmres_block_info
template <class T, class MakeOp, class Prec>
void gmres_block_run(MakeOp make_op, const Prec& Pr, int64_t n, const T* B, int64_t ldb, T* X, int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol,
                     int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  gmres_run<T>(make_op, Pr, [nrhs](size_t per_col) { return group_width(per_col, nrhs); }, g_info, n, B, ldb, X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter,
               resnorm, iters, converged, stream);
}
// hs_gmres_* / hs_gmres_t_*: one column in a group of width 1; the figures are nobody's
template <class T, class MakeOp, class Prec>
void gmres_one_run(MakeOp make_op, const Prec& Pr, int64_t n, const T* b, T* x, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter,
                   double* resnorm, int64_t* iters, int* converged, void* stream) {
  double unused[8];
  gmres_run<T>(make_op, Pr, [](size_t) { return (int64_t)1; }, unused, n, b, n, x, n, (int64_t)1, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged,
               stream);
}

// the CSR upload of the caller's CSC arrays as the operator
template <class T>
auto csr_op_of(int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz) {
  return [=](HsDevBuf& buf, hipStream_t) {
    int64_t* d_rp;
    int32_t* d_ci;
    T* d_v;
    upload_csr<T>(buf, n, colptr, rowval, nz, &d_rp, &d_ci, &d_v);
    return CsrSpmm<T>{d_rp, d_ci, d_v};
  };
}

template <class T>
void gmres_entry(hs_handle* F, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, const T* b, T* x, int where, int use_x0, double reltol, double abstol,
                 int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  if (n <= 0 || !colptr || !rowval || !nz || !b || !x || !iters || !converged)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_gmres needs A (CSC), b, x and the two result slots");
  gmres_defaults<T>(F, n, &restart, &maxiter, &reltol);
  // hs_ulv_mode 1 on a handle with HSS interior blocks: what hs_ldiv_ulv_dev_* refuses is refused here, before any device work (mode 0 keeps
  // its order of events: hs_ldiv_dev_* speaks inside the run, as it always did)
  if (hs_ulv_routed(F)) HS_CHECK(hs_block_probe<T>(F, HS_VIA_COLS, 0));
  gmres_one_run<T>(csr_op_of<T>(n, colptr, rowval, nz), PrecFwd<T>{F}, n, b, x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream);
}

// hs_gmres_t_*: op(A) x = b right-preconditioned by op(Pr); A explicit or the handle's own
template <class T>
void gmres_t_entry(hs_handle* F, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, const T* b, T* x, int where, int use_x0, double reltol,
                   double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  bool own = false;
  HS_CHECK(gm_check_op_args("hs_gmres_t_*", F, trans, colptr, rowval, nz, &own));
  if (trans == 0 && !own) return gmres_entry<T>(F, n, colptr, rowval, nz, b, x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream);
  if (n <= 0 || !b || !x || !iters || !converged) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_gmres_t needs n >= 1, b, x and the two result slots");
  gmres_defaults<T>(F, n, &restart, &maxiter, &reltol);
  if (own) HS_CHECK(hs_gmres_own_check(F, "hs_gmres_t_*", 1));
  // what hs_ldiv_t_* refuses (or an unfactored handle) is refused here, before any device work: zero columns are solved
  if (F) HS_CHECK((PrecOp<T>{F, trans}((T*)nullptr, (const T*)nullptr, n, n, 0, nullptr)));
  if (own) HS_CHECK(hs_gmres_own_check(F, "hs_gmres_t_*", 0));
  auto make_op = [&](HsDevBuf& buf, hipStream_t s) { return RowsSpmm<T>{gm_rows_of_op<T>(buf, F, trans, own, n, colptr, rowval, nz, s)}; };
  gmres_one_run<T>(make_op, PrecOp<T>{F, trans}, n, b, x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream);
}

// What the block solve refuses is refused before any device work, so nothing is silently looped: an "unsupported" is reworded for the caller
// of `fn` (`hint` says who serves such a handle), any other status travels on as it is (hs_block_apply.h).
template <class T>
void refuse_what_block_solve_refuses(hs_handle* F, int trans, const char* fn, const char* hint) {
  hs_block_probe_or_fail<T>(F, trans == 0 ? HS_VIA_BLOCK : HS_VIA_BLOCK_T, trans, fn, "preconditioner", hint, true);
}

template <class T>
void gmres_block_entry(hs_handle* F, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, const T* B, int64_t ldb, T* X, int64_t ldx, int64_t nrhs, int where,
                       int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  if (n <= 0 || nrhs < 0 || !colptr || !rowval || !nz) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_gmres_block needs A (CSC) and nrhs >= 0");
  if (nrhs == 0) {
    for (double& v : g_info) v = 0.0;
    return;
  }
  gmres_block_check<T>(F, n, B, ldb, X, ldx, where, &restart, &maxiter, &reltol, iters, converged);
  // (the hint is true only while hs_gmres_* takes another route than this call: with hs_ulv_mode 1 both go through hs_ldiv_ulv_dev_*)
  if (F) refuse_what_block_solve_refuses<T>(F, 0, "hs_gmres_block_*", hs_ulv_routed(F) ? "" : "; hs_gmres_* serves it, one right-hand side at a time");
  gmres_block_run<T>(csr_op_of<T>(n, colptr, rowval, nz), PrecBlockFwd<T>{F}, n, B, ldb, X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged,
                     stream);
}

// hs_gmres_block_t_*: op(A) X = B right-preconditioned by op(Pr); A explicit or the handle's own
template <class T>
void gmres_block_t_entry(hs_handle* F, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, const T* B, int64_t ldb, T* X, int64_t ldx, int64_t nrhs,
                         int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  bool own = false;
  HS_CHECK(gm_check_op_args("hs_gmres_block_t_*", F, trans, colptr, rowval, nz, &own));
  if (trans == 0 && !own)
    return gmres_block_entry<T>(F, n, colptr, rowval, nz, B, ldb, X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream);
  if (n <= 0 || nrhs < 0) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_gmres_block_t needs n >= 1 and nrhs >= 0");
  if (own && hs_size(F) != n)
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: the handle's own A is %lld x %lld, n = %lld", (long long)hs_size(F), (long long)hs_size(F), (long long)n);
  if (nrhs == 0) {
    for (double& v : g_info) v = 0.0;
    return;
  }
  gmres_block_check<T>(F, n, B, ldb, X, ldx, where, &restart, &maxiter, &reltol, iters, converged);
  if (own) HS_CHECK(hs_gmres_own_check(F, "hs_gmres_block_t_*", 1));
  if (F) refuse_what_block_solve_refuses<T>(F, trans, "hs_gmres_block_t_*", "");  // (whatever trans is)
  if (own) HS_CHECK(hs_gmres_own_check(F, "hs_gmres_block_t_*", 0));
  auto make_op = [&](HsDevBuf& buf, hipStream_t s) { return RowsSpmm<T>{gm_rows_of_op<T>(buf, F, trans, own, n, colptr, rowval, nz, s)}; };
  gmres_block_run<T>(make_op, PrecBlockOp<T>{F, trans}, n, B, ldb, X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream);
}

// What the entry below needs of a preconditioner object other than a handle: its names in the messages (fn, obj; mat: what the messages
// call the matrix; csc: why it must be given), the object's own size / element type check, the handle gmres_block_check and the row form
// of op(A) read (null: none), and the functor.
template <class T>
struct PrecObjMod {  // hs_gmres_block_mod_*: op(A1) X = B right-preconditioned by op(A1)^-1 as hs_mod_ldiv_dev_* applies it
  typedef hs_mod Obj;
  static constexpr const char *fn = "hs_gmres_block_mod_*", *obj = "hs_mod", *mat = "A1";
  static constexpr const char* csc = "the modified matrix A1 must be given as CSC (the handle holds the unmodified A)";
  static void check(hs_mod*, int64_t) {}
  static hs_handle* handle(hs_mod* M) { return hs_mod_handle(M); }
  static PrecBlockMod<T> prec(hs_mod* M, int trans) { return {hs_mod_handle(M), M, trans}; }
};
template <class T>
struct PrecObjF32 {  // hs_gmres_block_f32_*: op(A) X = B right-preconditioned by op(F)^-1 as hs_f32_ldiv_dev_* applies it
  typedef hs_f32 Obj;
  static constexpr const char *fn = "hs_gmres_block_f32_*", *obj = "hs_f32", *mat = "A";
  static constexpr const char* csc = "A must be given as CSC (a demoted factorization holds no matrix)";
  static void check(hs_f32* G, int64_t n) {
    if (hs_f32_size(G) != n || (hs_f32_is_complex(G) != 0) != (sizeof(T) == 16))
      HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: the preconditioner is %lld x %lld %s, A is %lld x %lld %s", (long long)hs_f32_size(G), (long long)hs_f32_size(G),
              hs_f32_is_complex(G) ? "ComplexF64" : "Float64", (long long)n, (long long)n, sizeof(T) == 16 ? "ComplexF64" : "Float64");
  }
  static hs_handle* handle(hs_f32*) { return nullptr; }
  static PrecBlockF32<T> prec(hs_f32* G, int trans) { return {reinterpret_cast<hs_handle*>(G), G, trans}; }
};

// op(A) X = B right-preconditioned by a preconditioner object other than a handle (O: above); A is the caller's CSC
template <class T, class O>
void gmres_block_obj_entry(typename O::Obj* P, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, const T* B, int64_t ldb, T* X, int64_t ldx,
                           int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged,
                           void* stream) {
  if (!P) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null %s", O::fn, O::obj);
  if (trans < 0 || trans > 2)
    HS_FAIL(HS_ERR_ARGUMENT, trans, "ArgumentError: %s: trans = %d (0: %s, 1: transpose(%s), 2: adjoint(%s))", O::fn, trans, O::mat, O::mat, O::mat);
  if (!colptr || !rowval || !nz) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: %s", O::fn, O::csc);
  if (n <= 0 || nrhs < 0) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s needs n >= 1 and nrhs >= 0", O::fn);
  O::check(P, n);
  if (nrhs == 0) {
    for (double& v : g_info) v = 0.0;
    return;
  }
  hs_handle* F = O::handle(P);
  gmres_block_check<T>(F, n, B, ldb, X, ldx, where, &restart, &maxiter, &reltol, iters, converged);
  const auto Pr = O::prec(P, trans);
  if (trans == 0)
    return gmres_block_run<T>(csr_op_of<T>(n, colptr, rowval, nz), Pr, n, B, ldb, X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged,
                              stream);
  auto make_op = [&](HsDevBuf& buf, hipStream_t s) { return RowsSpmm<T>{gm_rows_of_op<T>(buf, F, trans, false, n, colptr, rowval, nz, s)}; };
  gmres_block_run<T>(make_op, Pr, n, B, ldb, X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream);
}

// What hsk_spmm_* and hsk_spmm_op_* share once A is on the device: X, Y and B (null: none) go up as they are, launch(dX, dY, dB) runs on
// the null stream, Y comes down.
template <class T, class Launch>
void spmm_on_host_blocks(HsDevBuf& buf, const T* X, int64_t ldx, const T* B, int64_t ldb, T* Y, int64_t ldy, int64_t nrhs, Launch launch) {
  T* dX = buf.get<T>((size_t)ldx * nrhs);
  T* dY = buf.get<T>((size_t)ldy * nrhs);
  T* dB = B ? buf.get<T>((size_t)ldb * nrhs) : nullptr;
  HS_HIP(hipMemcpy(dX, X, sizeof(T) * (size_t)ldx * nrhs, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dY, Y, sizeof(T) * (size_t)ldy * nrhs, hipMemcpyHostToDevice));
  if (B) HS_HIP(hipMemcpy(dB, B, sizeof(T) * (size_t)ldb * nrhs, hipMemcpyHostToDevice));
  launch(dX, dY, dB);
  HS_HIP(hipDeviceSynchronize());
  HS_HIP(hipMemcpy(Y, dY, sizeof(T) * (size_t)ldy * nrhs, hipMemcpyDeviceToHost));
}

// hsk_spmm_*: the SpMM kernel alone on host data
template <class T>
void spmm_hook(int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, const T* X, int64_t ldx, const T* B, int64_t ldb, T* Y, int64_t ldy, int64_t nrhs) {
  if (n <= 0 || nrhs < 1 || !colptr || !rowval || !nz || !X || !Y || ldx < n || ldy < n || (B && ldb < n))
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_spmm: n >= 1, nrhs >= 1, leading dimensions >= n and non-null arrays required");
  need_device();
  HsDevBuf buf("GMRES workspace");
  int64_t* d_rp;
  int32_t* d_ci;
  T* d_v;
  upload_csr<T>(buf, n, colptr, rowval, nz, &d_rp, &d_ci, &d_v);
  spmm_on_host_blocks<T>(buf, X, ldx, B, ldb, Y, ldy, nrhs, [&](const T* dX, T* dY, const T* dB) {
    launch_spmm<T>(d_rp, d_ci, d_v, dX, ldx, (const int64_t*)nullptr, dY, ldy, dB, ldb, (const int64_t*)nullptr, n, (int)nrhs, (hipStream_t)0);
  });
}

// hsk_spmm_op_*: the op(A) SpMM kernel alone on host data.  trans = 0 reads the CSR upload of A, trans = 1, 2 the 0-based CSC upload itself.
template <class T>
void spmm_op_hook(int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, const T* X, int64_t ldx, const T* B, int64_t ldb, T* Y, int64_t ldy,
                  int64_t nrhs) {
  if (trans < 0 || trans > 2 || n <= 0 || nrhs < 1 || !colptr || !rowval || !nz || !X || !Y || ldx < n || ldy < n || (B && ldb < n))
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_spmm_op: trans in 0:2, n >= 1, nrhs >= 1, leading dimensions >= n and non-null arrays required");
  need_device();
  HsDevBuf buf("GMRES workspace");
  int64_t* d_p;
  int32_t* d_i;
  T* d_v;
  if (trans == 0)
    upload_csr<T>(buf, n, colptr, rowval, nz, &d_p, &d_i, &d_v);
  else
    upload_csc<T>(buf, n, colptr, rowval, nz, &d_p, &d_i, &d_v);
  RowsOf<T> A;
  A.ptr = d_p;
  A.idx = d_i;
  A.val = d_v;
  A.conj = trans == 2;
  spmm_on_host_blocks<T>(buf, X, ldx, B, ldb, Y, ldy, nrhs, [&](const T* dX, T* dY, const T* dB) {
    launch_spmm_op<T>(A, dX, ldx, (const int64_t*)nullptr, dY, ldy, dB, ldb, (const int64_t*)nullptr, n, (int)nrhs, (hipStream_t)0);
  });
}

}  // namespace

extern "C" int hs_gmres_d(hs_handle* Pr, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where, int use_x0,
                          double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_entry<double>(Pr, n, colptr, rowval, nzval, b, x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream));
}
extern "C" int hs_gmres_z(hs_handle* Pr, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where, int use_x0,
                          double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_entry<cplx>(Pr, n, colptr, rowval, (const cplx*)nzval, (const cplx*)b, (cplx*)x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged,
                             stream));
}
extern "C" int hs_gmres_t_d(hs_handle* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where,
                            int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_t_entry<double>(Pr, trans, n, colptr, rowval, nzval, b, x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream));
}
extern "C" int hs_gmres_t_z(hs_handle* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where,
                            int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_t_entry<cplx>(Pr, trans, n, colptr, rowval, (const cplx*)nzval, (const cplx*)b, (cplx*)x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters,
                               converged, stream));
}
extern "C" int hs_gmres_block_d(hs_handle* Pr, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb, double* X,
                                int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm,
                                int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_block_entry<double>(Pr, n, colptr, rowval, nzval, B, ldb, X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream));
}
extern "C" int hs_gmres_block_z(hs_handle* Pr, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb, double* X,
                                int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm,
                                int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_block_entry<cplx>(Pr, n, colptr, rowval, (const cplx*)nzval, (const cplx*)B, ldb, (cplx*)X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter, resnorm,
                                   iters, converged, stream));
}
static void gmres_block_info(double* out8) {
  if (!out8) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_gmres_block_info: null argument");
  for (int i = 0; i < 8; ++i) out8[i] = g_info[i];
}
extern "C" int hs_gmres_block_info(double* out8) { HS_GUARD(gmres_block_info(out8)); }
extern "C" int hsk_spmm_d(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* X, int64_t ldx, const double* B, int64_t ldb, double* Y,
                          int64_t ldy, int64_t nrhs) {
  HS_GUARD(spmm_hook<double>(n, colptr, rowval, nzval, X, ldx, B, ldb, Y, ldy, nrhs));
}
extern "C" int hsk_spmm_z(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* X, int64_t ldx, const double* B, int64_t ldb, double* Y,
                          int64_t ldy, int64_t nrhs) {
  HS_GUARD(spmm_hook<cplx>(n, colptr, rowval, (const cplx*)nzval, (const cplx*)X, ldx, (const cplx*)B, ldb, (cplx*)Y, ldy, nrhs));
}
extern "C" int hs_gmres_block_t_d(hs_handle* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb,
                                  double* X, int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm,
                                  int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_block_t_entry<double>(Pr, trans, n, colptr, rowval, nzval, B, ldb, X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged,
                                       stream));
}
extern "C" int hs_gmres_block_t_z(hs_handle* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb,
                                  double* X, int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm,
                                  int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_block_t_entry<cplx>(Pr, trans, n, colptr, rowval, (const cplx*)nzval, (const cplx*)B, ldb, (cplx*)X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter,
                                     resnorm, iters, converged, stream));
}
extern "C" int hsk_spmm_op_d(int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* X, int64_t ldx, const double* B,
                             int64_t ldb, double* Y, int64_t ldy, int64_t nrhs) {
  HS_GUARD(spmm_op_hook<double>(trans, n, colptr, rowval, nzval, X, ldx, B, ldb, Y, ldy, nrhs));
}
extern "C" int hsk_spmm_op_z(int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* X, int64_t ldx, const double* B,
                             int64_t ldb, double* Y, int64_t ldy, int64_t nrhs) {
  HS_GUARD(spmm_op_hook<cplx>(trans, n, colptr, rowval, (const cplx*)nzval, (const cplx*)X, ldx, (const cplx*)B, ldb, (cplx*)Y, ldy, nrhs));
}
extern "C" int hs_gmres_block_mod_d(hs_mod* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb,
                                    double* X, int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter,
                                    double* resnorm, int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_block_obj_entry<double, PrecObjMod<double>>(Pr, trans, n, colptr, rowval, nzval, B, ldb, X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged,
                                         stream));
}
extern "C" int hs_gmres_block_mod_z(hs_mod* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb,
                                    double* X, int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter,
                                    double* resnorm, int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_block_obj_entry<cplx, PrecObjMod<cplx>>(Pr, trans, n, colptr, rowval, (const cplx*)nzval, (const cplx*)B, ldb, (cplx*)X, ldx, nrhs, where, use_x0, reltol, abstol, restart,
                                       maxiter, resnorm, iters, converged, stream));
}
extern "C" int hs_gmres_block_f32_d(hs_f32* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb,
                                    double* X, int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter,
                                    double* resnorm, int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_block_obj_entry<double, PrecObjF32<double>>(Pr, trans, n, colptr, rowval, nzval, B, ldb, X, ldx, nrhs, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged,
                                         stream));
}
extern "C" int hs_gmres_block_f32_z(hs_f32* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* B, int64_t ldb,
                                    double* X, int64_t ldx, int64_t nrhs, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter,
                                    double* resnorm, int64_t* iters, int* converged, void* stream) {
  HS_GUARD(gmres_block_obj_entry<cplx, PrecObjF32<cplx>>(Pr, trans, n, colptr, rowval, (const cplx*)nzval, (const cplx*)B, ldb, (cplx*)X, ldx, nrhs, where, use_x0, reltol, abstol, restart,
                                       maxiter, resnorm, iters, converged, stream));
}
