// hs_condest.h -- what the accuracy tools (hs_condest.hip: norm and condition estimates, refined solves; hs_refine_block.hip: refined solves
// for a block in lockstep) read from a factorization handle: hs_api.hip owns the handle, and the two calls below are the whole interface to
// it.  Behind HS_CONDEST_KERNELS: what the two files share besides the estimator (hs_normest.h) -- scalar helpers, the +-1 hash, the xGERFS
// ratio, the op(F)^-1 code table, the rows of op(A), and the argument checks of the refined solves.  Errors, device buffers and the
// refusals every module words alike are hs_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct hs_handle;

struct HsHandleView {
  int64_t n = 0, nnz = 0;
  int is_complex = 0;
  int factored = 0;        // a numeric factorization is complete
  int device = 0;          // 0: a host-side plan only (hs_plan)
  int nranks = 1;
  int t_refused_node = -1; // first owned node whose transposed solve is refused (D kept as an HSS matrix: hss_d, mf = 2, 3); -1: none
  int ulv = 0;             // hs_ulv_mode is 1 and t_refused_node >= 0: op(F)^-1 goes through hs_ldiv_ulv_dev_* (hs_block_apply.h)
  int64_t seed = 0;        // hs_options.seed
  const int64_t* colptr = nullptr;  // A in CSC on the device, 0-based; hs_numeric_begin keeps the values current
  const int32_t* rowval = nullptr;
  const void* nz = nullptr;
  const int64_t* rowptr = nullptr;  // hs_options.mf: the CSR pattern the matrix-free fronts already keep (CSR entry -> CSC entry in tperm); else null
  const int32_t* colind = nullptr;
  const int64_t* tperm = nullptr;
  hipStream_t stream = nullptr;     // the handle's own stream
  void** cx = nullptr;              // cache slot of hs_condest.hip (the CSR map of A), freed by hs_free through *cx_free
  void (**cx_free)(void*) = nullptr;
};

void hs_handle_view(hs_handle* h, HsHandleView* v);
// HsHandleView::ulv alone (null: 0): what hs_block_apply.h asks before every application; no node is looked at while hs_ulv_mode is 0
int hs_handle_ulv_routed(const hs_handle* h);
// HS_OK, or HS_ERR_DEVICE with hs_last_error set when a dataflow sweep since the last check timed out (call after every synchronisation)
int hs_handle_flow_check(hs_handle* h);

// ---- shared by hs_condest.hip and hs_refine_block.hip (define HS_CONDEST_KERNELS before the include; needs hs_solver.h and hs_common.h) ----
#ifdef HS_CONDEST_KERNELS
#include <algorithm>
#include <vector>

#include "hs_host.h"
// No contraction of a*b + c into an fma from here to the end of the including file: residuals and weights are the plain products and sums,
// entry by entry, in both files (see hs_condest.hip).
#pragma clang fp contract(off)

#define CE_ROWS 2048    // rows per workgroup of the reduction kernels (256 threads x 8)

namespace hs_ce {

// ---- scalar helpers ------------------------------------------------------------------------------------------------------------
__device__ inline double abs_(double a) { return fabs(a); }
__device__ inline double abs_(cplx a) { return hypot(a.re, a.im); }
__device__ inline double abs1_(double a) { return fabs(a); }
__device__ inline double abs1_(cplx a) { return fabs(a.re) + fabs(a.im); }  // cabs1, as zgerfs
template <bool CJ>
__device__ inline double cj_(double a) { return a; }
template <bool CJ>
__device__ inline cplx cj_(cplx a) { return CJ ? cplx{a.re, -a.im} : a; }
__device__ inline double sign_(double a) { return a >= 0.0 ? 1.0 : -1.0; }  // sign(0) = 1
__device__ inline cplx sign_(cplx a) {
  const double m = hypot(a.re, a.im);
  return m == 0.0 ? cplx{1.0, 0.0} : cplx{a.re / m, a.im / m};
}
template <class T>
__device__ inline T from_real(double a);
template <>
__device__ inline double from_real<double>(double a) { return a; }
template <>
__device__ inline cplx from_real<cplx>(double a) { return {a, 0.0}; }
__device__ inline double mul_(double a, double b) { return a * b; }
__device__ inline cplx mul_(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ inline double add_(double a, double b) { return a + b; }
__device__ inline cplx add_(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ inline double sub_(double a, double b) { return a - b; }
__device__ inline cplx sub_(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ inline double scale_(double a, double s) { return a * s; }
__device__ inline cplx scale_(cplx a, double s) { return {a.re * s, a.im * s}; }

__host__ __device__ inline uint64_t sm64(uint64_t x) {  // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// the +-1 column `col` of draw `salt` (0: the start block; k * 64 + attempt: a re-drawn sign column of iteration k): entry i = low bit of
// splitmix64(key ^ i)
__host__ __device__ inline uint64_t col_key(int64_t seed, int col, int salt) { return sm64(sm64((uint64_t)seed) ^ ((uint64_t)salt << 8) ^ (uint64_t)col); }
__device__ inline double pm1(uint64_t key, int64_t i) { return (sm64(key ^ (uint64_t)i) & 1) ? -1.0 : 1.0; }

// the xGERFS ratio |r_i| / w_i with its safe1 / safe2 guard
struct ResidArgs {
  double safe1, safe2;
};
__device__ inline double berr_ratio(double ra, double wa, ResidArgs g) { return wa > g.safe2 ? ra / wa : (ra + g.safe1) / (wa + g.safe1); }

inline unsigned nb256(int64_t cnt) { return (unsigned)std::max<int64_t>(1, (cnt + 255) / 256); }
inline unsigned nbrows(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + CE_ROWS - 1) / CE_ROWS); }

// kept in the handle (hs_handle::cx): the CSR map of A (borrowed from the matrix-free fronts when hs_options.mf built one), a buffer for its
// values, and the longest row / column of A
struct CsrMap {
  int64_t* rowptr = nullptr;
  int32_t* colind = nullptr;
  int64_t* tperm = nullptr;
  bool owned = false;
  void* valr = nullptr;
  int64_t maxrow = -1, maxcol = -1;
};

constexpr double CE_EPS = 1.1102230246251565e-16;     // dlamch('Epsilon') = 2^-53
constexpr double CE_SAFMIN = 2.2250738585072014e-308;  // dlamch('Safe minimum')

// hs_condest.hip: the longest column of A, and the CSR map of A (built on first use, kept in the handle) with its values gathered from the
// CSC values of the last hs_numeric_begin
int64_t max_col(const HsHandleView& v, hipStream_t s);
template <class T>
CsrMap* csr_of(const HsHandleView& v, hipStream_t s);

// ---- op(F)^-1 by code ---------------------------------------------------------------------------------------------------------------------
// 0 = F^-1, 1 = F^-T, 2 = F^-H, 3 = conj(F)^-1; adj() gives the code of the adjoint.  A solve takes trans = 0, 1, 2: real T folds 2 and 3 into
// 1 and 0, and code 3 is conjugate, solve with trans = 0, conjugate.
inline int adj(int code) { return code == 0 ? 2 : code == 1 ? 3 : code == 2 ? 0 : 1; }
struct OpDir {
  int trans;  // of the solve
  bool conj;  // conjugate the block before and after it
};
template <class T>
inline OpDir op_dir(int code) {
  if (sizeof(T) == 8) code = (code == 2) ? 1 : (code == 3 ? 0 : code);
  return {code == 3 ? 0 : code, code == 3};
}

// ---- the rows of op(A) ------------------------------------------------------------------------------------------------------------------
// Row i of op(A) is row i of the CSR map (op = N) or column i of the CSC arrays (op = T, H: cj conjugates on load); nz = its longest row + 1
// and the safe1 / safe2 guards of xGERFS go with it.
template <class T>
struct OpRows {
  const int64_t* ptr;
  const int32_t* idx;
  const T* val;
  int64_t maxlen;
  bool cj;
  double nz;
  ResidArgs g;
};
template <class T>
OpRows<T> op_rows(const HsHandleView& v, int trans, hipStream_t s) {
  OpRows<T> r;
  if (trans == 0) {
    CsrMap* m = csr_of<T>(v, s);
    r.ptr = m->rowptr;
    r.idx = m->colind;
    r.val = (const T*)m->valr;
    r.maxlen = m->maxrow;
  } else {
    r.ptr = v.colptr;
    r.idx = v.rowval;
    r.val = (const T*)v.nz;
    r.maxlen = max_col(v, s);
  }
  r.cj = trans == 2 && sizeof(T) == 16;
  r.nz = (double)(r.maxlen + 1);
  r.g = ResidArgs{r.nz * CE_SAFMIN, r.nz * CE_SAFMIN / CE_EPS};
  return r;
}

// ---- argument checks of the refined solves: refuse, never drop ---------------------------------------------------------------------------
// hs_ldiv_refine_* and hs_ldiv_refine_block_* refuse the same things with the same words (fn names the entry point), in the same order; what
// differs -- ranks, a host-side plan, the HSS-D node, the probe of the block solve -- stays with each entry point, between these three.
template <class T>
void check_refine_args(const char* fn, const HsHandleView& v, int trans, const T* X, int64_t ldx, const T* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                       const double* berr, const int64_t* steps) {
  if ((v.is_complex != 0) != (sizeof(T) == 16)) HS_FAIL(HS_ERR_ARGUMENT, 0, "MethodError: %s: eltype of F and B differ", fn);
  hs_check_trans(fn, trans);
  if (n != v.n || nrhs < 0 || ldx < n || ldb < n)
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: B has %lld rows (ldx %lld, ldb %lld, nrhs %lld), F is %lld x %lld", fn, (long long)n, (long long)ldx,
            (long long)ldb, (long long)nrhs, (long long)v.n, (long long)v.n);
  if (itmax < 0) HS_FAIL(HS_ERR_ARGUMENT, itmax, "ArgumentError: %s: itmax = %lld < 0", fn, (long long)itmax);
  if (nrhs > 0 && (!X || !B || !berr || !steps)) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: X, B, berr and steps must not be NULL", fn);
}
template <class T>
void check_no_alias(const char* fn, const T* X, int64_t ldx, const T* B, int64_t ldb, int64_t nrhs) {
  if (nrhs > 0 && X < B + (size_t)ldb * nrhs && B < X + (size_t)ldx * nrhs) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: X may not alias B", fn);
}

}  // namespace hs_ce
#endif  // HS_CONDEST_KERNELS
