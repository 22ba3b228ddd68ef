// hs_gmres_common.h -- what the GMRES driver (hs_gmres_block.hip: hs_gmres_* and hs_gmres_block_*) shares with the other Krylov code
// (hs_eigs.hip): the restart limit, the scalar helpers of the kernels, the CSC -> CSR upload, and what the
// hs_gmres_t_* / hs_gmres_block_t_* calls add: the product with op(A) over "entry ranges as rows", the 0-based CSC upload and the checks of
// their arguments.  Everything has internal linkage.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/hs_solver.h"
#include "hs_common.h"
#include "hs_host.h"
#include "hs_gmres_op.h"

#define GM_MAXK 64  // restart length limit (Krylov vectors held: restart + 1)

namespace {

template <class T>
__device__ inline T conj_(T a);
template <>
__device__ inline double conj_<double>(double a) { return a; }
template <>
__device__ inline cplx conj_<cplx>(cplx a) { return {a.re, -a.im}; }
template <class T>
__device__ inline double abs2_(T a);
template <>
__device__ inline double abs2_<double>(double a) { return a * a; }
template <>
__device__ inline double abs2_<cplx>(cplx a) { return a.re * a.re + a.im * a.im; }
template <class T>
__device__ inline T scale_(T a, double s);
template <>
__device__ inline double scale_<double>(double a, double s) { return a * s; }
template <>
__device__ inline cplx scale_<cplx>(cplx a, double s) { return {a.re * s, a.im * s}; }

__device__ inline double absT(double a) { return fabs(a); }
__device__ inline double absT(cplx a) { return sqrt(a.re * a.re + a.im * a.im); }

// the device forms of A hold row / column indices in 32 bits
inline void gm_check_index_width(int64_t n) {
  if (n > (int64_t)INT32_MAX) HS_FAIL(HS_ERR_ARGUMENT, n, "ArgumentError: n = %lld exceeds the 32-bit indices of the device matrix (limit %d)", (long long)n, INT32_MAX);
}

// CSR (0-based, device) of a host CSC matrix given with 1-based Julia fields
template <class T>
void upload_csr(HsDevBuf& buf, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, int64_t** d_rp, int32_t** d_ci, T** d_v) {
  gm_check_index_width(n);
  if (colptr[0] != 1) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: colptr must be 1-based (SparseMatrixCSC)");
  const int64_t nnz = colptr[n] - 1;
  std::vector<int64_t> rp((size_t)n + 1, 0);
  std::vector<int32_t> ci((size_t)nnz);
  std::vector<T> v((size_t)nnz);
  for (int64_t e = 0; e < nnz; ++e) {
    if (rowval[e] < 1 || rowval[e] > n) HS_FAIL(HS_ERR_DIMENSION, e, "BoundsError: rowval[%lld] = %lld outside 1:%lld", (long long)e + 1, (long long)rowval[e], (long long)n);
    rp[(size_t)rowval[e]]++;
  }
  for (int64_t r = 0; r < n; ++r) rp[(size_t)r + 1] += rp[(size_t)r];
  std::vector<int64_t> fill(rp.begin(), rp.end() - 1);
  for (int64_t c = 0; c < n; ++c)
    for (int64_t e = colptr[c] - 1; e < colptr[c + 1] - 1; ++e) {
      const int64_t at = fill[(size_t)(rowval[e] - 1)]++;
      ci[(size_t)at] = (int32_t)c;
      v[(size_t)at] = nz[e];
    }
  *d_rp = buf.get<int64_t>((size_t)n + 1);
  *d_ci = buf.get<int32_t>((size_t)nnz);
  *d_v = buf.get<T>((size_t)nnz);
  HS_HIP(hipMemcpy(*d_rp, rp.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(*d_ci, ci.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(*d_v, v.data(), sizeof(T) * (size_t)nnz, hipMemcpyHostToDevice));
}

// ---- op(A) over "entry ranges as rows" (hs_gmres_t_*, hs_gmres_block_t_*) -------------------------------------------------------------
// Row i of the operator is the entry range ptr[i] .. ptr[i + 1] of (idx, val): a CSR of A, or -- the rows of transpose(A) ARE the columns
// of A -- the CSC arrays of A as the handle holds them (64-bit colptr, 32-bit rowval), read in place.  CJ conjugates every value as it is
// loaded (adjoint(A)); no transposed or conjugated copy exists anywhere.
template <class T>
struct RowsOf {
  const int64_t* ptr = nullptr;
  const int32_t* idx = nullptr;
  const T* val = nullptr;
  bool conj = false;
};
template <bool CJ, class T>
__device__ inline T opval_(T a) {
  if constexpr (CJ) return conj_(a);
  return a;
}
// Y[:, c] = op(A) X[:, xmap[c]]   or, with B,   Y[:, c] = B[:, bmap[c]] - op(A) X[:, xmap[c]]   (null map: identity), c < nc.  CJ = false on a
// CSR is the product of hs_gmres_* and hs_gmres_block_* (launch_spmm, hs_gmres_block.hip).  256 rows per workgroup, lanes along rows, CB columns of accumulators in registers, the row's
// entries read once per chunk of CB columns; per (row, column) the sum runs over the stored entries in order with Scal<T>::fma.
template <class T, int CB, bool CJ>
__global__ __launch_bounds__(256) void spmm_op_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val,
                                                      const T* __restrict__ X, int64_t ldx, const int64_t* __restrict__ xmap, T* __restrict__ Y, int64_t ldy,
                                                      const T* __restrict__ B, int64_t ldb, const int64_t* __restrict__ bmap, int64_t n, int nc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t e0 = ptr[i], e1 = ptr[i + 1];
  for (int c0 = 0; c0 < nc; c0 += CB) {
    T acc[CB];
    const T* xp[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const int cc = min(c0 + c, nc - 1);  // a ragged chunk recomputes its last column and does not store it
      xp[c] = X + (size_t)(xmap ? xmap[cc] : cc) * ldx;
      acc[c] = Scal<T>::zero();
    }
    for (int64_t e = e0; e < e1; ++e) {
      const T a = opval_<CJ>(val[e]);
      const int32_t j = idx[e];
#pragma unroll
      for (int c = 0; c < CB; ++c) acc[c] = Scal<T>::fma(a, xp[c][j], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const int cc = c0 + c;
      if (cc < nc) Y[(size_t)cc * ldy + i] = B ? B[(size_t)(bmap ? bmap[cc] : cc) * ldb + i] - acc[c] : acc[c];
    }
  }
}
template <class T>
void launch_spmm_op(const RowsOf<T>& A, const T* X, int64_t ldx, const int64_t* xmap, T* Y, int64_t ldy, const T* B, int64_t ldb, const int64_t* bmap, int64_t n, int nc,
                    hipStream_t s) {
  constexpr int CB = sizeof(T) == 16 ? 4 : 8;
  const dim3 g((unsigned)((n + 255) / 256));
  if constexpr (sizeof(T) == 16)  // Float64: the adjoint is the transpose
    if (A.conj) {
      hipLaunchKernelGGL((spmm_op_kernel<T, CB, true>), g, dim3(256), 0, s, A.ptr, A.idx, A.val, X, ldx, xmap, Y, ldy, B, ldb, bmap, n, nc);
      return;
    }
  hipLaunchKernelGGL((spmm_op_kernel<T, CB, false>), g, dim3(256), 0, s, A.ptr, A.idx, A.val, X, ldx, xmap, Y, ldy, B, ldb, bmap, n, nc);
}

// The CSC arrays of a host matrix (1-based Julia fields) on the device, 0-based with 32-bit row indices -- the form the handle keeps its
// own A in.  The host rebases the indices and nothing else: no transposition, no pass that reorders the values.
template <class T>
void upload_csc(HsDevBuf& buf, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, int64_t** d_cp, int32_t** d_ri, T** d_v) {
  gm_check_index_width(n);
  if (colptr[0] != 1) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: colptr must be 1-based (SparseMatrixCSC)");
  const int64_t nnz = colptr[n] - 1;
  std::vector<int64_t> cp((size_t)n + 1);
  std::vector<int32_t> ri((size_t)nnz);
  for (int64_t c = 0; c <= n; ++c) {
    cp[(size_t)c] = colptr[c] - 1;
    if (cp[(size_t)c] < (c ? cp[(size_t)c - 1] : 0) || cp[(size_t)c] > nnz) HS_FAIL(HS_ERR_ARGUMENT, c, "ArgumentError: colptr[%lld] = %lld is not monotone within 1:%lld", (long long)c + 1, (long long)colptr[c], (long long)nnz + 1);
  }
  for (int64_t e = 0; e < nnz; ++e) {
    if (rowval[e] < 1 || rowval[e] > n) HS_FAIL(HS_ERR_DIMENSION, e, "BoundsError: rowval[%lld] = %lld outside 1:%lld", (long long)e + 1, (long long)rowval[e], (long long)n);
    ri[(size_t)e] = (int32_t)(rowval[e] - 1);
  }
  *d_cp = buf.get<int64_t>((size_t)n + 1);
  *d_ri = buf.get<int32_t>((size_t)nnz);
  *d_v = buf.get<T>((size_t)nnz);
  HS_HIP(hipMemcpy(*d_cp, cp.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(*d_ri, ri.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(*d_v, nz, sizeof(T) * (size_t)nnz, hipMemcpyHostToDevice));
}

// What hs_gmres_t_* and hs_gmres_block_t_* check first, with no device work: trans, and how A is passed (all three arrays, or none of them
// = the handle's own A, which needs the handle).  *own receives whether the handle's A is meant.
inline int gm_check_op_args(const char* fn, hs_handle* F, int trans, const void* colptr, const void* rowval, const void* nz, bool* own) {
  if (trans < 0 || trans > 2) {
    hs_set_error(HS_ERR_ARGUMENT, trans, "ArgumentError: %s: trans = %d (0: A, 1: transpose(A), 2: adjoint(A))", fn, trans);
    return HS_ERR_ARGUMENT;
  }
  const int given = (colptr ? 1 : 0) + (rowval ? 1 : 0) + (nz ? 1 : 0);
  if (given != 0 && given != 3) {
    hs_set_error(HS_ERR_ARGUMENT, given, "ArgumentError: %s: colptr, rowval and nzval must all be given, or all be NULL (the handle's own A)", fn);
    return HS_ERR_ARGUMENT;
  }
  *own = given == 0;
  if (*own && !F) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: colptr = rowval = nzval = NULL selects the matrix of the handle Pr, which is NULL", fn);
    return HS_ERR_ARGUMENT;
  }
  return HS_OK;
}
// the rows of op(A): the handle's own A (no host pass, no upload), or an upload of the caller's CSC arrays (trans != 0 only)
template <class T>
RowsOf<T> gm_rows_of_op(HsDevBuf& buf, hs_handle* F, int trans, bool own, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, hipStream_t s) {
  RowsOf<T> A;
  A.conj = trans == 2;
  if (own) {
    HsGmresRows r;
    const int st = hs_gmres_own_rows(F, trans, s, &r);
    if (st != HS_OK) throw st;
    A.ptr = r.ptr;
    A.idx = r.idx;
    A.val = (const T*)r.val;
  } else {
    int64_t* cp;
    int32_t* ri;
    T* v;
    upload_csc<T>(buf, n, colptr, rowval, nz, &cp, &ri, &v);
    A.ptr = cp;
    A.idx = ri;
    A.val = v;
  }
  return A;
}

}  // namespace
