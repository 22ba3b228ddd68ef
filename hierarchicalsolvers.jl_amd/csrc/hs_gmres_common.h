// hs_gmres_common.h -- what the two GMRES drivers share (hs_gmres.hip: one vector, hs_gmres_block.hip: a block in lockstep): the restart
// limit, the scalar helpers of the kernels, the device-buffer holder and the CSC -> CSR upload.  Everything has internal linkage.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/hs_solver.h"
#include "hs_common.h"

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

struct DevBuf {
  std::vector<void*> p;
  ~DevBuf() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
  template <class U>
  U* get(size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(count * sizeof(U), 256)) != hipSuccess) {
      hs_set_error(HS_ERR_NOMEM, 0, "hipMalloc of %zu bytes failed (GMRES workspace)", count * sizeof(U));
      throw (int)HS_ERR_NOMEM;
    }
    p.push_back(q);
    return (U*)q;
  }
};

#define GM_HIP(call)                                                                              \
  do {                                                                                            \
    hipError_t e__ = (call);                                                                      \
    if (e__ != hipSuccess) {                                                                      \
      hs_set_error(HS_ERR_DEVICE, 0, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
      throw (int)HS_ERR_DEVICE;                                                                   \
    }                                                                                             \
  } while (0)

// CSR (0-based, device) of a host CSC matrix given with 1-based Julia fields
template <class T>
void upload_csr(DevBuf& buf, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, int64_t** d_rp, int32_t** d_ci, T** d_v) {
  if (colptr[0] != 1) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: colptr must be 1-based (SparseMatrixCSC)");
    throw (int)HS_ERR_ARGUMENT;
  }
  const int64_t nnz = colptr[n] - 1;
  std::vector<int64_t> rp((size_t)n + 1, 0);
  std::vector<int32_t> ci((size_t)nnz);
  std::vector<T> v((size_t)nnz);
  for (int64_t e = 0; e < nnz; ++e) {
    if (rowval[e] < 1 || rowval[e] > n) {
      hs_set_error(HS_ERR_DIMENSION, e, "BoundsError: rowval[%lld] = %lld outside 1:%lld", (long long)e + 1, (long long)rowval[e], (long long)n);
      throw (int)HS_ERR_DIMENSION;
    }
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
  GM_HIP(hipMemcpy(*d_rp, rp.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice));
  GM_HIP(hipMemcpy(*d_ci, ci.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
  GM_HIP(hipMemcpy(*d_v, v.data(), sizeof(T) * (size_t)nnz, hipMemcpyHostToDevice));
}

}  // namespace
