// kernels_gn.hip -- the kernels of the tangent-linear solves and Gauss-Newton products (hs_gn.h): the right-hand side P = -op(E) X of the
// tangent solve, the receiver rows of its solution, the row square sums and the diagonal of the Gauss-Newton Hessian.
//
// The right-hand side gives one lane one row of op(E) and a register chunk of columns: per stored entry the lane reads the value of E once
// (in place: through the CSR map's permutation for trans = 0, straight from the CSC order otherwise) and one element of X per column of
// its chunk; the lanes of a wave own neighbouring rows, which for a stencil in natural order read neighbouring rows of X.
#include <algorithm>

#include "hs_gn.h"

// no fused multiply-add in the sums: a step is the same rounded products and sums as in kernels_sens.hip
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ double cj(double a, int) { return a; }
__device__ __forceinline__ cplx cj(cplx a, int on) { return on ? cplx{a.re, -a.im} : a; }
// acc - l * r
__device__ __forceinline__ double step(double acc, double l, double r) { return acc - l * r; }
__device__ __forceinline__ cplx step(cplx acc, cplx l, cplx r) { return {acc.re - (l.re * r.re - l.im * r.im), acc.im - (l.re * r.im + l.im * r.re)}; }
__device__ __forceinline__ double abs2(double a) { return a * a; }
__device__ __forceinline__ double abs2(cplx a) { return a.re * a.re + a.im * a.im; }

inline unsigned blocks_of(int64_t cnt, int per) { return (unsigned)std::max<int64_t>(1, (cnt + per - 1) / per); }

template <class T>
struct Chunk {  // columns a lane keeps in registers
  static constexpr int W = sizeof(T) == 16 ? 4 : 8;
};

template <class T>
__global__ __launch_bounds__(256) void rhs_kernel(HsGnRows r, const T* __restrict__ E, int64_t n, const T* __restrict__ X, int64_t ldx, int kc, T* __restrict__ P,
                                                  int64_t ldp) {
  constexpr int W = Chunk<T>::W;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c0 = (int)blockIdx.y * W;
  T acc[W];
#pragma unroll
  for (int u = 0; u < W; ++u) acc[u] = Scal<T>::zero();
  for (int64_t e = r.ptr[i], e1 = r.ptr[i + 1]; e < e1; ++e) {
    const T v = cj(gld(E + (r.perm ? r.perm[e] : e)), r.conj);
    const T* xp = X + r.idx[e];
#pragma unroll
    for (int u = 0; u < W; ++u)
      if (c0 + u < kc) acc[u] = step(acc[u], v, gld(xp + (size_t)(c0 + u) * ldx));
  }
#pragma unroll
  for (int u = 0; u < W; ++u)
    if (c0 + u < kc) P[(size_t)(c0 + u) * ldp + i] = acc[u];
}

template <class T>
__global__ __launch_bounds__(256) void rhs_diag_kernel(const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval, const T* __restrict__ Ed, int conj, int64_t n,
                                                       const T* __restrict__ X, int64_t ldx, int kc, T* __restrict__ P, int64_t ldp) {
  constexpr int W = Chunk<T>::W;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c0 = (int)blockIdx.y * W;
  bool found = false;
  for (int64_t e = colptr[i], e1 = colptr[i + 1]; e < e1 && !found; ++e) found = rowval[e] == (int32_t)i;
  const T v = cj(Ed[i], conj);
#pragma unroll
  for (int u = 0; u < W; ++u)
    if (c0 + u < kc) P[(size_t)(c0 + u) * ldp + i] = found ? step(Scal<T>::zero(), v, gld(X + (size_t)(c0 + u) * ldx + i)) : Scal<T>::zero();
}

template <class T>
__global__ __launch_bounds__(256) void rows_kernel(const T* __restrict__ D, int64_t ldd, const int32_t* __restrict__ rows, const int32_t* __restrict__ slot, int64_t nrows,
                                                   T* __restrict__ JE, int64_t ldj, T* __restrict__ Wv, int conj) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= nrows) return;
  const size_t c = blockIdx.y;
  const T v = D[c * ldd + rows[q]];
  if (JE) JE[c * ldj + q] = v;
  if (Wv) Wv[c * nrows + slot[q]] = cj(v, conj);
}

template <class T>
__global__ __launch_bounds__(256) void rowsq_kernel(const T* __restrict__ X, int64_t ldx, int64_t n, int kc, double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double a = acc[i];
#pragma unroll 4
  for (int c = 0; c < kc; ++c) a = a + abs2(gld(X + (size_t)c * ldx + i));
  acc[i] = a;
}

__global__ __launch_bounds__(256) void diag_kernel(const int32_t* __restrict__ rowval, const int32_t* __restrict__ ecol, int64_t nnz, const double* __restrict__ z2,
                                                   const double* __restrict__ x2, int swap, double* __restrict__ Hd) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= nnz) return;
  const int32_t i = rowval[p], j = ecol[p];
  Hd[p] = z2[swap ? j : i] * x2[swap ? i : j];
}
__global__ __launch_bounds__(256) void diag_diag_kernel(const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval, int64_t n, const double* __restrict__ z2,
                                                        const double* __restrict__ x2, double* __restrict__ Hd) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  bool found = false;
  for (int64_t e = colptr[j], e1 = colptr[j + 1]; e < e1 && !found; ++e) found = rowval[e] == (int32_t)j;
  Hd[j] = found ? z2[j] * x2[j] : 0.0;
}

}  // namespace

template <class T>
void launch_gn_rhs(HsGnRows r, const T* E, int64_t n, const T* X, int64_t ldx, int kc, T* P, int64_t ldp, hipStream_t s) {
  if (n <= 0 || kc <= 0) return;
  constexpr int W = Chunk<T>::W;
  hipLaunchKernelGGL(rhs_kernel<T>, dim3(blocks_of(n, 256), (unsigned)((kc + W - 1) / W)), dim3(256), 0, s, r, E, n, X, ldx, kc, P, ldp);
}
template <class T>
void launch_gn_rhs_diag(const int64_t* colptr, const int32_t* rowval, const T* Ed, int conj, int64_t n, const T* X, int64_t ldx, int kc, T* P, int64_t ldp, hipStream_t s) {
  if (n <= 0 || kc <= 0) return;
  constexpr int W = Chunk<T>::W;
  hipLaunchKernelGGL(rhs_diag_kernel<T>, dim3(blocks_of(n, 256), (unsigned)((kc + W - 1) / W)), dim3(256), 0, s, colptr, rowval, Ed, conj, n, X, ldx, kc, P, ldp);
}
template <class T>
void launch_gn_rows(const T* D, int64_t ldd, const int32_t* rows, const int32_t* slot, int64_t nrows, int kc, T* JE, int64_t ldj, T* Wv, int conj, hipStream_t s) {
  if (nrows <= 0 || kc <= 0) return;
  hipLaunchKernelGGL(rows_kernel<T>, dim3(blocks_of(nrows, 256), (unsigned)kc), dim3(256), 0, s, D, ldd, rows, slot, nrows, JE, ldj, Wv, conj);
}
template <class T>
void launch_gn_rowsq(const T* X, int64_t ldx, int64_t n, int kc, double* acc, hipStream_t s) {
  if (n <= 0 || kc <= 0) return;
  hipLaunchKernelGGL(rowsq_kernel<T>, dim3(blocks_of(n, 256)), dim3(256), 0, s, X, ldx, n, kc, acc);
}
void launch_gn_diag(const int32_t* rowval, const int32_t* ecol, int64_t nnz, const double* z2, const double* x2, int swap, double* Hd, hipStream_t s) {
  if (nnz <= 0) return;
  hipLaunchKernelGGL(diag_kernel, dim3(blocks_of(nnz, 256)), dim3(256), 0, s, rowval, ecol, nnz, z2, x2, swap, Hd);
}
void launch_gn_diag_diag(const int64_t* colptr, const int32_t* rowval, int64_t n, const double* z2, const double* x2, double* Hd, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(diag_diag_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, colptr, rowval, n, z2, x2, Hd);
}

#define INST(T)                                                                                                                                  \
  template void launch_gn_rhs<T>(HsGnRows, const T*, int64_t, const T*, int64_t, int, T*, int64_t, hipStream_t);                                  \
  template void launch_gn_rhs_diag<T>(const int64_t*, const int32_t*, const T*, int, int64_t, const T*, int64_t, int, T*, int64_t, hipStream_t);  \
  template void launch_gn_rows<T>(const T*, int64_t, const int32_t*, const int32_t*, int64_t, int, T*, int64_t, T*, int, hipStream_t);            \
  template void launch_gn_rowsq<T>(const T*, int64_t, int64_t, int, double*, hipStream_t);
INST(double)
INST(cplx)
