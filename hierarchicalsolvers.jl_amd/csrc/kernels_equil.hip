// kernels_equil.hip -- device code of hs_options.equilibrate: the Ruiz sweeps that find the power-of-two row and column scales of A, the
// scaled copy of its values, and the row scaling of a block of right-hand sides (hs_common.h has the contracts).
//
// Everything that decides an exponent is integer arithmetic on the exponent field of a double: ldexp by an integer is exact, a maximum does
// not depend on the order it is taken in, and floor(log2 m) is read with frexp.  Two runs, and a NumPy restatement, give the same exponents.
#include <float.h>

#include "hs_common.h"

__device__ __forceinline__ double equil_mag(double a) { return fabs(a); }
__device__ __forceinline__ double equil_mag(cplx a) { return fabs(a.re) + fabs(a.im); }  // as zgeequb

// ------------------------------------------------------------------------------------------------
// equil_maxima: one thread per column c.  The column maximum is a loop; the row maxima over the CSC arrays are atomicMax on the bit
// pattern of the non-negative double (the order of two such doubles is the order of their patterns).  An entry that cannot raise its row's
// maximum -- most of them after the first few columns -- skips the atomic: a stale read only costs an atomic that changes nothing.
// ------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void equil_maxima_kernel(int64_t n, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval, const T* __restrict__ nz,
                                                           const int32_t* __restrict__ er, const int32_t* __restrict__ ec, unsigned long long* rmax,
                                                           unsigned long long* __restrict__ cmax) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int sc = ec[c];
  double cm = 0.0;
  for (int64_t e = colptr[c]; e < colptr[c + 1]; ++e) {
    const int32_t r = rowval[e];
    const double m = ldexp(equil_mag(gld(nz + e)), er[r] + sc);
    if (!(m > 0.0)) continue;  // (a stored zero; NaN never enters a maximum)
    cm = fmax(cm, m);
    const unsigned long long b = (unsigned long long)__double_as_longlong(m);
    if (b > rmax[r]) atomicMax(rmax + r, b);
  }
  cmax[c] = (unsigned long long)__double_as_longlong(cm);
}

// -floor((floor(log2 m) + 1) / 2): frexp gives m = f 2^e with f in [0.5, 1), so floor(log2 m) + 1 = e.  An infinite maximum -- an
// infinite entry, or a magnitude near the largest double that overflowed (|re| + |im| can, unscaled) -- has no exponent to read and moves
// nothing: that row and column keep their exponents and may end outside [0.5, 2) (include/hs_solver.h says so)
__device__ __forceinline__ int equil_step(unsigned long long bits) {
  const double m = __longlong_as_double((long long)bits);
  if (!(m > 0.0) || isinf(m)) return 0;
  int e;
  (void)frexp(m, &e);
  return -(e >= 0 ? e / 2 : -((1 - e) / 2));
}

__global__ __launch_bounds__(256) void equil_update_kernel(int64_t n, const unsigned long long* __restrict__ rmax, const unsigned long long* __restrict__ cmax,
                                                           int32_t* __restrict__ er, int32_t* __restrict__ ec, int* __restrict__ changed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int dr = equil_step(rmax[i]), dc = equil_step(cmax[i]);
  if (dr) er[i] += dr;
  if (dc) ec[i] += dc;
  if (dr | dc) *changed = 1;  // (every writer writes the same value)
}

// ------------------------------------------------------------------------------------------------
// equil_scale: one thread per column
// ------------------------------------------------------------------------------------------------
// a non-zero finite x whose ldexp left the normal range
__device__ __forceinline__ bool equil_lost(double x, double y) { return x != 0.0 && !isinf(x) && x == x && (isinf(y) || fabs(y) < DBL_MIN); }
__device__ __forceinline__ bool equil_scaled(double a, int s, double& out) {
  out = ldexp(a, s);
  return equil_lost(a, out);
}
__device__ __forceinline__ bool equil_scaled(cplx a, int s, cplx& out) {
  out.re = ldexp(a.re, s);
  out.im = ldexp(a.im, s);
  return equil_lost(a.re, out.re) || equil_lost(a.im, out.im);
}

template <class T>
__global__ __launch_bounds__(256) void equil_scale_kernel(int64_t n, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval, const T* __restrict__ nz,
                                                          const int32_t* __restrict__ er, const int32_t* __restrict__ ec, T* __restrict__ nzs,
                                                          unsigned long long* __restrict__ bad) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int sc = ec[c];
  bool lost = false;
  for (int64_t e = colptr[c]; e < colptr[c + 1]; ++e) {
    T v;
    if (equil_scaled(gld(nz + e), er[rowval[e]] + sc, v) && !lost) {
      atomicMin(bad, (unsigned long long)e);  // (the entries of a column come in increasing e)
      lost = true;
    }
    gst(nzs + e, v);
  }
}

// ------------------------------------------------------------------------------------------------
// scale_rows: C[i, j] = ldexp(B[i, j], e[i]); threads along a column (contiguous), blockIdx.y strides over the columns
// ------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void scale_rows_kernel(int64_t n, int64_t nrhs, const int32_t* __restrict__ e, const T* B, int64_t ldb, T* C, int64_t ldc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = e[i];
  for (int64_t j = blockIdx.y; j < nrhs; j += gridDim.y) {
    T v;
    (void)equil_scaled(gld(B + j * ldb + i), s, v);
    gst(C + j * ldc + i, v);
  }
}

template <class T>
void launch_equil_maxima(int64_t n, const int64_t* colptr, const int32_t* rowval, const T* nz, const int32_t* er, const int32_t* ec, unsigned long long* rmax,
                         unsigned long long* cmax, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(equil_maxima_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, colptr, rowval, nz, er, ec, rmax, cmax);
}
void launch_equil_update(int64_t n, const unsigned long long* rmax, const unsigned long long* cmax, int32_t* er, int32_t* ec, int* changed, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(equil_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, rmax, cmax, er, ec, changed);
}
template <class T>
void launch_equil_scale(int64_t n, const int64_t* colptr, const int32_t* rowval, const T* nz, const int32_t* er, const int32_t* ec, T* nzs, unsigned long long* bad,
                        hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(equil_scale_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, colptr, rowval, nz, er, ec, nzs, bad);
}
template <class T>
void launch_scale_rows(int64_t n, int64_t nrhs, const int32_t* e, const T* B, int64_t ldb, T* C, int64_t ldc, hipStream_t s) {
  if (n <= 0 || nrhs <= 0) return;
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)std::min<int64_t>(nrhs, 1024));
  hipLaunchKernelGGL(scale_rows_kernel<T>, grid, dim3(256), 0, s, n, nrhs, e, B, ldb, C, ldc);
}

#define HS_INST(T)                                                                                                                                              \
  template void launch_equil_maxima<T>(int64_t, const int64_t*, const int32_t*, const T*, const int32_t*, const int32_t*, unsigned long long*, unsigned long long*, \
                                       hipStream_t);                                                                                                            \
  template void launch_equil_scale<T>(int64_t, const int64_t*, const int32_t*, const T*, const int32_t*, const int32_t*, T*, unsigned long long*, hipStream_t);  \
  template void launch_scale_rows<T>(int64_t, int64_t, const int32_t*, const T*, int64_t, T*, int64_t, hipStream_t);
HS_INST(double)
HS_INST(cplx)
#undef HS_INST
