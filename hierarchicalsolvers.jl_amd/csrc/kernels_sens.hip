// kernels_sens.hip -- the kernels of the adjoint-state sensitivities (hs_sens.h): the sampled dense-dense product over A's pattern in two
// forms, the diagonal mode, the row staging, and the small movers of the driver (copy / conjugate, expansion of a sparse block, misfit).
//
// Both forms give one lane one stored entry and run its chain serially in a register: no atomics, no cross-lane reduction, nothing whose
// shape depends on kc.  The direct form reads L[a, c] and R[b, c] from the column-major blocks: per column c the lanes of a wave read the
// rows `a` of their entries (neighbouring rows for a stencil in natural order) and share the row `b` of a column of A through the cache.  The
// row-staged form reads row a of Lt and row b of Rt, each one contiguous run of kc elements, 16 bytes per load.
#include <algorithm>

#include "hs_sens.h"

// no fused multiply-add in the chains: a step is the same rounded products and sums in every kernel of this file
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ double cj(double a, int) { return a; }
__device__ __forceinline__ cplx cj(cplx a, int on) { return on ? cplx{a.re, -a.im} : a; }
// acc - l * r
__device__ __forceinline__ double step(double acc, double l, double r) { return acc - l * r; }
__device__ __forceinline__ cplx step(cplx acc, cplx l, cplx r) { return {acc.re - (l.re * r.re - l.im * r.im), acc.im - (l.re * r.im + l.im * r.re)}; }

inline unsigned blocks_of(int64_t cnt, int per) { return (unsigned)std::max<int64_t>(1, (cnt + per - 1) / per); }

__global__ __launch_bounds__(256) void entry_cols_kernel(const int64_t* __restrict__ colptr, int64_t n, int64_t nnz, int32_t* __restrict__ ecol) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= nnz) return;
  int64_t lo = 0, hi = n;  // colptr[lo] <= p < colptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (colptr[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  ecol[p] = (int32_t)lo;
}

template <class T>
__global__ __launch_bounds__(256) void sddmm_kernel(const int32_t* __restrict__ rowval, const int32_t* __restrict__ ecol, int64_t nnz, const T* __restrict__ L, int64_t ldl,
                                                    const T* __restrict__ R, int64_t ldr, int kc, HsSddmmFlags f, T* __restrict__ G) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= nnz) return;
  const int32_t i = rowval[p], j = ecol[p];
  const T* lp = L + (f.swap ? j : i);
  const T* rp = R + (f.swap ? i : j);
  T acc = G[p];
#pragma unroll 4
  for (int c = 0; c < kc; ++c) acc = step(acc, cj(gld(lp + (size_t)c * ldl), f.conjl), cj(gld(rp + (size_t)c * ldr), f.conjr));
  G[p] = acc;
}

// 16 bytes per load: two columns of a Float64 row, one of a ComplexF64 row (rows start 16-byte aligned: hs_sens_row_stride)
__device__ __forceinline__ double row_chain(double acc, const double* lp, const double* rp, int kc, HsSddmmFlags) {
  int c = 0;
#pragma unroll 4
  for (; c + 1 < kc; c += 2) {
    const double2 l = *(const double2*)(lp + c), r = *(const double2*)(rp + c);
    acc = step(acc, l.x, r.x);
    acc = step(acc, l.y, r.y);
  }
  if (c < kc) acc = step(acc, lp[c], rp[c]);
  return acc;
}
__device__ __forceinline__ cplx row_chain(cplx acc, const cplx* lp, const cplx* rp, int kc, HsSddmmFlags f) {
#pragma unroll 4
  for (int c = 0; c < kc; ++c) acc = step(acc, cj(gld(lp + c), f.conjl), cj(gld(rp + c), f.conjr));
  return acc;
}
template <class T>
__global__ __launch_bounds__(256) void sddmm_rows_kernel(const int32_t* __restrict__ rowval, const int32_t* __restrict__ ecol, int64_t nnz, const T* __restrict__ Lt,
                                                         const T* __restrict__ Rt, int64_t stride, int kc, HsSddmmFlags f, T* __restrict__ G) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= nnz) return;
  const int32_t i = rowval[p], j = ecol[p];
  const T* lp = Lt + (size_t)(f.swap ? j : i) * stride;
  const T* rp = Rt + (size_t)(f.swap ? i : j) * stride;
  G[p] = row_chain(G[p], lp, rp, kc, f);
}

// in: n x kc column-major -> out: row r at out + r * stride.  A workgroup moves 64 rows, 32 columns at a time, through a padded tile: the
// reads run along the rows of `in`, the writes along the columns of a row of `out`.
template <class T>
__global__ __launch_bounds__(256) void rowstage_kernel(const T* __restrict__ in, int64_t ld, int64_t n, int kc, T* __restrict__ out, int64_t stride) {
  __shared__ T tile[64][33];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  for (int c0 = 0; c0 < kc; c0 += 32) {
    {
      const int r = tid & 63;
      for (int cc = tid >> 6; cc < 32; cc += 4)
        if (r0 + r < n && c0 + cc < kc) tile[r][cc] = in[(size_t)(c0 + cc) * ld + r0 + r];
    }
    __syncthreads();
    {
      const int cc = tid & 31;
      for (int r = tid >> 5; r < 64; r += 8)
        if (r0 + r < n && c0 + cc < kc) out[(size_t)(r0 + r) * stride + c0 + cc] = tile[r][cc];
    }
    __syncthreads();
  }
}

template <class T>
__global__ __launch_bounds__(256) void sddmm_diag_kernel(const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval, int64_t n, const T* __restrict__ L,
                                                         int64_t ldl, const T* __restrict__ R, int64_t ldr, int kc, HsSddmmFlags f, T* __restrict__ Gd) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  bool found = false;
  for (int64_t e = colptr[j], e1 = colptr[j + 1]; e < e1 && !found; ++e) found = rowval[e] == (int32_t)j;
  if (!found) {
    Gd[j] = Scal<T>::zero();
    return;
  }
  const T* lp = L + j;
  const T* rp = R + j;
  T acc = Gd[j];
#pragma unroll 4
  for (int c = 0; c < kc; ++c) acc = step(acc, cj(gld(lp + (size_t)c * ldl), f.conjl), cj(gld(rp + (size_t)c * ldr), f.conjr));
  Gd[j] = acc;
}

template <class T>
__global__ __launch_bounds__(256) void copy_kernel(T* __restrict__ out, int64_t ldo, const T* __restrict__ in, int64_t ldi, int64_t n, int conj) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t c = blockIdx.y;
  out[c * ldo + i] = cj(in[c * ldi + i], conj);
}
template <class T>
__global__ __launch_bounds__(256) void expand_kernel(T* __restrict__ out, int64_t ldo, const int32_t* __restrict__ erow, const int32_t* __restrict__ ecol,
                                                     const T* __restrict__ val, int64_t cnt, int conj) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= cnt) return;
  out[(size_t)ecol[e] * ldo + erow[e]] = cj(val[e], conj);
}

__device__ __forceinline__ double abs2(double a) { return a * a; }
__device__ __forceinline__ double abs2(cplx a) { return a.re * a.re + a.im * a.im; }
template <class T>
__global__ __launch_bounds__(256) void misfit_kernel(const T* __restrict__ X, int64_t ldx, const int32_t* __restrict__ rows, const int32_t* __restrict__ slot,
                                                     const T* __restrict__ D, int64_t ldd, int64_t nrows, T* __restrict__ R, int64_t ldr, T* __restrict__ Wv, int conj,
                                                     double* __restrict__ J) {
  __shared__ double sh[256];
  const size_t c = blockIdx.x;
  double sum = 0.0;
  for (int64_t q = threadIdx.x; q < nrows; q += 256) {
    const T r = X[c * ldx + rows[q]] - D[c * ldd + q];
    if (R) R[c * ldr + q] = r;
    Wv[c * nrows + slot[q]] = cj(r, conj);
    sum += abs2(r);
  }
  sh[threadIdx.x] = sum;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) J[c] = 0.5 * sh[0];
}

}  // namespace

void launch_sens_entry_cols(const int64_t* colptr, int64_t n, int64_t nnz, int32_t* ecol, hipStream_t s) {
  if (nnz <= 0) return;
  hipLaunchKernelGGL(entry_cols_kernel, dim3(blocks_of(nnz, 256)), dim3(256), 0, s, colptr, n, nnz, ecol);
}
int64_t hs_sens_row_stride(int kc, int is_complex) { return is_complex ? kc : (kc + 1) / 2 * 2; }

template <class T>
void launch_sddmm(const int32_t* rowval, const int32_t* ecol, int64_t nnz, const T* L, int64_t ldl, const T* R, int64_t ldr, int kc, HsSddmmFlags f, T* G, hipStream_t s) {
  if (nnz <= 0 || kc <= 0) return;
  hipLaunchKernelGGL(sddmm_kernel<T>, dim3(blocks_of(nnz, 256)), dim3(256), 0, s, rowval, ecol, nnz, L, ldl, R, ldr, kc, f, G);
}
template <class T>
void launch_sens_rowstage(const T* in, int64_t ld, int64_t n, int kc, T* out, int64_t stride, hipStream_t s) {
  if (n <= 0 || kc <= 0) return;
  hipLaunchKernelGGL(rowstage_kernel<T>, dim3(blocks_of(n, 64)), dim3(256), 0, s, in, ld, n, kc, out, stride);
}
template <class T>
void launch_sddmm_rows(const int32_t* rowval, const int32_t* ecol, int64_t nnz, const T* Lt, const T* Rt, int64_t stride, int kc, HsSddmmFlags f, T* G, hipStream_t s) {
  if (nnz <= 0 || kc <= 0) return;
  hipLaunchKernelGGL(sddmm_rows_kernel<T>, dim3(blocks_of(nnz, 256)), dim3(256), 0, s, rowval, ecol, nnz, Lt, Rt, stride, kc, f, G);
}
template <class T>
void launch_sddmm_diag(const int64_t* colptr, const int32_t* rowval, int64_t n, const T* L, int64_t ldl, const T* R, int64_t ldr, int kc, HsSddmmFlags f, T* Gd,
                       hipStream_t s) {
  if (n <= 0 || kc <= 0) return;
  hipLaunchKernelGGL(sddmm_diag_kernel<T>, dim3(blocks_of(n, 256)), dim3(256), 0, s, colptr, rowval, n, L, ldl, R, ldr, kc, f, Gd);
}
template <class T>
void launch_sens_copy(T* out, int64_t ldo, const T* in, int64_t ldi, int64_t n, int kc, int conj, hipStream_t s) {
  if (n <= 0 || kc <= 0) return;
  hipLaunchKernelGGL(copy_kernel<T>, dim3(blocks_of(n, 256), (unsigned)kc), dim3(256), 0, s, out, ldo, in, ldi, n, conj);
}
template <class T>
void launch_sens_expand(T* out, int64_t ldo, const int32_t* erow, const int32_t* ecol, const T* val, int64_t cnt, int conj, hipStream_t s) {
  if (cnt <= 0) return;
  hipLaunchKernelGGL(expand_kernel<T>, dim3(blocks_of(cnt, 256)), dim3(256), 0, s, out, ldo, erow, ecol, val, cnt, conj);
}
template <class T>
void launch_sens_misfit(const T* X, int64_t ldx, const int32_t* rows, const int32_t* slot, const T* D, int64_t ldd, int64_t nrows, int kc, T* R, int64_t ldr, T* Wv,
                        int conj, double* J, hipStream_t s) {
  if (kc <= 0) return;
  hipLaunchKernelGGL(misfit_kernel<T>, dim3((unsigned)kc), dim3(256), 0, s, X, ldx, rows, slot, D, ldd, nrows, R, ldr, Wv, conj, J);
}

#define INST(T)                                                                                                                                            \
  template void launch_sddmm<T>(const int32_t*, const int32_t*, int64_t, const T*, int64_t, const T*, int64_t, int, HsSddmmFlags, T*, hipStream_t);        \
  template void launch_sens_rowstage<T>(const T*, int64_t, int64_t, int, T*, int64_t, hipStream_t);                                                       \
  template void launch_sddmm_rows<T>(const int32_t*, const int32_t*, int64_t, const T*, const T*, int64_t, int, HsSddmmFlags, T*, hipStream_t);            \
  template void launch_sddmm_diag<T>(const int64_t*, const int32_t*, int64_t, const T*, int64_t, const T*, int64_t, int, HsSddmmFlags, T*, hipStream_t);   \
  template void launch_sens_copy<T>(T*, int64_t, const T*, int64_t, int64_t, int, int, hipStream_t);                                                      \
  template void launch_sens_expand<T>(T*, int64_t, const int32_t*, const int32_t*, const T*, int64_t, int, hipStream_t);                                  \
  template void launch_sens_misfit<T>(const T*, int64_t, const int32_t*, const int32_t*, const T*, int64_t, int64_t, int, T*, int64_t, T*, int, double*, hipStream_t);
INST(double)
INST(cplx)
