// hs_condest.hip -- the accuracy tools of a factorization behind the C ABI (include/hs_solver.h): ||A||_1 and ||A||_Inf of the handle's A,
// the Higham-Tisseur block 1-norm estimate of op(F)^-1 (Julia's opnormestinv, LAPACK xGECON), cond(A, p), and refined solves with the
// componentwise backward error berr and the forward error bound ferr of LAPACK xGERFS.
//
// The Higham-Tisseur estimator is est_run of hs_normest.h, shared with hs_refine_block.hip: here it runs a single estimator (ne = 1) whose
// application of op(F)^-1 is one hs_ldiv_dev_t_* call on its t columns -- <8> for hs_normestinv and hs_condest, <2> on diag(v) op(F)^-H for
// ferr.  Every n-vector operation is a kernel; the host reads a few scalars per half-step (like hs_gmres_block.hip) and checks the dataflow-sweep
// error flag after every synchronisation, so a timed-out sweep becomes an error and never an estimate.
//
// Determinism: the estimator's is stated in hs_normest.h; the residual, the weights and the norms here are per-workgroup partials in LDS and
// one ordered final pass, the only atomics are on integers (row counts).  Two calls on the same handle return the same bits.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/hs_solver.h"
#include "hs_common.h"
#define HS_CONDEST_KERNELS
#include "hs_condest.h"
#include "hs_normest.h"
#include "hs_block_apply.h"

// No contraction of a*b + c into an fma in this file: the residual r = b - op(A) x and the weights w are then the plain products and sums, row by
// row in column order, that scipy's CSR product computes -- a test can recompute berr from the returned X and compare (berr is ~eps, and the
// rounding of r is of the size of r itself).
#pragma clang fp contract(off)

#define CE_MAXT 8                         // estimator columns of hs_normestinv and hs_condest
#define CE_MAXIT EstDim<CE_MAXT>::ITMAX   // their estimator iterations (the index history holds t * itmax entries)
#define CE_WAVE_ROW 64  // rows of op(A) longer than this are gathered by a whole wave (graphs from hs_symbolic_from_graph)

using namespace hs_ce;

namespace {

// ---- residual, norms, CSR map ----------------------------------------------------------------------------------------------------
// Row i of op(A) is row i of the CSR map (op = N) or column i of the CSC arrays (op = T, H: CJ conjugates).  One pass reads A, x, b and
// writes r = b - op(A) x and w = |b| + |op(A)| |x| (cabs1), and the workgroup's max of the xGERFS ratio |r_i| / w_i (safe1 / safe2 guard).
template <class T, bool CJ>
__global__ __launch_bounds__(256) void resid_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val,
                                                    const T* __restrict__ x, const T* __restrict__ b, T* __restrict__ r, double* __restrict__ w,
                                                    double* __restrict__ part, int64_t n, ResidArgs g) {
  __shared__ double sh[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double ratio = 0.0;
  if (i < n) {
    T acc = Scal<T>::zero();
    double wa = 0.0;
    for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
      const T a = cj_<CJ>(val[e]);
      const T xv = x[idx[e]];
      acc = add_(acc, mul_(a, xv));
      wa += abs1_(a) * abs1_(xv);
    }
    const T bi = b[i];
    const T ri = sub_(bi, acc);
    wa += abs1_(bi);
    r[i] = ri;
    w[i] = wa;
    ratio = berr_ratio(abs1_(ri), wa, g);
  }
  sh[threadIdx.x] = ratio;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
// the same with one wave per row (rows longer than CE_WAVE_ROW entries): lanes stride the row, a fixed butterfly sums the lanes
template <class T>
__device__ inline T shfl_xor_(T v, int m);
template <>
__device__ inline double shfl_xor_<double>(double v, int m) { return __shfl_xor(v, m, 64); }
template <>
__device__ inline cplx shfl_xor_<cplx>(cplx v, int m) { return {__shfl_xor(v.re, m, 64), __shfl_xor(v.im, m, 64)}; }
template <class T, bool CJ>
__global__ __launch_bounds__(256) void resid_wave_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val,
                                                         const T* __restrict__ x, const T* __restrict__ b, T* __restrict__ r, double* __restrict__ w,
                                                         double* __restrict__ part, int64_t n, ResidArgs g) {
  __shared__ double sh[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + wv;
  double ratio = 0.0;
  if (i < n) {
    T acc = Scal<T>::zero();
    double wa = 0.0;
    for (int64_t e = ptr[i] + lane; e < ptr[i + 1]; e += 64) {
      const T a = cj_<CJ>(val[e]);
      const T xv = x[idx[e]];
      acc = add_(acc, mul_(a, xv));
      wa += abs1_(a) * abs1_(xv);
    }
    for (int m = 32; m > 0; m >>= 1) {
      acc = add_(acc, shfl_xor_<T>(acc, m));
      wa += __shfl_xor(wa, m, 64);
    }
    if (lane == 0) {
      const T bi = b[i];
      const T ri = sub_(bi, acc);
      wa += abs1_(bi);
      r[i] = ri;
      w[i] = wa;
      ratio = berr_ratio(abs1_(ri), wa, g);
    }
  }
  if (lane == 0) sh[wv] = ratio;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}
// out[0] = max of part[0..cnt)   (one workgroup)
__global__ __launch_bounds__(256) void max_final_kernel(const double* __restrict__ part, int64_t cnt, double* __restrict__ out) {
  __shared__ double sh[256];
  double m = 0.0;
  for (int64_t b = threadIdx.x; b < cnt; b += 256) m = fmax(m, part[b]);
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}
// part[b] = max over the workgroup's entries of cabs1(x)
template <class T>
__global__ __launch_bounds__(256) void absmax_part_kernel(const T* __restrict__ x, int64_t n, double* __restrict__ part) {
  __shared__ double sh[256];
  double m = 0.0;
  for (int q = 0; q < CE_ROWS / 256; ++q) {
    const int64_t i = (int64_t)blockIdx.x * CE_ROWS + q * 256 + threadIdx.x;
    if (i < n) m = fmax(m, abs1_(x[i]));
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
// v = |r| + nz eps w (+ safe1 where w is tiny): the xGERFS weights of the forward error bound
template <class T>
__global__ __launch_bounds__(256) void ferr_weights_kernel(const T* __restrict__ r, const double* __restrict__ w, double* __restrict__ v, int64_t n,
                                                           double nzeps, ResidArgs g) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double wi = w[i];
  v[i] = wi > g.safe2 ? abs1_(r[i]) + nzeps * wi : abs1_(r[i]) + nzeps * wi + g.safe1;
}
template <class T>
__global__ __launch_bounds__(256) void axpy1_kernel(T* __restrict__ x, const T* __restrict__ d, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = add_(x[i], d[i]);
}
// sums[i] = sum_e |val[e]| over entry range i (a column of CSC or a row of CSR), in entry order
template <class T>
__global__ __launch_bounds__(256) void abssum_kernel(const int64_t* __restrict__ ptr, const T* __restrict__ val, int64_t n, double* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) acc += abs_(val[e]);
  sums[i] = acc;
}
__global__ __launch_bounds__(256) void dmax_part_kernel(const double* __restrict__ a, int64_t n, double* __restrict__ part) {
  __shared__ double sh[256];
  double m = 0.0;
  for (int q = 0; q < CE_ROWS / 256; ++q) {
    const int64_t i = (int64_t)blockIdx.x * CE_ROWS + q * 256 + threadIdx.x;
    if (i < n) m = fmax(m, a[i]);
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
// CSR map of the pattern: count entries per row, scan, place, sort each row by column
__global__ __launch_bounds__(256) void csr_count_kernel(const int32_t* __restrict__ rowval, int64_t nnz, unsigned long long* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < nnz) atomicAdd(cnt + rowval[e] + 1, 1ull);
}
// inclusive scan of a[0..len) in place (one workgroup of 1024: contiguous chunks, a scan of the chunk sums in LDS, then the chunks)
__global__ __launch_bounds__(1024) void scan_kernel(int64_t* __restrict__ a, int64_t len) {
  __shared__ int64_t sh[1024];
  const int64_t chunk = (len + 1023) / 1024;
  const int64_t lo = (int64_t)threadIdx.x * chunk, hi = min(len, lo + chunk);
  int64_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += a[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int st = 1; st < 1024; st <<= 1) {
    const int64_t v = (int)threadIdx.x >= st ? sh[threadIdx.x - st] : 0;
    __syncthreads();
    sh[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t run = sh[threadIdx.x] - s;  // exclusive prefix of this chunk
  for (int64_t i = lo; i < hi; ++i) {
    run += a[i];
    a[i] = run;
  }
}
__global__ __launch_bounds__(256) void csr_place_kernel(const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval, int64_t n,
                                                        unsigned long long* __restrict__ cursor, int32_t* __restrict__ colind, int64_t* __restrict__ tperm) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  for (int64_t e = colptr[c]; e < colptr[c + 1]; ++e) {
    const unsigned long long at = atomicAdd(cursor + rowval[e], 1ull);
    colind[at] = (int32_t)c;
    tperm[at] = e;
  }
}
__global__ __launch_bounds__(256) void csr_sort_kernel(const int64_t* __restrict__ rowptr, int32_t* __restrict__ colind, int64_t* __restrict__ tperm, int64_t n) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int64_t lo = rowptr[r], hi = rowptr[r + 1];
  for (int64_t a = lo + 1; a < hi; ++a) {  // insertion sort: stencil rows are short, the map is built once
    const int32_t c = colind[a];
    const int64_t p = tperm[a];
    int64_t k = a;
    while (k > lo && colind[k - 1] > c) {
      colind[k] = colind[k - 1];
      tperm[k] = tperm[k - 1];
      --k;
    }
    colind[k] = c;
    tperm[k] = p;
  }
}
__global__ __launch_bounds__(256) void seglen_max_kernel(const int64_t* __restrict__ ptr, int64_t n, unsigned long long* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) atomicMax(out, (unsigned long long)(ptr[i + 1] - ptr[i]));
}

// ---- device buffers, handle cache --------------------------------------------------------------------------------------------------
void csrmap_free(void* p) {
  CsrMap* m = (CsrMap*)p;
  if (m->owned)
    for (void* q : {(void*)m->rowptr, (void*)m->colind, (void*)m->tperm})
      if (q) (void)hipFree(q);
  if (m->valr) (void)hipFree(m->valr);
  delete m;
}
CsrMap* cache_of(const HsHandleView& v) {
  if (!*v.cx) {
    *v.cx = new CsrMap();
    *v.cx_free = csrmap_free;
  }
  return (CsrMap*)*v.cx;
}
int64_t seg_max(const int64_t* ptr, int64_t n, hipStream_t s) {
  HsDevBuf buf("condest workspace");
  unsigned long long* d = buf.get<unsigned long long>(1);
  HS_HIP(hipMemsetAsync(d, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(seglen_max_kernel, dim3(nb256(n)), dim3(256), 0, s, ptr, n, d);
  unsigned long long m = 0;
  HS_HIP(hipMemcpyAsync(&m, d, sizeof m, hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  return (int64_t)m;
}
}  // namespace
namespace hs_ce {
int64_t max_col(const HsHandleView& v, hipStream_t s) {
  CsrMap* m = cache_of(v);
  if (m->maxcol < 0) m->maxcol = seg_max(v.colptr, v.n, s);
  return m->maxcol;
}
// the CSR map (built on first use), its values gathered from the CSC values of the last hs_numeric_begin
template <class T>
CsrMap* csr_of(const HsHandleView& v, hipStream_t s) {
  CsrMap* m = cache_of(v);
  const int64_t n = v.n, nnz = v.nnz;
  if (!m->rowptr) {
    if (v.rowptr) {
      m->rowptr = (int64_t*)v.rowptr;
      m->colind = (int32_t*)v.colind;
      m->tperm = (int64_t*)v.tperm;
      m->owned = false;
    } else {
      int64_t* rp = nullptr;
      int32_t* ci = nullptr;
      int64_t* tp = nullptr;
      HS_HIP(hipMalloc((void**)&rp, sizeof(int64_t) * (size_t)(n + 1)));
      if (hipMalloc((void**)&ci, sizeof(int32_t) * (size_t)std::max<int64_t>(nnz, 1)) != hipSuccess ||
          hipMalloc((void**)&tp, sizeof(int64_t) * (size_t)std::max<int64_t>(nnz, 1)) != hipSuccess) {
        (void)hipFree(rp);
        if (ci) (void)hipFree(ci);
        HS_FAIL(HS_ERR_NOMEM, 0, "hipMalloc of the CSR map of A failed");
      }
      m->rowptr = rp;
      m->colind = ci;
      m->tperm = tp;
      m->owned = true;
      HsDevBuf buf("condest workspace");
      unsigned long long* cur = buf.get<unsigned long long>((size_t)n);
      HS_HIP(hipMemsetAsync(rp, 0, sizeof(int64_t) * (size_t)(n + 1), s));
      hipLaunchKernelGGL(csr_count_kernel, dim3(nb256(nnz)), dim3(256), 0, s, v.rowval, nnz, (unsigned long long*)rp);
      hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, rp, n + 1);
      HS_HIP(hipMemcpyAsync(cur, rp, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToDevice, s));
      hipLaunchKernelGGL(csr_place_kernel, dim3(nb256(n)), dim3(256), 0, s, v.colptr, v.rowval, n, cur, ci, tp);
      hipLaunchKernelGGL(csr_sort_kernel, dim3(nb256(n)), dim3(256), 0, s, (const int64_t*)rp, ci, tp, n);
      HS_HIP(hipStreamSynchronize(s));  // `cur` goes with buf
    }
    m->maxrow = seg_max(m->rowptr, n, s);
  }
  if (!m->valr) {
    void* q = nullptr;
    if (hipMalloc(&q, sizeof(T) * (size_t)std::max<int64_t>(nnz, 1)) != hipSuccess) HS_FAIL(HS_ERR_NOMEM, 0, "hipMalloc of the CSR values of A failed");
    m->valr = q;
  }
  launch_perm_gather<T>((const T*)v.nz, m->tperm, (T*)m->valr, nnz, s);
  return m;
}
template CsrMap* csr_of<double>(const HsHandleView&, hipStream_t);
template CsrMap* csr_of<cplx>(const HsHandleView&, hipStream_t);
}  // namespace hs_ce
namespace {

// ---- solves --------------------------------------------------------------------------------------------------------------------------
// F^-1, F^-T, F^-H (tr = 0, 1, 2) in place on nc columns of leading dimension n
template <class T>
void solve_dev(hs_handle* F, int tr, T* X, int64_t n, int64_t nc, hipStream_t s) {
  HS_CHECK(hs_block_apply_dev<T>(F, HS_VIA_COLS_T, tr, X, n, (const T*)X, n, n, nc, s));
}

// ---- argument checks: refuse, never drop ----------------------------------------------------------------------------------------------
HsHandleView checked_view(hs_handle* F, const char* fn) {
  const HsHandleView v = hs_view_of(F, fn);
  if (!v.device) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: handle holds a host-side plan only (hs_plan)", fn);
  if (v.nranks > 1) HS_FAIL(HS_ERR_UNSUPPORTED, v.nranks, "%s: a factorization over %d ranks is not supported (single-rank factorizations only)", fn, v.nranks);
  return v;
}
void check_factored(const HsHandleView& v, const char* fn) {
  if (!v.factored) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: factorization is not complete", fn);
}
void check_t_solves(const HsHandleView& v, const char* fn, const char* what) {
  if (v.t_refused_node >= 0 && !v.ulv)  // (hs_ulv_mode 1: solve_dev goes through hs_ldiv_ulv_dev_*, which serves N, T and H)
    HS_FAIL(HS_ERR_UNSUPPORTED, v.t_refused_node, "%s: %s needs transposed solves, and node %d keeps its interior block D as an HSS matrix (hs_options.hss_d / mf = 2, 3): "
            "transposed ULV solves are not implemented", fn, what, v.t_refused_node);
}
// hs_ulv_mode 1 on a handle with such fronts: what hs_ldiv_ulv_dev_* refuses is refused before any device work, with its words
void check_ulv_serves(hs_handle* F, const HsHandleView& v) {
  if (!v.ulv) return;
  HS_CHECK(v.is_complex ? hs_block_probe<cplx>(F, HS_VIA_COLS_T, 0) : hs_block_probe<double>(F, HS_VIA_COLS_T, 0));
}
void check_t(const HsHandleView& v, int64_t t, const char* fn) {
  const int64_t tmax = std::min<int64_t>(CE_MAXT, v.n);
  if (t < 1 || t > tmax) HS_FAIL(HS_ERR_ARGUMENT, t, "ArgumentError: %s: t = %lld outside 1:%lld (min(8, n))", fn, (long long)t, (long long)tmax);
}

// ---- drivers -------------------------------------------------------------------------------------------------------------------------
template <class T>
double opnorm_impl(hs_handle* F, const HsHandleView& v, int p, hipStream_t s) {
  HsDevBuf buf("condest workspace");
  const int64_t n = v.n;
  double* sums = buf.get<double>((size_t)n);
  double* part = buf.get<double>((size_t)nbrows(n));
  double* out = buf.get<double>(1);
  if (p == 1) {
    hipLaunchKernelGGL(abssum_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, v.colptr, (const T*)v.nz, n, sums);
  } else {
    CsrMap* m = csr_of<T>(v, s);
    hipLaunchKernelGGL(abssum_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, (const int64_t*)m->rowptr, (const T*)m->valr, n, sums);
  }
  hipLaunchKernelGGL(dmax_part_kernel, dim3(nbrows(n)), dim3(256), 0, s, (const double*)sums, n, part);
  hipLaunchKernelGGL(max_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (int64_t)nbrows(n), out);
  double r = 0.0;
  HS_HIP(hipMemcpyAsync(&r, out, sizeof r, hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  HS_CHECK(hs_handle_flow_check(F));
  return r;
}

template <class T>
double normestinv_impl(hs_handle* F, const HsHandleView& v, int trans, int t, int itmax, int64_t* nsolves, hipStream_t s) {
  HsDevBuf buf("condest workspace");
  HostIo io{F, s};
  EstWork<T, CE_MAXT> ew;
  ew.alloc(buf, v.n, t, 1);
  int64_t ns = 0;
  double est = 0.0;
  est_run(io, ew, v.seed, trans, nullptr, 1, itmax, [&](int tr, T* blk, int64_t nc) {
    solve_dev<T>(F, tr, blk, v.n, nc, s);
    ns += nc;
  }, &est);
  if (nsolves) *nsolves = ns;
  return est;
}

template <class T>
void refine_dev(hs_handle* F, const HsHandleView& v, int trans, T* dX, int64_t ldx, const T* dB, int64_t ldb, int64_t nrhs, int64_t itmax, double* berr,
                double* ferr, int64_t* steps, hipStream_t s) {
  const int64_t n = v.n;
  HsDevBuf buf("condest workspace");
  HostIo io{F, s};
  double* res = buf.get<double>(1);  // the scalar the host reads
  T* r = buf.get<T>((size_t)n);
  T* d = buf.get<T>((size_t)n);
  double* w = buf.get<double>((size_t)n);
  double* wv = buf.get<double>((size_t)n);
  double* part = buf.get<double>((size_t)std::max<int64_t>(nb256(n), (n + 3) / 4));
  const OpRows<T> A = op_rows<T>(v, trans, s);
  const bool wave = A.maxlen > CE_WAVE_ROW;
  const int tr = op_dir<T>(trans).trans;
  EstWork<T, 2> ew;  // ferr: t = min(2, n) columns, 5 iterations, as xGERFS
  if (ferr) ew.alloc(buf, n, (int)std::min<int64_t>(2, n), 1);
  const int64_t npart = wave ? (n + 3) / 4 : (int64_t)nb256(n);
  auto residual = [&](const T* x, const T* b) {
    if (wave) {
      auto k = A.cj ? resid_wave_kernel<T, true> : resid_wave_kernel<T, false>;
      hipLaunchKernelGGL(k, dim3((unsigned)npart), dim3(256), 0, s, A.ptr, A.idx, A.val, x, b, r, w, part, n, A.g);
    } else {
      auto k = A.cj ? resid_kernel<T, true> : resid_kernel<T, false>;
      hipLaunchKernelGGL(k, dim3((unsigned)npart), dim3(256), 0, s, A.ptr, A.idx, A.val, x, b, r, w, part, n, A.g);
    }
    hipLaunchKernelGGL(max_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, npart, res);
  };
  for (int64_t col = 0; col < nrhs; ++col) {
    T* x = dX + col * ldx;
    const T* b = dB + col * ldb;
    HS_HIP(hipMemcpyAsync(x, b, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, s));
    solve_dev<T>(F, tr, x, n, 1, s);
    double lst = 3.0, be = 0.0;
    int64_t cnt = 0;
    for (;;) {
      residual(x, b);
      io.read(res, 1);
      be = io.hd[0];
      if (!(be > CE_EPS && 2.0 * be <= lst && cnt < itmax)) break;
      HS_HIP(hipMemcpyAsync(d, r, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, s));
      solve_dev<T>(F, tr, d, n, 1, s);
      hipLaunchKernelGGL(axpy1_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, x, (const T*)d, n);
      lst = be;
      ++cnt;
    }
    berr[col] = be;
    steps[col] = cnt;
    if (ferr) {
      // || |op(A)^-1| v ||_Inf = || diag(v) op(A)^-H ||_1, estimated on diag(v) op(F)^-H
      hipLaunchKernelGGL(ferr_weights_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, (const T*)r, (const double*)w, wv, n, A.nz * CE_EPS, A.g);
      double est = 0.0;
      est_run(io, ew, v.seed, adj(trans), wv, 1, 5, [&](int dir, T* blk, int64_t nc) { solve_dev<T>(F, dir, blk, n, nc, s); }, &est);
      hipLaunchKernelGGL(absmax_part_kernel<T>, dim3(nbrows(n)), dim3(256), 0, s, (const T*)x, n, part);
      hipLaunchKernelGGL(max_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (int64_t)nbrows(n), res);
      io.read(res, 1);
      const double xn = io.hd[0];
      ferr[col] = xn != 0.0 ? est / xn : est;
    }
  }
  HS_HIP(hipStreamSynchronize(s));
  HS_CHECK(hs_handle_flow_check(F));
}

template <class T>
void refine_entry(hs_handle* F, int trans, T* X, int64_t ldx, const T* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax, double* berr, double* ferr,
                  int64_t* steps, bool on_device, void* stream) {
  const char* fn = on_device ? "hs_ldiv_refine_dev_*" : "hs_ldiv_refine_*";
  const HsHandleView v = checked_view(F, fn);
  check_factored(v, fn);
  check_refine_args<T>(fn, v, trans, X, ldx, B, ldb, n, nrhs, itmax, berr, steps);
  if (trans != 0) check_t_solves(v, fn, "trans != 0");
  if (ferr) check_t_solves(v, fn, "the forward error bound ferr");
  check_ulv_serves(F, v);
  if (nrhs == 0) return;
  if (on_device) {
    check_no_alias<T>(fn, X, ldx, B, ldb, nrhs);
    return refine_dev<T>(F, v, trans, X, ldx, B, ldb, nrhs, itmax, berr, ferr, steps, (hipStream_t)stream);
  }
  hipStream_t s = v.stream;
  HsDevBuf buf("condest workspace");
  T* dX = buf.get<T>((size_t)n * nrhs);
  T* dB = buf.get<T>((size_t)n * nrhs);
  HS_HIP(hipMemcpy2DAsync(dB, sizeof(T) * n, B, sizeof(T) * ldb, sizeof(T) * n, nrhs, hipMemcpyHostToDevice, s));
  refine_dev<T>(F, v, trans, dX, n, dB, n, nrhs, itmax, berr, ferr, steps, s);
  HS_HIP(hipMemcpy2DAsync(X, sizeof(T) * ldx, dX, sizeof(T) * n, sizeof(T) * n, nrhs, hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
extern "C" int hs_opnorm(hs_handle* F, int p, double* norm) {
  HS_GUARD(const HsHandleView v = checked_view(F, "hs_opnorm"); if (p != 0 && p != 1) HS_FAIL(HS_ERR_ARGUMENT, p, "ArgumentError: hs_opnorm: p = %d (1 or 0 = Inf)", p);
           if (!norm) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_opnorm: norm == NULL");
           *norm = v.is_complex ? opnorm_impl<cplx>(F, v, p, v.stream) : opnorm_impl<double>(F, v, p, v.stream));
}

extern "C" int hs_normestinv(hs_handle* F, int trans, int64_t t, int64_t itmax, double* est, int64_t* nsolves, void* stream) {
  HS_GUARD(const HsHandleView v = checked_view(F, "hs_normestinv"); check_factored(v, "hs_normestinv");
           if (trans < 0 || trans > 2) HS_FAIL(HS_ERR_ARGUMENT, trans, "ArgumentError: hs_normestinv: trans = %d (0: F, 1: transpose(F), 2: adjoint(F))", trans);
           check_t(v, t, "hs_normestinv");
           if (itmax < 1 || itmax > CE_MAXIT) HS_FAIL(HS_ERR_ARGUMENT, itmax, "ArgumentError: hs_normestinv: itmax = %lld outside 1:%d", (long long)itmax, CE_MAXIT);
           if (!est) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_normestinv: est == NULL");
           check_t_solves(v, "hs_normestinv", "the estimator"); check_ulv_serves(F, v);
           hipStream_t s = (hipStream_t)stream;
           *est = v.is_complex ? normestinv_impl<cplx>(F, v, trans, (int)t, (int)itmax, nsolves, s) : normestinv_impl<double>(F, v, trans, (int)t, (int)itmax, nsolves, s));
}

extern "C" int hs_condest(hs_handle* F, int p, int64_t t, double* cond, double* normA, double* normFinv, void* stream) {
  HS_GUARD(const HsHandleView v = checked_view(F, "hs_condest"); check_factored(v, "hs_condest");
           if (p != 0 && p != 1) HS_FAIL(HS_ERR_ARGUMENT, p, "ArgumentError: hs_condest: p = %d (1 or 0 = Inf)", p);
           check_t(v, t, "hs_condest"); if (!cond) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_condest: cond == NULL");
           check_t_solves(v, "hs_condest", "the estimator"); check_ulv_serves(F, v);
           hipStream_t s = (hipStream_t)stream;
           const int trans = p == 1 ? 0 : 1;  // ||F^-1||_Inf = ||F^-T||_1
           const double na = v.is_complex ? opnorm_impl<cplx>(F, v, p, s) : opnorm_impl<double>(F, v, p, s);
           const double ne = v.is_complex ? normestinv_impl<cplx>(F, v, trans, (int)t, 5, nullptr, s) : normestinv_impl<double>(F, v, trans, (int)t, 5, nullptr, s);
           *cond = na * ne; if (normA) *normA = na; if (normFinv) *normFinv = ne);
}

extern "C" int hs_ldiv_refine_d(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                double* berr, double* ferr, int64_t* steps) {
  HS_GUARD(refine_entry<double>(F, trans, X, ldx, B, ldb, n, nrhs, itmax, berr, ferr, steps, false, nullptr));
}
extern "C" int hs_ldiv_refine_z(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                double* berr, double* ferr, int64_t* steps) {
  HS_GUARD(refine_entry<cplx>(F, trans, (cplx*)X, ldx, (const cplx*)B, ldb, n, nrhs, itmax, berr, ferr, steps, false, nullptr));
}
extern "C" int hs_ldiv_refine_dev_d(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                    double* berr, double* ferr, int64_t* steps, void* stream) {
  HS_GUARD(refine_entry<double>(F, trans, dX, ldx, dB, ldb, n, nrhs, itmax, berr, ferr, steps, true, stream));
}
extern "C" int hs_ldiv_refine_dev_z(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                    double* berr, double* ferr, int64_t* steps, void* stream) {
  HS_GUARD(refine_entry<cplx>(F, trans, (cplx*)dX, ldx, (const cplx*)dB, ldb, n, nrhs, itmax, berr, ferr, steps, true, stream));
}
