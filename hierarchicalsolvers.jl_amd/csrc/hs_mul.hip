// hs_mul.hip -- the stored factorization applied as an operator (include/hs_solver.h): hs_mul_* / hs_mul_dev_* compute C = op(F) B for a
// block (hs_mul_run, hs_solve_multi.hip: the schedule and its kernels), hs_mul_info reports the last product's figures, and
// hs_factor_error_* measures ||op(A) W - op(F) W||_F / ||op(A) W||_F for a block of probes W on the device: the handle's own A
// (hs_gmres_own_rows) through the SpMM of the GMRES drivers, one hs_mul_run, and the ordered column reduction of hs_eigs_*.
//
// Everything is refused before any device work, with the outputs untouched, in the order hs_ldiv_block_t_* refuses it: a null handle,
// trans, an unfinished or plan-only handle, the element type, the dimensions, more than one rank, HSS interior blocks.
#include <cmath>

#include "../../include/hs_solver.h"
#include "hs_common.h"
#define HS_CONDEST_KERNELS  // the +-1 generator of the estimators (col_key, pm1)
#include "hs_condest.h"
#include "hs_gmres_common.h"  // RowsOf, launch_spmm_op; includes hs_solver.h, hs_common.h, hs_host.h, hs_gmres_op.h
#include "hs_eigs.h"
#include "hs_solve_multi.h"

namespace {

HsHandleView mul_check(hs_handle* F, const char* fn, int trans, bool cplx_call, int64_t n, int64_t ld1, int64_t ld2, int64_t ncols) {
  const HsHandleView v = hs_view_of(F, fn);
  hs_check_trans(fn, trans);
  hs_refuse_equilibrated(F, fn);
  HS_CHECK(hs_handle_flow_check(F));
  if (!v.factored) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: factorization is not complete", fn);
  if ((v.is_complex != 0) != cplx_call) HS_FAIL(HS_ERR_ARGUMENT, 0, "MethodError: %s: eltype of F and B differ", fn);
  if (n != v.n || ld1 < n || ld2 < n || ncols < 0)
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: B has %lld rows, F is %lld x %lld", fn, (long long)n, (long long)v.n, (long long)v.n);
  if (v.nranks > 1) HS_FAIL(HS_ERR_UNSUPPORTED, 0, "%s: products with a factorization over %d ranks are not implemented (single-rank factorizations only)", fn, v.nranks);
  if (v.t_refused_node >= 0)
    HS_FAIL(HS_ERR_UNSUPPORTED, (long long)v.t_refused_node,
            "%s: node %d keeps its interior block D as an HSS matrix (hs_options.hss_d / mf = 2, 3): products with the ULV factors are not implemented", fn, v.t_refused_node);
  return v;
}

template <class T>
void mul_host(hs_handle* F, int trans, T* C, int64_t ldc, const T* B, int64_t ldb, int64_t n, int64_t nrhs) {
  const HsHandleView hv = mul_check(F, "hs_mul_*", trans, sizeof(T) == 16, n, ldc, ldb, nrhs);
  if (nrhs == 0) return;
  if (!C || !B) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_mul_*: null block");
  HsMultiView v;
  hs_multi_view(F, &v);
  hs_stage_block<T>(hv.stream, "hs_mul block", C, ldc, B, ldb, n, nrhs, [&](T* d, int64_t ld, hipStream_t s) { hs_mul_run<T>(v, trans, d, ld, nrhs, s); });
}
template <class T>
void mul_dev(hs_handle* F, int trans, T* dC, int64_t ldc, const T* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream) {
  mul_check(F, "hs_mul_dev_*", trans, sizeof(T) == 16, n, ldc, ldb, nrhs);
  if (nrhs == 0) return;
  if (!dC || !dB) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_mul_dev_*: null block");
  hipStream_t s = (hipStream_t)stream;
  if (dC != dB) HS_HIP(hipMemcpy2DAsync(dC, ldc * sizeof(T), dB, ldb * sizeof(T), n * sizeof(T), nrhs, hipMemcpyDeviceToDevice, s));
  HsMultiView v;
  hs_multi_view(F, &v);
  hs_mul_run<T>(v, trans, dC, ldc, nrhs, s);
}

// W[i, c] = the entry i of the +-1 column col0 + c of draw 0 (hs_condest.h)
template <class T>
__global__ __launch_bounds__(256) void mul_probe_kernel(T* W, int64_t ldw, int64_t n, int64_t seed, int col0) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  W[(size_t)blockIdx.y * ldw + i] = hs_ce::from_real<T>(hs_ce::pm1(hs_ce::col_key(seed, col0 + (int)blockIdx.y, 0), i));
}

#define MUL_FE_COLS 256  // probe columns per pass of hs_factor_error_*

template <class T>
void factor_error(hs_handle* F, int trans, const T* Omega, int64_t ldo, int64_t k, int64_t seed, int where, double* out4) {
  const char* fn = "hs_factor_error_*";
  const HsHandleView hv = mul_check(F, fn, trans, sizeof(T) == 16, hs_view_of(F, fn).n, Omega ? ldo : INT64_MAX, INT64_MAX, 0);
  if (k < 1) HS_FAIL(HS_ERR_ARGUMENT, k, "ArgumentError: %s: k = %lld probe columns (at least 1)", fn, (long long)k);
  if (!out4) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: out4 == NULL", fn);
  if (where != 0 && where != 1) HS_FAIL(HS_ERR_ARGUMENT, where, "ArgumentError: %s: where = %d (0: host pointer, 1: device pointer)", fn, where);
  if (const int st = hs_gmres_own_check(F, fn, 0)) throw st;
  const int64_t n = hv.n;
  gm_check_index_width(n);
  hipStream_t s = hv.stream;
  const int kb = (int)std::min<int64_t>(k, MUL_FE_COLS);
  HsDevBuf buf(fn);
  T* W = buf.get<T>((size_t)n * kb);   // the probes
  T* Y = buf.get<T>((size_t)n * kb);   // op(F) W
  T* R = buf.get<T>((size_t)n * kb);   // op(F) W - op(A) W
  T* AW = buf.get<T>((size_t)n * kb);  // op(A) W
  double* part = buf.get<double>((size_t)hs_eigs_slabs(n) * kb);
  double* d = buf.get<double>((size_t)2 * kb);
  HsEvents<2> ev;
  HsDrain drain{s};
  HsMultiView v;
  hs_multi_view(F, &v);
  const RowsOf<T> A = gm_rows_of_op<T>(buf, F, trans, true, n, nullptr, nullptr, nullptr, s);
  std::vector<double> h((size_t)2 * kb);
  double r2 = 0.0, a2 = 0.0;
  HS_HIP(hipEventRecord(ev[0], s));
  for (int64_t c0 = 0; c0 < k; c0 += kb) {
    const int nc = (int)std::min<int64_t>(kb, k - c0);
    if (Omega)
      HS_HIP(hipMemcpy2DAsync(W, n * sizeof(T), Omega + c0 * ldo, ldo * sizeof(T), n * sizeof(T), nc, where ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    else
      hipLaunchKernelGGL((mul_probe_kernel<T>), dim3((unsigned)((n + 255) / 256), nc), dim3(256), 0, s, W, n, n, seed, (int)c0);
    HS_HIP(hipMemcpyAsync(Y, W, (size_t)n * nc * sizeof(T), hipMemcpyDeviceToDevice, s));
    hs_mul_run<T>(v, trans, Y, n, nc, s);
    launch_spmm_op<T>(A, W, n, nullptr, AW, n, nullptr, 0, nullptr, n, nc, s);
    launch_spmm_op<T>(A, W, n, nullptr, R, n, Y, n, nullptr, n, nc, s);  // R = op(F) W - op(A) W, the fused residual form
    launch_eigs_coldot<T>(R, n, R, n, nullptr, n, nc, part, d, s);
    launch_eigs_coldot<T>(AW, n, AW, n, nullptr, n, nc, part, d + kb, s);
    HS_HIP(hipMemcpyAsync(h.data(), d, sizeof(double) * 2 * kb, hipMemcpyDeviceToHost, s));
    HS_HIP(hipStreamSynchronize(s));
    for (int c = 0; c < nc; ++c) {  // columns in order: one summation order whatever the device did
      r2 += h[c];
      a2 += h[(size_t)kb + c];
    }
  }
  HS_HIP(hipEventRecord(ev[1], s));
  HS_HIP(hipEventSynchronize(ev[1]));
  HS_HIP(hipGetLastError());
  HS_CHECK(hs_handle_flow_check(F));
  float ms = 0.f;
  HS_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  const double rn = std::sqrt(r2), an = std::sqrt(a2);
  out4[0] = an > 0.0 ? rn / an : (rn > 0.0 ? INFINITY : 0.0);
  out4[1] = rn;
  out4[2] = an;
  out4[3] = ms * 1e-3;
}

}  // namespace

HS_LDIV_FAMILY(hs_handle, hs_mul, hs_mul_dev, mul_host, mul_dev)
extern "C" int hs_mul_info(const hs_handle* F, double* out6) {
  HS_GUARD(if (!F || !out6) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_mul_info: null argument"); HsMultiView v; hs_multi_view(const_cast<hs_handle*>(F), &v);
           hs_mul_figures(*v.mx, out6));
}
extern "C" int hs_factor_error_d(hs_handle* F, int trans, const double* Omega, int64_t ldo, int64_t k, int64_t seed, int where, double* out4) {
  HS_GUARD(factor_error<double>(F, trans, Omega, ldo, k, seed, where, out4));
}
extern "C" int hs_factor_error_z(hs_handle* F, int trans, const double* Omega, int64_t ldo, int64_t k, int64_t seed, int where, double* out4) {
  HS_GUARD(factor_error<cplx>(F, trans, (const cplx*)Omega, ldo, k, seed, where, out4));
}
