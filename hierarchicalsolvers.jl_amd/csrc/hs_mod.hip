// hs_mod.hip -- solves with A1 = A + U V^H from the stored factorization of A (hs_mod_*; include/hs_solver.h), by the
// Sherman-Morrison-Woodbury identity.  With Z = F^-1 U, W = F^-H V and C = I_k + V^H Z:
//
//   trans 0:  A1^-1 B = Y - Z C^-1 (V^H Y),            Y = F^-1 B
//   trans 2:  A1^-H B = Y - W C^-H (U^H Y),            Y = F^-H B
//   trans 1:  A1^-T B = Y - conj(W) C^-T (U^T Y),      Y = F^-T B
//
// Every solve with F is one of the library's own entry points (hs_ldiv_block_dev_t_*, hs_ldiv_sparse_dev_* with all rows), so Y carries the
// bits of those calls; the three pieces around them are kernels_mod.hip (hs_mod.h), each with one summation order per element.  The object
// owns copies of U, V (or the column list J of an entry modification), Z, LU(C), the partial sums of the inner product and the k x KC
// intermediate; W -- one block for both transposed forms -- is built by the first call that needs it.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/hs_solver.h"
#include "hs_common.h"
#include "hs_host.h"
#pragma clang fp contract(off)  // host arithmetic only (no kernel lives here): the plain products and sums
#include "hs_solve_multi.h"  // hs_ldiv_block_cols
#include "hs_mod.h"

struct hs_mod {
  hs_handle* F = nullptr;
  int cx = 0;
  int64_t n = 0;
  int k = 0;
  bool sparse = false;  // V = I[:, J]
  void *dU = nullptr, *dV = nullptr, *dZ = nullptr, *dW = nullptr, *dLU = nullptr, *dT = nullptr, *dPart = nullptr, *dUval = nullptr;
  int64_t* dJ = nullptr;  // 0-based
  int *dPiv = nullptr, *dInfo = nullptr;
  std::vector<int64_t> ucp, urv, J;  // the sparse form: U = dA[:, J] as 1-based CSC (host), J 1-based
  std::vector<void*> owned;
  size_t bytes = 0;
  double rcond = 1.0, t_build = 0.0, t_solve = 0.0;
  int64_t solves = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool pending = false;
  hipStream_t last = nullptr;  // the stream of the last solve
  ~hs_mod() {
    if (pending && e1) (void)hipEventSynchronize(e1);
    for (void* p : owned) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  template <class U_>
  U_* take(size_t count) {
    void* p = nullptr;
    const size_t b = std::max<size_t>(count * sizeof(U_), 256);
    if (hipMalloc(&p, b) != hipSuccess) HS_FAIL(HS_ERR_NOMEM, 0, "OutOfMemoryError: hs_mod_*: hipMalloc of %zu bytes failed", b);
    owned.push_back(p);
    bytes += b;
    return (U_*)p;
  }
};

namespace {

template <class T>
int block_solve(hs_handle* F, int t, T* C, int64_t ldc, const T* B, int64_t ldb, int64_t n, int64_t nc, hipStream_t s) {
  if (sizeof(T) == 16) return hs_ldiv_block_dev_t_z(F, t, (double*)C, ldc, (const double*)B, ldb, n, nc, (void*)s);
  return hs_ldiv_block_dev_t_d(F, t, (double*)C, ldc, (const double*)B, ldb, n, nc, (void*)s);
}
template <class T>
int sparse_solve(hs_handle* F, int t, int64_t n, int64_t nc, const int64_t* cp, const int64_t* rv, const T* dv, T* X, int64_t ldx, hipStream_t s) {
  if (sizeof(T) == 16) return hs_ldiv_sparse_dev_z(F, t, n, nc, cp, rv, (const double*)dv, nullptr, 0, (double*)X, ldx, (void*)s);
  return hs_ldiv_sparse_dev_d(F, t, n, nc, cp, rv, (const double*)dv, nullptr, 0, (double*)X, ldx, (void*)s);
}

inline double abs_h(double a) { return std::fabs(a); }
inline double abs_h(cplx a) { return std::hypot(a.re, a.im); }
template <class T>
double norm1_host(const std::vector<T>& A, int k) {
  double best = 0.0;
  for (int j = 0; j < k; ++j) {
    double s = 0.0;
    for (int i = 0; i < k; ++i) s += abs_h(A[(size_t)j * k + i]);
    best = std::max(best, s);
  }
  return best;
}

// what every create refuses of the handle and the sizes; the zero-column solve speaks for the block solve
template <class T>
HsHandleView check_create(const char* fn, hs_handle* F, int64_t n, int64_t k, hs_mod** out) {
  if (!out) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: M == NULL", fn);
  *out = nullptr;
  HsHandleView v = hs_view_of(F, fn);
  if ((v.is_complex != 0) != (sizeof(T) == 16)) HS_FAIL(HS_ERR_ARGUMENT, 0, "MethodError: %s: eltype of F and of the modification differ", fn);
  if (!v.device) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: handle holds a host-side plan only (hs_plan); use hs_analyze", fn);
  if (!v.factored) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: handle holds no numeric factorization", fn);
  if (n != v.n || k < 0) HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: the modification has %lld rows and rank %lld, F is %lld x %lld", fn, (long long)n, (long long)k, (long long)v.n, (long long)v.n);
  if (k > HS_MOD_MAXRANK)
    HS_FAIL(HS_ERR_UNSUPPORTED, k, "%s: rank %lld > HS_MOD_MAXRANK = %d: a modification of this rank is not applied through the capacitance matrix; refactor (hs_factor_*)", fn,
            (long long)k, HS_MOD_MAXRANK);
  HS_CHECK(block_solve<T>(F, 0, nullptr, n, nullptr, n, n, 0, v.stream));
  return v;
}

template <class T>
void common_buffers(hs_mod* M) {
  const int k = M->k;
  const int KC = hs_ldiv_block_cols();
  M->dZ = M->take<T>((size_t)M->n * k);
  M->dLU = M->take<T>((size_t)k * k);
  M->dT = M->take<T>((size_t)k * KC);
  M->dPiv = M->take<int>((size_t)k);
  M->dInfo = M->take<int>(1);
  HS_HIP(hipEventCreate(&M->e0));
  HS_HIP(hipEventCreate(&M->e1));
}

// C (k x k in dLU, before its identity) -> LU(C), rcond_1(C); waits for s
template <class T>
void factor_cap(const char* fn, hs_mod* M, hipStream_t s) {
  const int k = M->k;
  T* C = (T*)M->dLU;
  launch_mod_add_eye<T>(C, k, k, s);
  std::vector<T> hC((size_t)k * k), hI((size_t)k * k);
  HS_HIP(hipMemcpyAsync(hC.data(), C, hC.size() * sizeof(T), hipMemcpyDeviceToHost, s));
  launch_mod_cap_lu<T>(C, k, k, M->dPiv, M->dInfo, s);
  int info = 0;
  HS_HIP(hipMemcpyAsync(&info, M->dInfo, sizeof(int), hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  HS_HIP(hipGetLastError());
  if (info != 0)
    HS_FAIL(HS_ERR_SINGULAR, info, "SingularException(%d): %s: the capacitance matrix I + V^H F^-1 U is singular (A + U V^H is, if A is not)", info, fn);
  HsDevBuf tmp("condest workspace");
  T* dI = tmp.get<T>((size_t)k * k);
  std::vector<T> eye((size_t)k * k, Scal<T>::zero());
  for (int j = 0; j < k; ++j) eye[(size_t)j * k + j] = Scal<T>::one();
  HS_HIP(hipMemcpyAsync(dI, eye.data(), eye.size() * sizeof(T), hipMemcpyHostToDevice, s));
  launch_mod_cap_solve<T>(C, k, k, M->dPiv, 0, dI, k, k, s);
  HS_HIP(hipMemcpyAsync(hI.data(), dI, hI.size() * sizeof(T), hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  const double a = norm1_host(hC, k), b = norm1_host(hI, k);
  M->rcond = (a > 0.0 && b > 0.0 && std::isfinite(a) && std::isfinite(b)) ? 1.0 / (a * b) : 0.0;
}

// dU, dV hold the blocks (n x k, ld n): Z, C, LU(C)
template <class T>
void build_dense(const char* fn, hs_mod* M, hipStream_t s) {
  const int k = M->k;
  const int64_t n = M->n;
  if (k == 0) return;
  const int KC = hs_ldiv_block_cols();
  M->dPart = M->take<T>((size_t)hs_mod_slabs(n) * k * KC);
  HS_CHECK(block_solve<T>(M->F, 0, (T*)M->dZ, n, (const T*)M->dU, n, n, k, s));
  ++M->solves;
  for (int c0 = 0; c0 < k; c0 += KC) {
    const int mc = std::min(KC, k - c0);
    launch_mod_inner<T>((const T*)M->dV, n, (const T*)M->dZ + (size_t)c0 * n, n, n, k, mc, 0, (T*)M->dPart, (T*)M->dLU + (size_t)c0 * k, k, s);
  }
  factor_cap<T>(fn, M, s);
}

template <class T>
void create_dense(hs_handle* F, int64_t n, int64_t k, const T* U, int64_t ldu, const T* V, int64_t ldv, bool on_device, void* stream, hs_mod** out) {
  const char* fn = on_device ? "hs_mod_create_dev_*" : "hs_mod_create_*";
  const HsHandleView v = check_create<T>(fn, F, n, k, out);
  if (k > 0 && (!U || !V)) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: U and V must not be NULL", fn);
  if (k > 0 && (ldu < n || ldv < n)) HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: ldu = %lld, ldv = %lld, n = %lld", fn, (long long)ldu, (long long)ldv, (long long)n);
  const auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<hs_mod> M(new hs_mod());
  M->F = F;
  M->cx = sizeof(T) == 16;
  M->n = n;
  M->k = (int)k;
  hipStream_t s = on_device ? (hipStream_t)stream : v.stream;
  common_buffers<T>(M.get());
  if (k > 0) {
    M->dU = M->take<T>((size_t)n * k);
    M->dV = M->take<T>((size_t)n * k);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HS_HIP(hipMemcpy2DAsync(M->dU, n * sizeof(T), U, ldu * sizeof(T), n * sizeof(T), k, kind, s));
    HS_HIP(hipMemcpy2DAsync(M->dV, n * sizeof(T), V, ldv * sizeof(T), n * sizeof(T), k, kind, s));
    if (!on_device) HS_HIP(hipStreamSynchronize(s));  // the host blocks may go once the call returns
    build_dense<T>(fn, M.get(), s);
  }
  M->t_build = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out = M.release();
}

template <class T>
void create_sparse(hs_handle* F, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nzval, hs_mod** out) {
  const char* fn = "hs_mod_create_sparse_*";
  if (out) *out = nullptr;
  if (!colptr) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: colptr == NULL", fn);
  if (n < 0) HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: n = %lld", fn, (long long)n);
  if (colptr[0] != 1) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: colptr must be 1-based (SparseMatrixCSC)", fn);
  int64_t k = 0;
  for (int64_t j = 0; j < n; ++j) {
    if (colptr[j + 1] < colptr[j] || colptr[j + 1] - colptr[j] > n) HS_FAIL(HS_ERR_ARGUMENT, j, "ArgumentError: %s: colptr is inconsistent at column %lld", fn, (long long)j + 1);
    if (colptr[j + 1] > colptr[j]) ++k;
  }
  const int64_t nnz = colptr[n] - 1;
  if (nnz > 0 && (!rowval || !nzval)) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: rowval and nzval must not be NULL", fn);
  for (int64_t j = 0; j < n; ++j)
    for (int64_t e = colptr[j] - 1; e < colptr[j + 1] - 1; ++e) {
      if (rowval[e] < 1 || rowval[e] > n) HS_FAIL(HS_ERR_DIMENSION, e, "BoundsError: %s: rowval[%lld] = %lld outside 1:%lld", fn, (long long)e + 1, (long long)rowval[e], (long long)n);
      if (e > colptr[j] - 1 && rowval[e] <= rowval[e - 1])
        HS_FAIL(HS_ERR_ARGUMENT, e, "ArgumentError: %s: the rows of column %lld of dA are not strictly increasing", fn, (long long)j + 1);
    }
  const HsHandleView v = check_create<T>(fn, F, n, k, out);
  const auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<hs_mod> M(new hs_mod());
  M->F = F;
  M->cx = sizeof(T) == 16;
  M->n = n;
  M->k = (int)k;
  M->sparse = true;
  hipStream_t s = v.stream;
  common_buffers<T>(M.get());
  if (k > 0) {
    M->ucp.push_back(1);
    std::vector<int64_t> j0;
    for (int64_t j = 0; j < n; ++j)
      if (colptr[j + 1] > colptr[j]) {
        M->J.push_back(j + 1);
        j0.push_back(j);
        M->ucp.push_back(colptr[j + 1]);  // the nonempty columns are consecutive in the arrays: no rebasing of the entries
      }
    M->urv.assign(rowval, rowval + nnz);
    M->dUval = M->take<T>((size_t)nnz);
    M->dJ = M->take<int64_t>((size_t)k);
    HS_HIP(hipMemcpyAsync(M->dUval, nzval, (size_t)nnz * sizeof(T), hipMemcpyHostToDevice, s));
    HS_HIP(hipMemcpyAsync(M->dJ, j0.data(), (size_t)k * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HS_HIP(hipStreamSynchronize(s));
    HS_CHECK(sparse_solve<T>(F, 0, n, k, M->ucp.data(), M->urv.data(), (const T*)M->dUval, (T*)M->dZ, n, s));
    ++M->solves;
    launch_mod_gather<T>((T*)M->dLU, k, (const T*)M->dZ, n, M->dJ, (int)k, (int)k, s);
    factor_cap<T>(fn, M.get(), s);
  }
  M->t_build = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out = M.release();
}

// W = F^-H V, and for the sparse form the dense U the transposed inner products read
template <class T>
void build_w_blocks(hs_mod* M, hipStream_t s);
// the blocks become the object's only when every solve has succeeded: after a failure they are released, so that a later call starts over
template <class T>
void build_w(hs_mod* M, hipStream_t s) {
  const size_t owned0 = M->owned.size(), bytes0 = M->bytes;
  try {
    build_w_blocks<T>(M, s);
  } catch (...) {
    (void)hipStreamSynchronize(s);
    while (M->owned.size() > owned0) {
      (void)hipFree(M->owned.back());
      M->owned.pop_back();
    }
    M->bytes = bytes0;
    throw;
  }
}
template <class T>
void build_w_blocks(hs_mod* M, hipStream_t s) {
  const int k = M->k;
  const int64_t n = M->n;
  T* W = M->take<T>((size_t)n * k);
  if (!M->sparse) {
    HS_CHECK(block_solve<T>(M->F, 2, W, n, (const T*)M->dV, n, n, k, s));
  } else {
    const int64_t nnz = (int64_t)M->urv.size();
    std::vector<T> ones((size_t)k, Scal<T>::one());
    std::vector<int64_t> cp((size_t)k + 1);
    for (int j = 0; j <= k; ++j) cp[(size_t)j] = j + 1;
    std::vector<int32_t> er((size_t)nnz), ec((size_t)nnz);
    for (int j = 0; j < k; ++j)
      for (int64_t e = M->ucp[(size_t)j] - 1; e < M->ucp[(size_t)j + 1] - 1; ++e) {
        er[(size_t)e] = (int32_t)(M->urv[(size_t)e] - 1);
        ec[(size_t)e] = j;
      }
    HsDevBuf tmp("condest workspace");
    T* d1 = tmp.get<T>((size_t)k);
    int32_t* der = tmp.get<int32_t>((size_t)nnz);
    int32_t* dec = tmp.get<int32_t>((size_t)nnz);
    HS_HIP(hipMemcpyAsync(d1, ones.data(), (size_t)k * sizeof(T), hipMemcpyHostToDevice, s));
    HS_HIP(hipMemcpyAsync(der, er.data(), (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HS_HIP(hipMemcpyAsync(dec, ec.data(), (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, s));
    T* U = M->take<T>((size_t)n * k);
    T* part = M->take<T>((size_t)hs_mod_slabs(n) * k * hs_ldiv_block_cols());
    HS_HIP(hipMemsetAsync(U, 0, (size_t)n * k * sizeof(T), s));
    launch_mod_scatter<T>(U, n, der, dec, (const T*)M->dUval, nnz, s);
    HS_HIP(hipStreamSynchronize(s));
    HS_CHECK(sparse_solve<T>(M->F, 2, n, k, cp.data(), M->J.data(), d1, W, n, s));  // waits for s
    M->dU = U;
    M->dPart = part;
  }
  ++M->solves;
  M->dW = W;
}

template <class T>
void check_ldiv(const char* fn, hs_mod* M, int trans, int64_t ldc, int64_t ldb, int64_t n, int64_t nrhs) {
  if (!M) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null hs_mod", fn);
  if ((M->cx != 0) != (sizeof(T) == 16)) HS_FAIL(HS_ERR_ARGUMENT, 0, "MethodError: %s: eltype of M and B differ", fn);
  if (trans < 0 || trans > 2) HS_FAIL(HS_ERR_ARGUMENT, trans, "ArgumentError: %s: trans = %d (0: A1, 1: transpose(A1), 2: adjoint(A1))", fn, trans);
  if (n != M->n || nrhs < 0 || ldc < n || ldb < n)
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: B has %lld rows (ldc %lld, ldb %lld, nrhs %lld), A1 is %lld x %lld", fn, (long long)n, (long long)ldc, (long long)ldb,
            (long long)nrhs, (long long)M->n, (long long)M->n);
}

// dC = op(A1)^-1 dB, queued on s
template <class T>
void ldiv_core(hs_mod* M, int trans, T* dC, int64_t ldc, const T* dB, int64_t ldb, int64_t nrhs, hipStream_t s) {
  const int k = M->k;
  const int64_t n = M->n;
  const int KC = hs_ldiv_block_cols();
  // the intermediates (dT, dPart) are reused: a call queued on the same stream is ordered behind the last one by the stream, one on another
  // stream waits for it on the device
  if (M->pending && s != M->last) HS_HIP(hipStreamWaitEvent(s, M->e1, 0));
  M->last = s;
  if (trans != 0 && k > 0 && !M->dW) build_w<T>(M, s);
  HS_HIP(hipEventRecord(M->e0, s));
  for (int64_t c0 = 0; c0 < nrhs; c0 += KC) {
    const int kc = (int)std::min<int64_t>(KC, nrhs - c0);
    T* Y = dC + (size_t)c0 * ldc;
    HS_CHECK(block_solve<T>(M->F, trans, Y, ldc, dB + (size_t)c0 * ldb, ldb, n, kc, s));
    ++M->solves;
    if (k == 0) continue;
    T* Tm = (T*)M->dT;
    if (trans == 0 && M->sparse)
      launch_mod_gather<T>(Tm, k, Y, ldc, M->dJ, k, kc, s);
    else
      launch_mod_inner<T>((const T*)(trans == 0 ? M->dV : M->dU), n, Y, ldc, n, k, kc, trans == 1, (T*)M->dPart, Tm, k, s);
    launch_mod_cap_solve<T>((const T*)M->dLU, k, k, M->dPiv, trans, Tm, k, kc, s);
    launch_mod_apply<T>(Y, ldc, (const T*)(trans == 0 ? M->dZ : M->dW), n, Tm, k, n, k, kc, trans == 1, s);
  }
  HS_HIP(hipEventRecord(M->e1, s));
  HS_HIP(hipGetLastError());
  M->pending = true;
}

template <class T>
void ldiv_dev(hs_mod* M, int trans, T* dC, int64_t ldc, const T* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream) {
  const char* fn = "hs_mod_ldiv_dev_*";
  check_ldiv<T>(fn, M, trans, ldc, ldb, n, nrhs);
  if (nrhs == 0) return;
  if (!dC || !dB) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null block", fn);
  ldiv_core<T>(M, trans, dC, ldc, dB, ldb, nrhs, (hipStream_t)stream);
}

template <class T>
void ldiv_host(hs_mod* M, int trans, T* C, int64_t ldc, const T* B, int64_t ldb, int64_t n, int64_t nrhs) {
  const char* fn = "hs_mod_ldiv_*";
  check_ldiv<T>(fn, M, trans, ldc, ldb, n, nrhs);
  if (nrhs == 0) return;
  if (!C || !B) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null block", fn);
  HsHandleView v;
  hs_handle_view(M->F, &v);
  HsDevBuf tmp("condest workspace");
  hs_stage_block_on<T>(v.stream, tmp.get<T>((size_t)n * nrhs), C, ldc, B, ldb, n, nrhs, [&](T* d, int64_t ld, hipStream_t s) { ldiv_core<T>(M, trans, d, ld, d, ld, nrhs, s); });
}

}  // namespace

// hs_gmres_block.hip: the preconditioner call of hs_gmres_block_mod_*
int hs_mod_apply_prec(hs_mod* M, int trans, void* dC, int64_t ldc, const void* dB, int64_t ldb, int64_t n, int64_t nrhs, hipStream_t s) {
  if (M && M->cx) return hs_mod_ldiv_dev_z(M, trans, (double*)dC, ldc, (const double*)dB, ldb, n, nrhs, (void*)s);
  return hs_mod_ldiv_dev_d(M, trans, (double*)dC, ldc, (const double*)dB, ldb, n, nrhs, (void*)s);
}
hs_handle* hs_mod_handle(hs_mod* M) { return M ? M->F : nullptr; }

extern "C" int hs_mod_create_d(hs_handle* F, int64_t n, int64_t k, const double* U, int64_t ldu, const double* V, int64_t ldv, hs_mod** M) {
  HS_GUARD(create_dense<double>(F, n, k, U, ldu, V, ldv, false, nullptr, M));
}
extern "C" int hs_mod_create_z(hs_handle* F, int64_t n, int64_t k, const double* U, int64_t ldu, const double* V, int64_t ldv, hs_mod** M) {
  HS_GUARD(create_dense<cplx>(F, n, k, (const cplx*)U, ldu, (const cplx*)V, ldv, false, nullptr, M));
}
extern "C" int hs_mod_create_dev_d(hs_handle* F, int64_t n, int64_t k, const double* dU, int64_t ldu, const double* dV, int64_t ldv, void* stream, hs_mod** M) {
  HS_GUARD(create_dense<double>(F, n, k, dU, ldu, dV, ldv, true, stream, M));
}
extern "C" int hs_mod_create_dev_z(hs_handle* F, int64_t n, int64_t k, const double* dU, int64_t ldu, const double* dV, int64_t ldv, void* stream, hs_mod** M) {
  HS_GUARD(create_dense<cplx>(F, n, k, (const cplx*)dU, ldu, (const cplx*)dV, ldv, true, stream, M));
}
extern "C" int hs_mod_create_sparse_d(hs_handle* F, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, hs_mod** M) {
  HS_GUARD(create_sparse<double>(F, n, colptr, rowval, nzval, M));
}
extern "C" int hs_mod_create_sparse_z(hs_handle* F, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, hs_mod** M) {
  HS_GUARD(create_sparse<cplx>(F, n, colptr, rowval, (const cplx*)nzval, M));
}
HS_LDIV_FAMILY(hs_mod, hs_mod_ldiv, hs_mod_ldiv_dev, ldiv_host, ldiv_dev)
extern "C" int hs_mod_info(hs_mod* M, double* out8) {
  if (!M || !out8) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_mod_info: null argument");
    return HS_ERR_ARGUMENT;
  }
  if (M->pending) {
    float ms = 0.f;
    if (hipEventSynchronize(M->e1) == hipSuccess && hipEventElapsedTime(&ms, M->e0, M->e1) == hipSuccess) M->t_solve = ms * 1e-3;
    M->pending = false;
  }
  out8[0] = (double)M->k;
  out8[1] = M->rcond;
  out8[2] = M->t_build;
  out8[3] = M->t_solve;
  out8[4] = (double)M->bytes;
  out8[5] = M->dW ? 1.0 : 0.0;
  out8[6] = (double)M->solves;
  out8[7] = 0.0;
  return HS_OK;
}
extern "C" void hs_mod_free(hs_mod* M) { delete M; }
