// hs_host.h -- the host side every module's C entry points share: one error family, scoped device workspace, the staging of a host block,
// and the refusals whose text is the same everywhere.  Host code only; include it after hs_solver.h (the HS_ERR_* codes).  A new module
// uses these and writes no macros, buffer holders or try / catch of its own.
//
// Errors travel as a thrown int (the HS_ERR_* code) with the text in hs_last_error: HS_FAIL sets both, HS_GUARD turns them into the
// entry point's return value.  Code that sets the error and RETURNS a status (hs_lowrank*.hip and hs_hss.hip, whose functions are called
// from inside the factorization) is a different contract and does not use this header for it; a caller on this contract passes such a
// status on with HS_CHECK.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <new>
#include <vector>

void hs_set_error(int code, long long info, const char* fmt, ...);
// hs_set_error, then throw (int)code -- out of line (hs_api.hip), so that a refusal costs the code around it one call
[[noreturn]] void hs_fail(int code, long long info, const char* fmt, ...);

#define HS_FAIL(code, info, ...) hs_fail((code), (info), __VA_ARGS__)
#define HS_HIP(call)                                                                                                                \
  do {                                                                                                                              \
    hipError_t e__ = (call);                                                                                                        \
    if (e__ != hipSuccess) HS_FAIL(HS_ERR_DEVICE, 0, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)
// a status some other entry point returned (its message is already set): not HS_OK travels on
#define HS_CHECK(st)             \
  do {                           \
    int s__ = (st);              \
    if (s__ != HS_OK) throw s__; \
  } while (0)
#define HS_GUARD(...)                                        \
  try {                                                      \
    __VA_ARGS__;                                             \
    return HS_OK;                                            \
  } catch (int code) {                                       \
    return code;                                             \
  } catch (const std::bad_alloc&) {                          \
    hs_set_error(HS_ERR_NOMEM, 0, "host allocation failed"); \
    return HS_ERR_NOMEM;                                     \
  }

// ---- scoped device workspace ---------------------------------------------------------------------------------------------------------
// device scratch through the library's arena cache (a parked block of about that size, else hipMalloc with the library's retry); throws on failure
void* hs_scratch_take(size_t bytes, const char* what);
void hs_scratch_give(void* p, size_t bytes);

// Declare an HsDrain AFTER the buffers and events it protects: it then runs first, so nothing in flight on the stream outlives them.
namespace {  // internal linkage: the library exports nothing from here

// hipMalloc blocks, freed on scope exit; `what` names the workspace in the out-of-memory message
struct HsDevBuf {
  const char* what;
  std::vector<void*> p;
  explicit HsDevBuf(const char* what_) : what(what_) {}
  HsDevBuf(const HsDevBuf&) = delete;
  HsDevBuf& operator=(const HsDevBuf&) = delete;
  ~HsDevBuf() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
  template <class U>
  U* get(size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(count * sizeof(U), 256)) != hipSuccess) HS_FAIL(HS_ERR_NOMEM, 0, "hipMalloc of %zu bytes failed (%s)", count * sizeof(U), what);
    p.push_back(q);
    return (U*)q;
  }
};

struct HsScratch {  // one arena scratch block, given back on scope exit
  void* p = nullptr;
  size_t bytes = 0;
  HsScratch() = default;
  HsScratch(size_t b, const char* what) { take(b, what); }
  HsScratch(const HsScratch&) = delete;
  HsScratch& operator=(const HsScratch&) = delete;
  void take(size_t b, const char* what) {
    give();
    p = hs_scratch_take(b, what);
    bytes = b;
  }
  void give() {
    if (p) hs_scratch_give(p, bytes);
    p = nullptr;
    bytes = 0;
  }
  ~HsScratch() { give(); }
};

template <int N>
struct HsEvents {
  hipEvent_t e[N] = {};
  HsEvents() {
    for (int i = 0; i < N; ++i) {
      const hipError_t st = hipEventCreate(&e[i]);
      if (st != hipSuccess) {
        destroy();
        HS_FAIL(HS_ERR_DEVICE, 0, "%s failed: %s (%s:%d)", "hipEventCreate", hipGetErrorString(st), __FILE__, __LINE__);
      }
    }
  }
  HsEvents(const HsEvents&) = delete;
  HsEvents& operator=(const HsEvents&) = delete;
  ~HsEvents() { destroy(); }
  hipEvent_t operator[](int i) const { return e[i]; }

 private:
  void destroy() {
    for (hipEvent_t& x : e) {
      if (x) (void)hipEventDestroy(x);
      x = nullptr;
    }
  }
};

// Waits for the stream on scope exit.  Only where the success path has drained the stream already (there this is a call on an idle stream):
// an entry point that returns with work queued does not hold one.
struct HsDrain {
  hipStream_t s;
  ~HsDrain() { (void)hipStreamSynchronize(s); }
};

// ---- a host block on the device --------------------------------------------------------------------------------------------------------
// The n x nrhs block B goes up into d (ld n), run(d, n, s) works on it in place, and it comes down into C; returns with s drained.
template <class T, class Run>
void hs_stage_block_on(hipStream_t s, T* d, T* C, int64_t ldc, const T* B, int64_t ldb, int64_t n, int64_t nrhs, Run run) {
  HsDrain drain{s};
  HS_HIP(hipMemcpy2DAsync(d, n * sizeof(T), B, ldb * sizeof(T), n * sizeof(T), nrhs, hipMemcpyHostToDevice, s));
  run(d, n, s);
  HS_HIP(hipMemcpy2DAsync(C, ldc * sizeof(T), d, n * sizeof(T), n * sizeof(T), nrhs, hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
}
// the same with d a scratch block of the arena (`what` names it)
template <class T, class Run>
void hs_stage_block(hipStream_t s, const char* what, T* C, int64_t ldc, const T* B, int64_t ldb, int64_t n, int64_t nrhs, Run run) {
  HsScratch d((size_t)n * nrhs * sizeof(T), what);
  hs_stage_block_on<T>(s, (T*)d.p, C, ldc, B, ldb, n, nrhs, run);
}
}  // namespace

// ---- the C entry families over (H* F, trans, C, ldc, B, ldb, n, nrhs[, stream]) ---------------------------------------------------------------
// name##_d / _z on host blocks call host<T>, dname##_d / _z on device blocks call dev<T>
#define HS_LDIV_FAMILY(H, name, dname, host, dev)                                                                                                          \
  extern "C" int name##_d(H* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs) {                          \
    HS_GUARD(host<double>(F, trans, C, ldc, B, ldb, n, nrhs));                                                                                               \
  }                                                                                                                                                          \
  extern "C" int name##_z(H* F, int trans, double* C, int64_t ldc, const double* B, int64_t ldb, int64_t n, int64_t nrhs) {                          \
    HS_GUARD(host<cplx>(F, trans, (cplx*)C, ldc, (const cplx*)B, ldb, n, nrhs));                                                                             \
  }                                                                                                                                                          \
  extern "C" int dname##_d(H* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream) {         \
    HS_GUARD(dev<double>(F, trans, dC, ldc, dB, ldb, n, nrhs, stream));                                                                                      \
  }                                                                                                                                                          \
  extern "C" int dname##_z(H* F, int trans, double* dC, int64_t ldc, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream) {         \
    HS_GUARD(dev<cplx>(F, trans, (cplx*)dC, ldc, (const cplx*)dB, ldb, n, nrhs, stream));                                                                    \
  }

// ---- refusals with one text ------------------------------------------------------------------------------------------------------------
// Only for entry points that say exactly this; a module whose wording differs keeps its own line.
#include "hs_condest.h"  // HsHandleView
inline void hs_check_trans(const char* fn, int trans) {
  if (trans < 0 || trans > 2) HS_FAIL(HS_ERR_ARGUMENT, trans, "ArgumentError: %s: trans = %d (0: F, 1: transpose(F), 2: adjoint(F))", fn, trans);
}
// hs_options.equilibrate: the stored factors are those of A_s = 2^er A 2^ec.  An entry point that reads them directly (not through the
// hs_ldiv_* family, which scales around its sweeps) would answer for A_s: it refuses here, before any device work
int hs_handle_equilibrated(const hs_handle* F);  // hs_api.hip; null: 0
int64_t hs_handle_equil_sum(const hs_handle* F);  // sum er + sum ec of the last hs_numeric_begin (0 without the option)
inline void hs_refuse_equilibrated(const hs_handle* F, const char* fn) {
  if (hs_handle_equilibrated(F))
    HS_FAIL(HS_ERR_UNSUPPORTED, 0,
            "%s: the handle was factored with hs_options.equilibrate, its stored factors are those of the scaled matrix 2^er A 2^ec and this call reads "
            "them directly (the hs_ldiv_* family and the drivers built on it serve such a handle; factor without equilibrate for this call)", fn);
}
inline HsHandleView hs_view_of(hs_handle* F, const char* fn) {
  if (!F) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null factorization handle", fn);
  HsHandleView v;
  hs_handle_view(F, &v);
  return v;
}
