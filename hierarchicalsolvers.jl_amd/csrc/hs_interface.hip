// hs_interface.hip -- Schur-complement mode: the caller names an interface b (the boundary the root of the tree keeps), the factorization
// eliminates everything else (i), and these entry points hand out what a coupling needs (include/hs_solver.h, hs_interface_*):
//
//   S = A_bb - A_bi A_ii^-1 A_ib          hs_interface_matrix_*    from the pivoted LU P S = L U the handle's pseudo-root keeps
//   g = B_b - A_bi A_ii^-1 B_i            hs_interface_condense_*  the forward sweep of the block solve below the pseudo-root
//   y = S^-1 g                            hs_interface_solve_*     the pseudo-root's own two sweeps
//   x_i = A_ii^-1 (B_i - A_ib y)          hs_interface_expand_*    the backward sweep below the pseudo-root
//
// The object is the reference's: a root that keeps a boundary stores F.S and ldiv! solves with it (factornode.jl:72).  Here it is the
// level-0 front of the handle (hs_api.hip, "pseudo-node"), eliminated last by a pivoted dense LU, so S exists in every such handle as
// L\U and a row permutation.  hs_interface_matrix_* multiplies the two triangles back together (kernels_interface.hip: one launch that walks
// only the k <= min(i, j) part of K); nothing is factored twice and the handle keeps no copy of S.
//
// The three phases are hs_solve_multi_run (hs_solve_multi.hip) with a phase argument: the same chunks of columns, the same work blocks and
// the same launches as hs_ldiv_block_t_*, cut at level 0.  What has to survive between the calls is every front's forward result y, which
// the one-call solve keeps in work block 2: condense copies it into the caller's block at the front's own interior ids (those rows are
// dead between the sweeps -- the forward sweep has consumed them, the backward one overwrites them), expand copies it back.  So the handle
// holds nothing between the calls, any number of blocks may be in flight between condense and expand, and the caller may do what it likes
// with C[idx, :] in between.  The copies are exact: condense; solve; expand leaves the bits of hs_ldiv_block_t_*.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/hs_solver.h"
#include "../../include/hs_kernels.h"
#include "hs_common.h"
#include "hs_host.h"
#include "hs_interface.h"

namespace {

struct InterfaceCache {
  hipEvent_t e0 = nullptr, e1 = nullptr;  // around the last hs_interface_matrix_* launch
  bool pending = false;
  double t_matrix = 0.0, flops = 0.0;
  double t_phase[3] = {0.0, 0.0, 0.0};  // condense, solve, expand
  double chunks = 0.0;
  int open_phase = -1;  // the phase whose seconds are still behind the block solve's events
  ~InterfaceCache() {
    if (e1 && pending) (void)hipEventSynchronize(e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};
void free_cache(void* p) { delete (InterfaceCache*)p; }
InterfaceCache* cache_of(const HsInterfaceView& v) {
  if (!*v.ix) {
    *v.ix = new InterfaceCache();
    *v.ix_free = free_cache;
  }
  return (InterfaceCache*)*v.ix;
}
// the seconds of the last phase call, read from the block solve's events (waits for it)
void close_phase(InterfaceCache* c, void* mx) {
  if (c->open_phase < 0) return;
  double out6[6];
  hs_solve_multi_info(mx, out6);
  c->t_phase[c->open_phase] = out6[0];
  c->chunks = out6[4];
  c->open_phase = -1;
}

// ---- checks: everything here happens before any device work ---------------------------------------------------------------------------
void check_served(const HsInterfaceView& v, const char* fn) {
  if (v.nranks > 1)
    HS_FAIL(HS_ERR_UNSUPPORTED, v.nranks, "%s: interfaces of a factorization over %d ranks are not implemented (single-rank factorizations only)", fn, v.nranks);
  if (v.hss_node >= 0)
    HS_FAIL(HS_ERR_UNSUPPORTED, v.hss_node, "%s: node %d keeps its interior block D as an HSS matrix (hs_options.hss_d / mf = 2, 3): interface solves are not implemented",
            fn, v.hss_node);
}

void check_factored(hs_handle* F, HsInterfaceView& v, bool cplx, const char* fn) {
  if (!F) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null factorization handle", fn);
  hs_interface_view(F, &v);
  hs_refuse_equilibrated(F, fn);
  check_served(v, fn);
  if (!v.device || !v.factored)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s needs a completed numeric factorization (the handle is a plan, or hs_numeric_end has not run)", fn);
  if ((v.is_complex != 0) != cplx) HS_FAIL(HS_ERR_ARGUMENT, 0, "MethodError: %s: eltype of F and of the block differ", fn);
}
template <class T>
void matrix_impl(hs_handle* F, T* S, int64_t lds, int where, void* stream) {
  const char* fn = "hs_interface_matrix_*";
  HsInterfaceView v;
  check_factored(F, v, sizeof(T) == 16, fn);
  if (where < 0 || where > 1) HS_FAIL(HS_ERR_ARGUMENT, where, "ArgumentError: %s: where = %d (0: host, 1: device)", fn, where);
  if (v.flags & HS_IF_SLICED) HS_FAIL(HS_ERR_UNSUPPORTED, 0, "%s: the pseudo-root is eliminated in slices (hs_options.split): it has no single L, U", fn);
  if (v.flags & HS_IF_NOLU) HS_FAIL(HS_ERR_UNSUPPORTED, 0, "%s: the pseudo-root does not keep one dense pivoted LU of the interface block", fn);
  const int64_t nb = v.nb;
  if (nb > 0 && !S) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: S == NULL", fn);
  if (lds < std::max<int64_t>(nb, 1)) HS_FAIL(HS_ERR_DIMENSION, lds, "DimensionMismatch: %s: lds = %lld, S is %lld x %lld", fn, (long long)lds, (long long)nb, (long long)nb);
  InterfaceCache* c = cache_of(v);
  if (c->pending && c->e1) (void)hipEventSynchronize(c->e1);
  c->pending = false;
  c->t_matrix = 0.0;
  c->flops = 0.0;
  if (nb == 0) return;
  if (!c->e0) {
    HS_HIP(hipEventCreate(&c->e0));
    HS_HIP(hipEventCreate(&c->e1));
  }
  hipStream_t s = stream ? (hipStream_t)stream : v.stream;
  if (where == 1) {
    HS_HIP(hipEventRecord(c->e0, s));
    c->flops = launch_lu_product<T>((int)nb, (const T*)v.LU, v.ldlu, v.rperm, S, lds, s);
    HS_HIP(hipEventRecord(c->e1, s));
    HS_HIP(hipGetLastError());
    c->pending = true;
    HS_HIP(hipStreamSynchronize(s));
    return;
  }
  const size_t bytes = (size_t)nb * nb * sizeof(T);
  HsScratch buf(bytes, "interface matrix");
  HsDrain drain{s};
  T* d = (T*)buf.p;
  HS_HIP(hipEventRecord(c->e0, s));
  c->flops = launch_lu_product<T>((int)nb, (const T*)v.LU, v.ldlu, v.rperm, d, nb, s);
  HS_HIP(hipEventRecord(c->e1, s));
  HS_HIP(hipGetLastError());
  c->pending = true;
  HS_HIP(hipMemcpy2DAsync(S, lds * sizeof(T), d, nb * sizeof(T), nb * sizeof(T), nb, hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
}

// phase: HS_MULTI_CONDENSE / ROOT / EXPAND; dev: C is a device block and the call returns without waiting
template <class T>
void phase_impl(hs_handle* F, int phase, int trans, T* C, int64_t ldc, int64_t n, int64_t nrhs, bool dev, void* stream) {
  static const char* names[3] = {"hs_interface_condense_*", "hs_interface_solve_*", "hs_interface_expand_*"};
  const char* fn = names[phase - HS_MULTI_CONDENSE];
  HsInterfaceView v;
  check_factored(F, v, sizeof(T) == 16, fn);
  hs_check_trans(fn, trans);
  if (n != v.n || ldc < n || nrhs < 0)
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: the block has %lld rows (ld %lld, %lld columns), F is %lld x %lld", fn, (long long)n, (long long)ldc,
            (long long)nrhs, (long long)v.n, (long long)v.n);
  if (nrhs > 0 && !C) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null block", fn);
  HS_CHECK(hs_handle_flow_check(F));
  if (nrhs == 0) return;
  HsMultiView mv;
  hs_multi_view(F, &mv);
  InterfaceCache* c = cache_of(v);
  close_phase(c, *mv.mx);
  if (dev) {
    hs_solve_multi_run<T>(mv, trans, C, ldc, nrhs, (hipStream_t)stream, nullptr, phase);
    c->open_phase = phase - HS_MULTI_CONDENSE;
    return;
  }
  hs_stage_block<T>(v.stream, "interface block", C, ldc, (const T*)C, ldc, n, nrhs, [&](T* d, int64_t ld, hipStream_t s) {
    hs_solve_multi_run<T>(mv, trans, d, ld, nrhs, s, nullptr, phase);
    c->open_phase = phase - HS_MULTI_CONDENSE;
  });
  close_phase(c, *mv.mx);
}
}  // namespace

extern "C" int hs_interface_size(const hs_handle* F, int64_t* nb) {
  HS_GUARD(if (!F || !nb) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_interface_size: null %s", F ? "output" : "factorization handle");
           HsInterfaceView v; hs_interface_view(const_cast<hs_handle*>(F), &v);
           *nb = v.nb);
}
extern "C" int hs_interface_indices(const hs_handle* F, int64_t* idx) {
  HS_GUARD(if (!F) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_interface_indices: null factorization handle");
           HsInterfaceView v; hs_interface_view(const_cast<hs_handle*>(F), &v);
           if (v.nb > 0 && !idx) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_interface_indices: idx == NULL");
           for (int64_t i = 0; i < v.nb; ++i) idx[i] = (int64_t)v.idx[i] + 1);
}
extern "C" int hs_interface_matrix_d(hs_handle* F, double* S, int64_t lds, int where, void* stream) { HS_GUARD(matrix_impl<double>(F, S, lds, where, stream)); }
extern "C" int hs_interface_matrix_z(hs_handle* F, double* S, int64_t lds, int where, void* stream) { HS_GUARD(matrix_impl<cplx>(F, (cplx*)S, lds, where, stream)); }

#define IF_PHASE(name, phase)                                                                                                                   \
  extern "C" int hs_interface_##name##_d(hs_handle* F, int trans, double* C, int64_t ldc, int64_t n, int64_t nrhs) {                            \
    HS_GUARD(phase_impl<double>(F, phase, trans, C, ldc, n, nrhs, false, nullptr));                                                             \
  }                                                                                                                                             \
  extern "C" int hs_interface_##name##_z(hs_handle* F, int trans, double* C, int64_t ldc, int64_t n, int64_t nrhs) {                            \
    HS_GUARD(phase_impl<cplx>(F, phase, trans, (cplx*)C, ldc, n, nrhs, false, nullptr));                                                        \
  }                                                                                                                                             \
  extern "C" int hs_interface_##name##_dev_d(hs_handle* F, int trans, double* dC, int64_t ldc, int64_t n, int64_t nrhs, void* stream) {         \
    HS_GUARD(phase_impl<double>(F, phase, trans, dC, ldc, n, nrhs, true, stream));                                                              \
  }                                                                                                                                             \
  extern "C" int hs_interface_##name##_dev_z(hs_handle* F, int trans, double* dC, int64_t ldc, int64_t n, int64_t nrhs, void* stream) {         \
    HS_GUARD(phase_impl<cplx>(F, phase, trans, (cplx*)dC, ldc, n, nrhs, true, stream));                                                         \
  }
IF_PHASE(condense, HS_MULTI_CONDENSE)
IF_PHASE(solve, HS_MULTI_ROOT)
IF_PHASE(expand, HS_MULTI_EXPAND)

extern "C" int hs_interface_info(const hs_handle* F, double* out8) {
  HS_GUARD(if (!F || !out8) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_interface_info: null %s", F ? "output" : "factorization handle");
           HsInterfaceView v; hs_interface_view(const_cast<hs_handle*>(F), &v);
           for (int k = 0; k < 8; ++k) out8[k] = 0.0;
           out8[2] = (double)v.nb;
           InterfaceCache* c = (InterfaceCache*)*v.ix;
           if (!c) return HS_OK;
           if (c->pending) {
             float ms = 0.f;
             if (hipEventSynchronize(c->e1) == hipSuccess && hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) c->t_matrix = ms * 1e-3;
             c->pending = false;
           }
           if (c->open_phase >= 0) {
             HsMultiView mv; hs_multi_view(const_cast<hs_handle*>(F), &mv);
             close_phase(c, *mv.mx);
           }
           out8[0] = c->t_matrix; out8[1] = c->flops;
           out8[3] = c->t_phase[0]; out8[4] = c->t_phase[1]; out8[5] = c->t_phase[2];
           out8[6] = c->chunks);
}
