// hs_sens.hip -- adjoint-state sensitivities on A's pattern for a block of sources (hs_sens_*, hs_misfit_*; include/hs_solver.h).
//
// With X = op(A)^-1 B and the cotangent W of a real objective (dJ = Re<W, dX>), Lam = op(A)^-H W and
//
//   trans 0:  Lam = adjoint(F) \ W          G_ij = -sum_c Lam_ic conj(X_jc)
//   trans 1:  Lam = conj(F \ conj(W))       G_ij = -sum_c Lam_jc conj(X_ic)
//   trans 2:  Lam = F \ W                   G_ij = -sum_c conj(Lam_jc) X_ic        for every stored entry (i, j) of A,
//
// so that d/ds Re<W, op(A + sE)^-1 B> at s = 0 equals Re sum_p E_p conj(G_p) for any E on A's pattern.
//
// The columns are processed in groups of Gc.  Per group the forward solve writes the X block, the adjoint solve the Lam block, and the
// reduction kernel (kernels_sens.hip) continues the chain of every stored entry of A; neither block leaves the device unless the caller
// asked for it.  Every solve is one of the library's own entry points -- hs_ldiv_block_dev_t_* (dense blocks), hs_ldiv_sparse_dev_* with all
// rows (sparse blocks: the pruned forward sweep), hs_ldiv_refine_block_dev_* (itmax > 0; a sparse block is expanded on the device first) --
// so X and Lam carry the bits of those calls, which do not depend on the group width; the chain of an entry takes the columns in order, so
// G does not either.  For ComplexF64 with trans = 1 the solve runs on conj(W) and gives M = conj(Lam): the conjugation of W is folded into
// the copy (dense), the staged values (sparse) or the misfit kernel, and the one of M into the kernel's flag; Lam itself is formed only in
// the caller's copy.
//
// The misfit form builds W on the device: R = X[rows, :] - D, J_c = 0.5 ||R[:, c]||^2, W = scatter(R) -- a sparse block with nrows stored
// rows per column (ascending), which takes the pruned path when itmax = 0.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/hs_solver.h"
#include "hs_common.h"
#include "hs_host.h"
#include "hs_block_apply.h"
#pragma clang fp contract(off)  // host arithmetic only (no kernel lives here): the plain products and sums
#include "hs_solve_multi.h"  // hs_ldiv_block_cols
#include "hs_sens.h"
#include "hs_sens_solve.h"

namespace {

enum { SI_SECONDS = 0, SI_FORWARD, SI_ADJOINT, SI_REDUCE, SI_GROUPS, SI_PRODUCTS, SI_MOVED, SI_WORK_BYTES };

template <class T>
struct Call {
  hs_handle* F = nullptr;
  HsHandleView v;
  int trans = 0, pattern = 0;
  int64_t n = 0, nrhs = 0, itmax = 0;
  Blk<T> B, W;
  bool misfit = false;
  const int64_t* rows = nullptr;  // 1-based, distinct
  int64_t nrows = 0;
  const T* dD = nullptr;
  int64_t ldd = 0;
  T* dG = nullptr;
  T* dX = nullptr;
  int64_t ldx = 0;
  T* dLam = nullptr;
  int64_t ldl = 0;
  double* dJ = nullptr;
  T* dR = nullptr;
  int64_t ldr = 0;
  hipStream_t s = nullptr;
};

template <class T>
struct Driver {
  const Call<T>& c;
  HsDevBuf& buf;
  int64_t n, Gc = 0;
  T* Xg = nullptr;      // n x Gc
  T* Lg = nullptr;      // n x Gc: Lam, or M = conj(Lam) (ComplexF64, trans = 1)
  int32_t* ecol = nullptr;  // the column of every stored entry of A
  HsGroupSolve<T> gs;       // the solve of one group, with its staging (hs_sens_solve.h)
  HsReceiverRows<T> rr;     // misfit: the receiver rows and the sparse cotangent built on them

  void solve(int t, const Blk<T>& b, int64_t g0, int gc, bool cjin, T* out) { gs.solve(t, b, g0, gc, cjin, out); }

  void run(double* info) {
    hipStream_t s = c.s;
    n = c.n;
    gs.F = c.F;
    gs.n = n;
    gs.itmax = c.itmax;
    gs.s = s;
    // (an equilibrated handle takes the same route: the pruned sweeps refuse it, so the driver's own sparse cotangent of hs_misfit_* is
    // expanded and solved by the block solve, which scales around its sweeps)
    gs.ulv = c.v.ulv != 0 || hs_handle_equilibrated(c.F) != 0;
    const bool cplx_ = sizeof(T) == 16;
    const bool cjw = cplx_ && c.trans == 1;  // the adjoint solve runs on conj(W) and returns conj(Lam)
    const int tadj = c.trans == 0 ? 2 : 0;
    const int64_t nnz = c.v.nnz, glen = c.pattern == 0 ? nnz : n;
    HS_HIP(hipMemsetAsync(c.dG, 0, (size_t)glen * sizeof(T), s));
    if (c.nrhs == 0) {
      HS_HIP(hipStreamSynchronize(s));
      return;
    }
    const bool wsparse = c.misfit || c.W.sparse();
    const bool expand = c.itmax > 0 || gs.ulv;  // sparse blocks reach their solve as dense ones
    const bool need_stage = expand && (c.B.sparse() || wsparse || (cjw && c.itmax > 0));
    const size_t per_col = (size_t)n * sizeof(T) * (need_stage ? 3 : 2) + (c.misfit ? (size_t)c.nrows * sizeof(T) : 0);
    Gc = std::min<int64_t>(group_width(per_col, c.nrhs, "HS_SENS_GROUP", "hs_sens_*"), c.nrhs);
    Xg = buf.get<T>((size_t)n * Gc);
    Lg = buf.get<T>((size_t)n * Gc);
    if (need_stage) gs.stage = buf.get<T>((size_t)n * Gc);
    size_t extra = 0;
    int64_t maxw = 0, maxe = 0;  // the most stored entries a group of W / of either block holds
    for (int64_t g0 = 0; g0 < c.nrhs; g0 += Gc) {
      const int64_t g1 = std::min<int64_t>(g0 + Gc, c.nrhs);
      if (c.B.sparse()) maxe = std::max(maxe, c.B.nnz(g0, g1));
      if (!c.misfit && c.W.sparse()) maxw = std::max(maxw, c.W.nnz(g0, g1));
    }
    if (c.misfit) maxw = c.nrows * Gc;
    maxe = std::max(maxe, maxw);
    if (cjw && !c.misfit && c.W.sparse() && !expand) {
      gs.vstage = buf.get<T>((size_t)maxw);
      extra += (size_t)maxw * sizeof(T);
    }
    if (expand && (c.B.sparse() || wsparse)) {
      gs.d_er = buf.get<int32_t>((size_t)maxe);
      gs.d_ec = buf.get<int32_t>((size_t)maxe);
      extra += (size_t)maxe * 2 * sizeof(int32_t);
    }
    if (c.pattern == 0) {
      ecol = buf.get<int32_t>((size_t)nnz);
      extra += (size_t)nnz * sizeof(int32_t);
      launch_sens_entry_cols(c.v.colptr, n, nnz, ecol, s);
    }
    if (c.misfit) extra += rr.setup(c.rows, c.nrows, Gc, buf);
    info[SI_WORK_BYTES] = (double)(per_col * (size_t)Gc + extra);

    HsSddmmFlags fl;
    fl.swap = c.trans != 0;
    fl.conjl = cplx_ && c.trans != 0;  // trans 1: L holds M = conj(Lam); trans 2: conj(Lam) is what the sum takes
    fl.conjr = cplx_ && c.trans != 2;
    HsEvents<5> ev;
    HsDrain drain{s};  // nothing in flight may outlive the workspace
    for (int64_t g0 = 0; g0 < c.nrhs; g0 += Gc) {
      const int gc = (int)std::min<int64_t>(Gc, c.nrhs - g0);
      HS_HIP(hipEventRecord(ev[0], s));
      solve(c.trans, c.B, g0, gc, false, Xg);
      HS_HIP(hipEventRecord(ev[1], s));
      if (c.dX) HS_HIP(hipMemcpy2DAsync(c.dX + (size_t)g0 * c.ldx, c.ldx * sizeof(T), Xg, n * sizeof(T), n * sizeof(T), gc, hipMemcpyDeviceToDevice, s));
      if (c.misfit)
        launch_sens_misfit<T>(Xg, n, rr.d_rows, rr.d_slot, c.dD + (size_t)g0 * c.ldd, c.ldd, c.nrows, gc, c.dR ? c.dR + (size_t)g0 * c.ldr : nullptr, c.ldr, rr.Wv, cjw ? 1 : 0,
                              c.dJ + g0, s);
      HS_HIP(hipEventRecord(ev[2], s));
      if (c.misfit)
        solve(tadj, rr.W, 0, gc, false, Lg);  // the conjugation is in Wv already
      else
        solve(tadj, c.W, g0, gc, cjw, Lg);
      HS_HIP(hipEventRecord(ev[3], s));
      if (c.dLam) launch_sens_copy<T>(c.dLam + (size_t)g0 * c.ldl, c.ldl, Lg, n, n, gc, cjw ? 1 : 0, s);
      if (c.pattern == 0)
        launch_sddmm<T>(c.v.rowval, ecol, nnz, Lg, n, Xg, n, gc, fl, c.dG, s);
      else
        launch_sddmm_diag<T>(c.v.colptr, c.v.rowval, n, Lg, n, Xg, n, gc, fl, c.dG, s);
      HS_HIP(hipEventRecord(ev[4], s));
      HS_HIP(hipEventSynchronize(ev[4]));
      HS_CHECK(hs_handle_flow_check(c.F));
      float ms[4] = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < 4; ++k) HS_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
      info[SI_FORWARD] += ms[0] * 1e-3;
      info[SI_ADJOINT] += ms[2] * 1e-3;
      info[SI_REDUCE] += (ms[1] + ms[3]) * 1e-3;
      info[SI_SECONDS] += (ms[0] + ms[1] + ms[2] + ms[3]) * 1e-3;
      info[SI_GROUPS] += 1;
      info[SI_PRODUCTS] += (double)glen * gc;
    }
  }
};

// hs_ulv_mode 1 on a handle with HSS interior blocks: the caller's sparse blocks stay refused -- they are solved by the pruned sweeps of
// hs_ldiv_sparse_*, which run no HSS hook
void check_dense_under_ulv(const HsHandleView& v, const char* fn, const char* name, const hs_block_arg* b, int64_t nrhs) {
  if (v.ulv && nrhs > 0 && !b->dense)
    HS_FAIL(HS_ERR_UNSUPPORTED, v.t_refused_node,
            "%s: %s is a sparse block, and node %d keeps its interior block D as an HSS matrix (hs_options.hss_d / mf = 2, 3): with hs_ulv_mode 1 the ULV block solve "
            "serves dense blocks only (sparse blocks are solved on pruned tree paths, which run no ULV solves); pass %s dense",
            fn, name, v.t_refused_node, name);
}

void finish(hs_handle* F, const double* info) { memcpy(hs_handle_sens_info(F), info, 8 * sizeof(double)); }

template <class T>
void sens_entry(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const hs_block_arg* W, int64_t itmax, int pattern, T* G, T* X, int64_t ldx, T* Lam,
                int64_t ldl, bool on_device, void* stream) {
  const char* fn = on_device ? "hs_sens_dev_*" : "hs_sens_*";
  Call<T> c;
  check_common<T>(F, fn, trans, n, nrhs, itmax, pattern, &c.v, true);
  check_block<T>(F, trans, fn, "B", B, n, nrhs);
  check_block<T>(F, trans, fn, "W", W, n, nrhs);
  check_dense_under_ulv(c.v, fn, "B", B, nrhs);
  check_dense_under_ulv(c.v, fn, "W", W, nrhs);
  if (!G) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: G == NULL", fn);
  if ((X && ldx < n) || (Lam && ldl < n)) HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: ldx = %lld, ldl = %lld, the blocks have %lld rows", fn, (long long)ldx, (long long)ldl, (long long)n);
  c.F = F; c.trans = trans; c.pattern = pattern; c.n = n; c.nrhs = nrhs; c.itmax = itmax;
  double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HsDevBuf buf("condest workspace");  // freed after the stream is drained, on every path
  const int64_t glen = pattern == 0 ? c.v.nnz : n;
  if (on_device) {
    to_blk<T>(B, &c.B);
    to_blk<T>(W, &c.W);
    c.dG = G; c.dX = X; c.ldx = ldx; c.dLam = Lam; c.ldl = ldl;
    c.s = (hipStream_t)stream;
    Driver<T> d{c, buf};
    d.run(info);
    return finish(F, info);
  }
  c.s = c.v.stream;
  {
    HsDrain drain{c.s};
    upload<T>(B, n, nrhs, &c.B, buf, c.s, &info[SI_MOVED]);
    upload<T>(W, n, nrhs, &c.W, buf, c.s, &info[SI_MOVED]);
    c.dG = buf.get<T>((size_t)glen);
    if (X && nrhs > 0) { c.dX = buf.get<T>((size_t)n * nrhs); c.ldx = n; }
    if (Lam && nrhs > 0) { c.dLam = buf.get<T>((size_t)n * nrhs); c.ldl = n; }
    Driver<T> d{c, buf};
    d.run(info);
    // results go to the caller's arrays only when the whole call succeeded
    if (glen > 0) HS_HIP(hipMemcpyAsync(G, c.dG, (size_t)glen * sizeof(T), hipMemcpyDeviceToHost, c.s));
    if (c.dX) HS_HIP(hipMemcpy2DAsync(X, ldx * sizeof(T), c.dX, n * sizeof(T), n * sizeof(T), nrhs, hipMemcpyDeviceToHost, c.s));
    if (c.dLam) HS_HIP(hipMemcpy2DAsync(Lam, ldl * sizeof(T), c.dLam, n * sizeof(T), n * sizeof(T), nrhs, hipMemcpyDeviceToHost, c.s));
    HS_HIP(hipStreamSynchronize(c.s));
    info[SI_MOVED] += (double)glen + (c.dX ? (double)n * nrhs : 0.0) + (c.dLam ? (double)n * nrhs : 0.0);
  }
  finish(F, info);
}

template <class T>
void misfit_entry(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const int64_t* rows, int64_t nrows, const T* D, int64_t ldd, int64_t itmax,
                  int pattern, double* J, T* R, int64_t ldr, T* G, bool on_device, void* stream) {
  const char* fn = on_device ? "hs_misfit_dev_*" : "hs_misfit_*";
  Call<T> c;
  check_common<T>(F, fn, trans, n, nrhs, itmax, pattern, &c.v, true);
  check_block<T>(F, trans, fn, "B", B, n, nrhs);
  check_dense_under_ulv(c.v, fn, "B", B, nrhs);
  if (nrows < 0 || nrows > n) HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: nrows = %lld, F is %lld x %lld", fn, (long long)nrows, (long long)n, (long long)n);
  if (!G || (nrows > 0 && !rows) || (nrhs > 0 && !J) || (nrows > 0 && nrhs > 0 && !D)) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: G, rows, D and J must not be NULL", fn);
  if (ldd < nrows || (R && ldr < nrows))
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: ldd = %lld, ldr = %lld, D and R have %lld rows", fn, (long long)ldd, (long long)ldr, (long long)nrows);
  check_rows(fn, rows, nrows, n);
  c.F = F; c.trans = trans; c.pattern = pattern; c.n = n; c.nrhs = nrhs; c.itmax = itmax;
  c.misfit = true; c.rows = rows; c.nrows = nrows;
  double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HsDevBuf buf("condest workspace");
  const int64_t glen = pattern == 0 ? c.v.nnz : n;
  if (on_device) {
    to_blk<T>(B, &c.B);
    c.dD = D; c.ldd = ldd; c.dJ = J; c.dR = R; c.ldr = ldr; c.dG = G;
    c.s = (hipStream_t)stream;
    Driver<T> d{c, buf};
    d.run(info);
    return finish(F, info);
  }
  c.s = c.v.stream;
  {
    HsDrain drain{c.s};
    upload<T>(B, n, nrhs, &c.B, buf, c.s, &info[SI_MOVED]);
    const size_t dn = (size_t)nrows * nrhs;
    T* dD = buf.get<T>(dn);
    if (dn > 0) HS_HIP(hipMemcpy2DAsync(dD, nrows * sizeof(T), D, ldd * sizeof(T), nrows * sizeof(T), nrhs, hipMemcpyHostToDevice, c.s));
    c.dD = dD; c.ldd = nrows;
    c.dG = buf.get<T>((size_t)glen);
    c.dJ = buf.get<double>((size_t)nrhs);
    if (R) { c.dR = buf.get<T>(dn); c.ldr = nrows; }
    Driver<T> d{c, buf};
    d.run(info);
    if (glen > 0) HS_HIP(hipMemcpyAsync(G, c.dG, (size_t)glen * sizeof(T), hipMemcpyDeviceToHost, c.s));
    if (nrhs > 0) HS_HIP(hipMemcpyAsync(J, c.dJ, (size_t)nrhs * sizeof(double), hipMemcpyDeviceToHost, c.s));
    if (R && dn > 0) HS_HIP(hipMemcpy2DAsync(R, ldr * sizeof(T), c.dR, nrows * sizeof(T), nrows * sizeof(T), nrhs, hipMemcpyDeviceToHost, c.s));
    HS_HIP(hipStreamSynchronize(c.s));
    info[SI_MOVED] += (double)dn + (double)glen + (double)nrhs + (R ? (double)dn : 0.0);
  }
  finish(F, info);
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
extern "C" int hs_sens_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const hs_block_arg* W, int64_t itmax, int pattern, double* G, double* X,
                         int64_t ldx, double* Lam, int64_t ldl) {
  HS_GUARD(sens_entry<double>(F, trans, n, nrhs, B, W, itmax, pattern, G, X, ldx, Lam, ldl, false, nullptr));
}
extern "C" int hs_sens_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const hs_block_arg* W, int64_t itmax, int pattern, double* G, double* X,
                         int64_t ldx, double* Lam, int64_t ldl) {
  HS_GUARD(sens_entry<cplx>(F, trans, n, nrhs, B, W, itmax, pattern, (cplx*)G, (cplx*)X, ldx, (cplx*)Lam, ldl, false, nullptr));
}
extern "C" int hs_sens_dev_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const hs_block_arg* W, int64_t itmax, int pattern, double* dG,
                             double* dX, int64_t ldx, double* dLam, int64_t ldl, void* stream) {
  HS_GUARD(sens_entry<double>(F, trans, n, nrhs, B, W, itmax, pattern, dG, dX, ldx, dLam, ldl, true, stream));
}
extern "C" int hs_sens_dev_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const hs_block_arg* W, int64_t itmax, int pattern, double* dG,
                             double* dX, int64_t ldx, double* dLam, int64_t ldl, void* stream) {
  HS_GUARD(sens_entry<cplx>(F, trans, n, nrhs, B, W, itmax, pattern, (cplx*)dG, (cplx*)dX, ldx, (cplx*)dLam, ldl, true, stream));
}
extern "C" int hs_misfit_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const int64_t* rows, int64_t nrows, const double* D, int64_t ldd,
                           int64_t itmax, int pattern, double* J, double* R, int64_t ldr, double* G) {
  HS_GUARD(misfit_entry<double>(F, trans, n, nrhs, B, rows, nrows, D, ldd, itmax, pattern, J, R, ldr, G, false, nullptr));
}
extern "C" int hs_misfit_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const int64_t* rows, int64_t nrows, const double* D, int64_t ldd,
                           int64_t itmax, int pattern, double* J, double* R, int64_t ldr, double* G) {
  HS_GUARD(misfit_entry<cplx>(F, trans, n, nrhs, B, rows, nrows, (const cplx*)D, ldd, itmax, pattern, J, (cplx*)R, ldr, (cplx*)G, false, nullptr));
}
extern "C" int hs_misfit_dev_d(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const int64_t* rows, int64_t nrows, const double* dD, int64_t ldd,
                               int64_t itmax, int pattern, double* dJ, double* dR, int64_t ldr, double* dG, void* stream) {
  HS_GUARD(misfit_entry<double>(F, trans, n, nrhs, B, rows, nrows, dD, ldd, itmax, pattern, dJ, dR, ldr, dG, true, stream));
}
extern "C" int hs_misfit_dev_z(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const int64_t* rows, int64_t nrows, const double* dD, int64_t ldd,
                               int64_t itmax, int pattern, double* dJ, double* dR, int64_t ldr, double* dG, void* stream) {
  HS_GUARD(misfit_entry<cplx>(F, trans, n, nrhs, B, rows, nrows, (const cplx*)dD, ldd, itmax, pattern, dJ, (cplx*)dR, ldr, (cplx*)dG, true, stream));
}
extern "C" int hs_sens_info(const hs_handle* F, double* out8) {
  if (!F || !out8) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_sens_info: null argument");
    return HS_ERR_ARGUMENT;
  }
  memcpy(out8, hs_handle_sens_info(const_cast<hs_handle*>(F)), 8 * sizeof(double));
  return HS_OK;
}
