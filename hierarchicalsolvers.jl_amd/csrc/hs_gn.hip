// hs_gn.hip -- tangent-linear solves and Gauss-Newton Hessian products on A's pattern for a block of sources (hs_tangent_*, hs_gn_hessvec_*,
// hs_gn_diag_*; include/hs_solver.h): the forward mode next to the reverse mode of hs_sens.hip.
//
// With X = op(A)^-1 B and a perturbation E of the stored entries of A,
//
//   dX(E) = d/ds op(A + sE)^-1 B at s = 0 = -op(A)^-1 op(E) X,        J E = dX(E)[rows, :],        H E = J* J E,
//
// where J* is the adjoint in the real inner product: H E is the G of hs_sens_* for the cotangent W = scatter(J E).  The columns go in groups
// of Gc.  Per group: the forward solve (skipped when the caller supplies the fields), the right-hand side P = -op(E) X (kernels_gn.hip), the
// tangent solve, the receiver rows of its solution -- returned (hs_tangent_*) or turned into the sparse cotangent on the device -- the adjoint
// solve on the pruned path, and the reduction kernel of hs_sens_* (kernels_sens.hip, unchanged), which continues the chain of every stored
// entry.  Every solve is one of the library's own entry points, chosen as hs_sens.hip chooses (hs_sens_solve.h); nothing of size n x k leaves
// the device unless asked for.  The block that holds P is reused for the adjoint state.
//
// hs_gn_diag_* runs in two phases: the forward groups accumulate x2[q] = sum_c |X[q, c]|^2, then the unit columns of the receiver rows go in
// groups through the adjoint path and accumulate z2[q] = sum_r |Z[q, r]|^2, Z = op(A)^-H S; the diagonal of H at the stored (i, j) is
// z2[i] x2[j] (trans 0) or z2[j] x2[i] (trans 1, 2).
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
#define HS_CONDEST_KERNELS  // hs_ce::csr_of; switches contraction off for the rest of this file (host arithmetic only: no kernel lives here)
#include "hs_condest.h"
#include "hs_block_apply.h"
#include "hs_solve_multi.h"  // hs_ldiv_block_cols
#include "hs_sens.h"
#include "hs_sens_solve.h"
#include "hs_gn.h"

namespace {

enum { GI_SECONDS = 0, GI_FORWARD, GI_TANGENT, GI_ADJOINT, GI_PRODUCTS, GI_GROUPS, GI_SOLVES, GI_WORK_BYTES };
enum { GN_TANGENT = 0, GN_HESSVEC, GN_DIAG };

template <class T>
struct Call {
  hs_handle* F = nullptr;
  HsHandleView v;
  const char* fn = "";
  int trans = 0, pattern = 0, mode = GN_TANGENT;
  int64_t n = 0, nrhs = 0, itmax = 0;
  Blk<T> B;               // read when dXin is null
  const T* dXin = nullptr;  // the fields of an earlier call: the forward solve is skipped
  int64_t ldxin = 0;
  const T* dE = nullptr;  // nnz(A) or n values
  const int64_t* rows = nullptr;  // 1-based, distinct; null (hs_tangent_*): all rows
  int64_t nrows = 0;
  T* dOut = nullptr;  // hs_tangent_*: dX, n x nrhs or nrows x nrhs
  int64_t ldo = 0;
  T* dX = nullptr;
  int64_t ldx = 0;
  T* dHE = nullptr;
  T* dJE = nullptr;
  int64_t ldj = 0;
  double* dHd = nullptr;
  double* dz2 = nullptr;
  double* dx2 = nullptr;
  hipStream_t s = nullptr;

  int64_t glen() const { return pattern == 0 ? v.nnz : n; }
  bool empty() const { return nrhs == 0 || (nrows == 0 && (rows || mode != GN_TANGENT)); }
};

template <class T>
void zero_block(T* d, int64_t ld, int64_t rows, int64_t cols, hipStream_t s) {
  if (d && rows > 0 && cols > 0) HS_HIP(hipMemset2DAsync(d, ld * sizeof(T), 0, rows * sizeof(T), cols, s));
}

template <class T>
HsGnRows op_rows_of(const Call<T>& c) {
  if (c.trans == 0) {
    hs_ce::CsrMap* m = hs_ce::csr_of<T>(c.v, c.s);
    return HsGnRows{m->rowptr, m->colind, m->tperm, 0};
  }
  return HsGnRows{c.v.colptr, c.v.rowval, nullptr, (sizeof(T) == 16 && c.trans == 2) ? 1 : 0};
}

template <class T>
void group_solver(const Call<T>& c, HsGroupSolve<T>* gs) {
  gs->F = c.F;
  gs->n = c.n;
  gs->itmax = c.itmax;
  gs->s = c.s;
}

// hs_tangent_* and hs_gn_hessvec_*
template <class T>
void run_products(const Call<T>& c, HsDevBuf& buf, double* info) {
  hipStream_t s = c.s;
  const int64_t n = c.n, nnz = c.v.nnz;
  const bool cplx_ = sizeof(T) == 16, hv = c.mode == GN_HESSVEC;
  const bool cjw = cplx_ && c.trans == 1;  // the adjoint solve runs on conj(W) and returns conj(Lam), as in hs_sens.hip
  const int tadj = c.trans == 0 ? 2 : 0;
  if (hv) HS_HIP(hipMemsetAsync(c.dHE, 0, (size_t)c.glen() * sizeof(T), s));
  if (c.empty()) {
    zero_block<T>(c.dOut, c.ldo, c.rows ? c.nrows : n, c.nrhs, s);
    zero_block<T>(c.dJE, c.ldj, c.nrows, c.nrhs, s);
    zero_block<T>(c.dX, c.ldx, n, c.nrhs, s);
    HS_HIP(hipStreamSynchronize(s));
    return;
  }
  HsGroupSolve<T> gs;
  group_solver<T>(c, &gs);
  const bool bsparse = !c.dXin && c.B.sparse();
  const bool need_stage = c.itmax > 0 && (bsparse || hv);
  const size_t per_col = (size_t)n * sizeof(T) * ((c.dXin ? 2 : 3) + (need_stage ? 1 : 0)) + (hv ? (size_t)c.nrows * sizeof(T) : 0);
  const int64_t Gc = std::min<int64_t>(group_width(per_col, c.nrhs, "HS_GN_GROUP", c.fn), c.nrhs);
  T* Xg = c.dXin ? nullptr : buf.get<T>((size_t)n * Gc);
  T* Pg = buf.get<T>((size_t)n * Gc);  // P = -op(E) X, then Lam (or conj(Lam): ComplexF64, trans = 1)
  T* Dg = buf.get<T>((size_t)n * Gc);  // dX
  if (need_stage) gs.stage = buf.get<T>((size_t)n * Gc);
  size_t extra = 0;
  int64_t maxe = hv ? c.nrows * Gc : 0;  // the most stored entries a sparse group holds
  if (bsparse)
    for (int64_t g0 = 0; g0 < c.nrhs; g0 += Gc) maxe = std::max(maxe, c.B.nnz(g0, std::min<int64_t>(g0 + Gc, c.nrhs)));
  if (c.itmax > 0 && (bsparse || hv)) {
    gs.d_er = buf.get<int32_t>((size_t)maxe);
    gs.d_ec = buf.get<int32_t>((size_t)maxe);
    extra += (size_t)maxe * 2 * sizeof(int32_t);
  }
  int32_t* ecol = nullptr;
  if (hv && c.pattern == 0) {
    ecol = buf.get<int32_t>((size_t)nnz);
    extra += (size_t)nnz * sizeof(int32_t);
    launch_sens_entry_cols(c.v.colptr, n, nnz, ecol, s);
  }
  HsReceiverRows<T> rr;
  if (c.rows) extra += rr.setup(c.rows, c.nrows, hv ? Gc : 0, buf);
  HsGnRows er{nullptr, nullptr, nullptr, 0};
  if (c.pattern == 0) er = op_rows_of<T>(c);
  info[GI_WORK_BYTES] = (double)(per_col * (size_t)Gc + extra);

  HsSddmmFlags fl;
  fl.swap = c.trans != 0;
  fl.conjl = cplx_ && c.trans != 0;
  fl.conjr = cplx_ && c.trans != 2;
  HsEvents<7> ev;
  HsDrain drain{s};  // nothing in flight may outlive the workspace
  for (int64_t g0 = 0; g0 < c.nrhs; g0 += Gc) {
    const int gc = (int)std::min<int64_t>(Gc, c.nrhs - g0);
    HS_HIP(hipEventRecord(ev[0], s));
    const T* Xp = Xg;
    int64_t ldxp = n;
    if (c.dXin) {
      Xp = c.dXin + (size_t)g0 * c.ldxin;
      ldxp = c.ldxin;
    } else {
      gs.solve(c.trans, c.B, g0, gc, false, Xg);
    }
    HS_HIP(hipEventRecord(ev[1], s));
    if (c.dX && c.dX + (size_t)g0 * c.ldx != Xp)
      HS_HIP(hipMemcpy2DAsync(c.dX + (size_t)g0 * c.ldx, c.ldx * sizeof(T), Xp, ldxp * sizeof(T), n * sizeof(T), gc, hipMemcpyDeviceToDevice, s));
    if (c.pattern == 0)
      launch_gn_rhs<T>(er, c.dE, n, Xp, ldxp, gc, Pg, n, s);
    else
      launch_gn_rhs_diag<T>(c.v.colptr, c.v.rowval, c.dE, (cplx_ && c.trans == 2) ? 1 : 0, n, Xp, ldxp, gc, Pg, n, s);
    HS_HIP(hipEventRecord(ev[2], s));
    {
      Blk<T> Pb;
      Pb.dense = Pg;
      Pb.ld = n;
      gs.solve(c.trans, Pb, 0, gc, false, Dg);
    }
    HS_HIP(hipEventRecord(ev[3], s));
    if (hv)
      launch_gn_rows<T>(Dg, n, rr.d_rows, rr.d_slot, c.nrows, gc, c.dJE ? c.dJE + (size_t)g0 * c.ldj : nullptr, c.ldj, rr.Wv, cjw ? 1 : 0, s);
    else if (c.rows)
      launch_gn_rows<T>(Dg, n, rr.d_rows, rr.d_slot, c.nrows, gc, c.dOut + (size_t)g0 * c.ldo, c.ldo, nullptr, 0, s);
    else
      HS_HIP(hipMemcpy2DAsync(c.dOut + (size_t)g0 * c.ldo, c.ldo * sizeof(T), Dg, n * sizeof(T), n * sizeof(T), gc, hipMemcpyDeviceToDevice, s));
    HS_HIP(hipEventRecord(ev[4], s));
    if (hv) gs.solve(tadj, rr.W, 0, gc, false, Pg);  // the conjugation is in Wv already
    HS_HIP(hipEventRecord(ev[5], s));
    if (hv) {
      if (c.pattern == 0)
        launch_sddmm<T>(c.v.rowval, ecol, nnz, Pg, n, Xp, ldxp, gc, fl, c.dHE, s);
      else
        launch_sddmm_diag<T>(c.v.colptr, c.v.rowval, n, Pg, n, Xp, ldxp, gc, fl, c.dHE, s);
    }
    HS_HIP(hipEventRecord(ev[6], s));
    HS_HIP(hipEventSynchronize(ev[6]));
    HS_CHECK(hs_handle_flow_check(c.F));
    float ms[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 6; ++k) HS_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    info[GI_FORWARD] += ms[0] * 1e-3;
    info[GI_TANGENT] += ms[2] * 1e-3;
    info[GI_ADJOINT] += ms[4] * 1e-3;
    info[GI_PRODUCTS] += (ms[1] + ms[3] + ms[5]) * 1e-3;
    info[GI_SECONDS] += (ms[0] + ms[1] + ms[2] + ms[3] + ms[4] + ms[5]) * 1e-3;
    info[GI_GROUPS] += 1;
  }
  info[GI_SOLVES] = (double)gs.solves;
}

// hs_gn_diag_*
template <class T>
void run_diag(const Call<T>& c, double* info) {
  hipStream_t s = c.s;
  const int64_t n = c.n, nnz = c.v.nnz;
  const bool cplx_ = sizeof(T) == 16;
  const bool cjw = cplx_ && c.trans == 1;
  const int tadj = c.trans == 0 ? 2 : 0;
  HS_HIP(hipMemsetAsync(c.dHd, 0, (size_t)c.glen() * sizeof(double), s));
  HS_HIP(hipMemsetAsync(c.dz2, 0, (size_t)n * sizeof(double), s));
  HS_HIP(hipMemsetAsync(c.dx2, 0, (size_t)n * sizeof(double), s));
  if (c.empty()) {
    HS_HIP(hipStreamSynchronize(s));
    return;
  }
  size_t work = 0;
  {  // the forward groups: x2
    HsDevBuf buf("gn workspace");
    HsGroupSolve<T> gs;
    group_solver<T>(c, &gs);
    const bool bsparse = !c.dXin && c.B.sparse();
    const bool need_stage = c.itmax > 0 && bsparse;
    const size_t per_col = c.dXin ? 0 : (size_t)n * sizeof(T) * (need_stage ? 2 : 1);
    const int64_t Gc = c.dXin ? c.nrhs : std::min<int64_t>(group_width(per_col, c.nrhs, "HS_GN_GROUP", c.fn), c.nrhs);
    T* Xg = c.dXin ? nullptr : buf.get<T>((size_t)n * Gc);
    if (need_stage) {
      int64_t maxe = 0;
      for (int64_t g0 = 0; g0 < c.nrhs; g0 += Gc) maxe = std::max(maxe, c.B.nnz(g0, std::min<int64_t>(g0 + Gc, c.nrhs)));
      gs.stage = buf.get<T>((size_t)n * Gc);
      gs.d_er = buf.get<int32_t>((size_t)maxe);
      gs.d_ec = buf.get<int32_t>((size_t)maxe);
    }
    work = per_col * (size_t)Gc;
    HsEvents<3> ev;
    HsDrain drain{s};
    for (int64_t g0 = 0; g0 < c.nrhs; g0 += Gc) {
      const int gc = (int)std::min<int64_t>(Gc, c.nrhs - g0);
      HS_HIP(hipEventRecord(ev[0], s));
      if (!c.dXin) gs.solve(c.trans, c.B, g0, gc, false, Xg);
      HS_HIP(hipEventRecord(ev[1], s));
      if (c.dXin)
        launch_gn_rowsq<T>(c.dXin + (size_t)g0 * c.ldxin, c.ldxin, n, gc, c.dx2, s);
      else
        launch_gn_rowsq<T>(Xg, n, n, gc, c.dx2, s);
      HS_HIP(hipEventRecord(ev[2], s));
      HS_HIP(hipEventSynchronize(ev[2]));
      HS_CHECK(hs_handle_flow_check(c.F));
      float ms[2] = {0.f, 0.f};
      for (int k = 0; k < 2; ++k) HS_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
      info[GI_FORWARD] += ms[0] * 1e-3;
      info[GI_PRODUCTS] += ms[1] * 1e-3;
      info[GI_SECONDS] += (ms[0] + ms[1]) * 1e-3;
      info[GI_GROUPS] += 1;
    }
    info[GI_SOLVES] += (double)gs.solves;
  }
  {  // the unit columns of the receiver rows through the adjoint path: z2, then the diagonal
    HsDevBuf buf("gn workspace");
    HsGroupSolve<T> gs;
    group_solver<T>(c, &gs);
    const int64_t nr = c.nrows;
    const size_t per_col = (size_t)n * sizeof(T) * (c.itmax > 0 ? 2 : 1) + sizeof(T);
    const int64_t Gc = std::min<int64_t>(group_width(per_col, nr, "HS_GN_GROUP", c.fn), nr);
    T* Lg = buf.get<T>((size_t)n * Gc);
    T* ones = buf.get<T>((size_t)nr);
    {
      const std::vector<T> one((size_t)nr, Scal<T>::one());
      HS_HIP(hipMemcpy(ones, one.data(), (size_t)nr * sizeof(T), hipMemcpyHostToDevice));
    }
    std::vector<int64_t> scp((size_t)nr + 1);
    std::iota(scp.begin(), scp.end(), (int64_t)1);
    Blk<T> S;  // column r = the unit column of rows[r]
    S.colptr = scp.data();
    S.rowval = c.rows;
    S.nzval = ones;
    size_t extra = (size_t)nr * sizeof(T);
    if (c.itmax > 0) {
      gs.stage = buf.get<T>((size_t)n * Gc);
      gs.d_er = buf.get<int32_t>((size_t)Gc);
      gs.d_ec = buf.get<int32_t>((size_t)Gc);
    } else if (cjw) {
      gs.vstage = buf.get<T>((size_t)Gc);
    }
    int32_t* ecol = nullptr;
    if (c.pattern == 0) {
      ecol = buf.get<int32_t>((size_t)nnz);
      extra += (size_t)nnz * sizeof(int32_t);
      launch_sens_entry_cols(c.v.colptr, n, nnz, ecol, s);
    }
    work = std::max(work, per_col * (size_t)Gc + extra);
    HsEvents<3> ev;
    HsDrain drain{s};
    for (int64_t g0 = 0; g0 < nr; g0 += Gc) {
      const int gc = (int)std::min<int64_t>(Gc, nr - g0);
      HS_HIP(hipEventRecord(ev[0], s));
      gs.solve(tadj, S, g0, gc, cjw, Lg);
      HS_HIP(hipEventRecord(ev[1], s));
      launch_gn_rowsq<T>(Lg, n, n, gc, c.dz2, s);
      if (g0 + gc == nr) {
        if (c.pattern == 0)
          launch_gn_diag(c.v.rowval, ecol, nnz, c.dz2, c.dx2, c.trans != 0, c.dHd, s);
        else
          launch_gn_diag_diag(c.v.colptr, c.v.rowval, n, c.dz2, c.dx2, c.dHd, s);
      }
      HS_HIP(hipEventRecord(ev[2], s));
      HS_HIP(hipEventSynchronize(ev[2]));
      HS_CHECK(hs_handle_flow_check(c.F));
      float ms[2] = {0.f, 0.f};
      for (int k = 0; k < 2; ++k) HS_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
      info[GI_ADJOINT] += ms[0] * 1e-3;
      info[GI_PRODUCTS] += ms[1] * 1e-3;
      info[GI_SECONDS] += (ms[0] + ms[1]) * 1e-3;
      info[GI_GROUPS] += 1;
    }
    info[GI_SOLVES] += (double)gs.solves;
  }
  info[GI_WORK_BYTES] = (double)work;
}

// ---- refusals: before any device work, every output untouched ------------------------------------------------------------------------
template <class T>
void check_gn(Call<T>* c, hs_handle* F, const char* fn, int mode, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const T* Xin, int64_t ldxin, const T* E,
              int pattern, int64_t itmax, const int64_t* rows, int64_t nrows) {
  hs_view_of(F, fn);  // a null handle
  if (!B && !Xin) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: B and Xin are both NULL (the right-hand sides, or the fields of an earlier call)", fn);
  check_common<T>(F, fn, trans, n, nrhs, itmax, pattern, &c->v);
  // the adjoint columns of the receiver rows are sparse and take the pruned sweeps of hs_ldiv_sparse_* unless they are refined (itmax > 0)
  if (mode != GN_TANGENT && itmax == 0) hs_refuse_equilibrated(F, fn);
  if (Xin) {
    if (nrhs > 0 && ldxin < n) HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: the leading dimension of Xin is %lld, it has %lld rows", fn, (long long)ldxin, (long long)n);
  } else {
    check_block<T>(F, trans, fn, "B", B, n, nrhs);
  }
  const int64_t glen = pattern == 0 ? c->v.nnz : n;
  if (mode != GN_DIAG && !E && glen > 0) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: E == NULL", fn);
  if (rows || mode != GN_TANGENT) {
    if (nrows < 0 || nrows > n) HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: nrows = %lld, F is %lld x %lld", fn, (long long)nrows, (long long)n, (long long)n);
    if (nrows > 0 && !rows) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: rows == NULL", fn);
    check_rows(fn, rows, nrows, n);
  }
  c->F = F; c->fn = fn; c->mode = mode; c->trans = trans; c->pattern = pattern; c->n = n; c->nrhs = nrhs; c->itmax = itmax;
  c->rows = rows; c->nrows = rows || mode != GN_TANGENT ? nrows : 0;
}

void finish(hs_handle* F, const double* info) { memcpy(hs_handle_gn_info(F), info, 8 * sizeof(double)); }

template <class T>
const T* upload_values(const T* h, size_t cnt, HsDevBuf& buf, hipStream_t s) {
  T* d = buf.get<T>(cnt);
  if (cnt > 0) HS_HIP(hipMemcpyAsync(d, h, cnt * sizeof(T), hipMemcpyHostToDevice, s));
  return d;
}
// the inputs of a host form on the device
template <class T>
void upload_inputs(Call<T>* c, const hs_block_arg* B, const T* Xin, int64_t ldxin, const T* E, HsDevBuf& buf) {
  double moved = 0;
  const int64_t n = c->n, nrhs = c->nrhs;
  if (Xin) {
    T* d = buf.get<T>((size_t)n * nrhs);
    if (nrhs > 0) HS_HIP(hipMemcpy2DAsync(d, n * sizeof(T), Xin, ldxin * sizeof(T), n * sizeof(T), nrhs, hipMemcpyHostToDevice, c->s));
    c->dXin = d;
    c->ldxin = n;
  } else {
    upload<T>(B, n, nrhs, &c->B, buf, c->s, &moved);
  }
  if (E) c->dE = upload_values<T>(E, (size_t)c->glen(), buf, c->s);
}
template <class T>
void download_block(T* h, int64_t ldh, const T* d, int64_t rows, int64_t cols, hipStream_t s) {
  if (h && rows > 0 && cols > 0) HS_HIP(hipMemcpy2DAsync(h, ldh * sizeof(T), d, rows * sizeof(T), rows * sizeof(T), cols, hipMemcpyDeviceToHost, s));
}

template <class T>
void tangent_entry(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const T* Xin, int64_t ldxin, const T* E, int pattern, int64_t itmax,
                   const int64_t* rows, int64_t nrows, T* dXo, int64_t lddx, T* X, int64_t ldx, bool on_device, void* stream) {
  const char* fn = on_device ? "hs_tangent_dev_*" : "hs_tangent_*";
  Call<T> c;
  check_gn<T>(&c, F, fn, GN_TANGENT, trans, n, nrhs, B, Xin, ldxin, E, pattern, itmax, rows, nrows);
  const int64_t orows = rows ? nrows : n;
  if (!dXo && orows > 0 && nrhs > 0) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: dX == NULL", fn);
  if (lddx < orows || (X && ldx < n))
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: lddx = %lld, ldx = %lld, dX has %lld rows and X %lld", fn, (long long)lddx, (long long)ldx, (long long)orows, (long long)n);
  double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HsDevBuf buf("gn workspace");  // freed after the stream is drained, on every path
  if (on_device) {
    if (!Xin) to_blk<T>(B, &c.B);
    c.dXin = Xin; c.ldxin = ldxin; c.dE = E; c.dOut = dXo; c.ldo = lddx; c.dX = X; c.ldx = ldx;
    c.s = (hipStream_t)stream;
    run_products<T>(c, buf, info);
    return finish(F, info);
  }
  c.s = c.v.stream;
  {
    HsDrain drain{c.s};
    upload_inputs<T>(&c, B, Xin, ldxin, E, buf);
    c.dOut = buf.get<T>((size_t)orows * nrhs); c.ldo = std::max<int64_t>(orows, 1);
    if (X && nrhs > 0) { c.dX = buf.get<T>((size_t)n * nrhs); c.ldx = n; }
    run_products<T>(c, buf, info);
    // results go to the caller's arrays only when the whole call succeeded
    download_block<T>(dXo, lddx, c.dOut, orows, nrhs, c.s);
    if (c.dX) download_block<T>(X, ldx, c.dX, n, nrhs, c.s);
    HS_HIP(hipStreamSynchronize(c.s));
  }
  finish(F, info);
}

template <class T>
void hessvec_entry(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const T* Xin, int64_t ldxin, const T* E, int pattern, int64_t itmax,
                   const int64_t* rows, int64_t nrows, T* HE, T* JE, int64_t ldje, T* X, int64_t ldx, bool on_device, void* stream) {
  const char* fn = on_device ? "hs_gn_hessvec_dev_*" : "hs_gn_hessvec_*";
  Call<T> c;
  check_gn<T>(&c, F, fn, GN_HESSVEC, trans, n, nrhs, B, Xin, ldxin, E, pattern, itmax, rows, nrows);
  if (!HE) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: HE == NULL", fn);
  if ((JE && ldje < nrows) || (X && ldx < n))
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: ldje = %lld, ldx = %lld, JE has %lld rows and X %lld", fn, (long long)ldje, (long long)ldx, (long long)nrows, (long long)n);
  double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HsDevBuf buf("gn workspace");
  const int64_t glen = c.glen();
  if (on_device) {
    if (!Xin) to_blk<T>(B, &c.B);
    c.dXin = Xin; c.ldxin = ldxin; c.dE = E; c.dHE = HE; c.dJE = JE; c.ldj = ldje; c.dX = X; c.ldx = ldx;
    c.s = (hipStream_t)stream;
    run_products<T>(c, buf, info);
    return finish(F, info);
  }
  c.s = c.v.stream;
  {
    HsDrain drain{c.s};
    upload_inputs<T>(&c, B, Xin, ldxin, E, buf);
    c.dHE = buf.get<T>((size_t)glen);
    if (JE && nrhs > 0) { c.dJE = buf.get<T>((size_t)nrows * nrhs); c.ldj = std::max<int64_t>(nrows, 1); }
    if (X && nrhs > 0) { c.dX = buf.get<T>((size_t)n * nrhs); c.ldx = n; }
    run_products<T>(c, buf, info);
    if (glen > 0) HS_HIP(hipMemcpyAsync(HE, c.dHE, (size_t)glen * sizeof(T), hipMemcpyDeviceToHost, c.s));
    if (c.dJE) download_block<T>(JE, ldje, c.dJE, nrows, nrhs, c.s);
    if (c.dX) download_block<T>(X, ldx, c.dX, n, nrhs, c.s);
    HS_HIP(hipStreamSynchronize(c.s));
  }
  finish(F, info);
}

template <class T>
void diag_entry(hs_handle* F, int trans, int64_t n, int64_t nrhs, const hs_block_arg* B, const T* Xin, int64_t ldxin, const int64_t* rows, int64_t nrows, int pattern,
                int64_t itmax, double* Hd, double* z2, double* x2, bool on_device, void* stream) {
  const char* fn = on_device ? "hs_gn_diag_dev_*" : "hs_gn_diag_*";
  Call<T> c;
  check_gn<T>(&c, F, fn, GN_DIAG, trans, n, nrhs, B, Xin, ldxin, nullptr, pattern, itmax, rows, nrows);
  if (!Hd) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: Hd == NULL", fn);
  double info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HsDevBuf buf("gn workspace");
  const int64_t glen = c.glen();
  if (on_device) {
    if (!Xin) to_blk<T>(B, &c.B);
    c.dXin = Xin; c.ldxin = ldxin;
    c.dHd = Hd;
    c.dz2 = z2 ? z2 : buf.get<double>((size_t)n);
    c.dx2 = x2 ? x2 : buf.get<double>((size_t)n);
    c.s = (hipStream_t)stream;
    HsDrain drain{c.s};
    run_diag<T>(c, info);
    return finish(F, info);
  }
  c.s = c.v.stream;
  {
    HsDrain drain{c.s};
    upload_inputs<T>(&c, B, Xin, ldxin, nullptr, buf);
    c.dHd = buf.get<double>((size_t)glen);
    c.dz2 = buf.get<double>((size_t)n);
    c.dx2 = buf.get<double>((size_t)n);
    run_diag<T>(c, info);
    if (glen > 0) HS_HIP(hipMemcpyAsync(Hd, c.dHd, (size_t)glen * sizeof(double), hipMemcpyDeviceToHost, c.s));
    if (z2 && n > 0) HS_HIP(hipMemcpyAsync(z2, c.dz2, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c.s));
    if (x2 && n > 0) HS_HIP(hipMemcpyAsync(x2, c.dx2, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c.s));
    HS_HIP(hipStreamSynchronize(c.s));
  }
  finish(F, info);
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
#define GN_TANGENT_ARGS                                                                                                                                             \
  hs_handle *F, int trans, int64_t n, int64_t nrhs, const hs_block_arg *B, const double *Xin, int64_t ldxin, const double *E, int pattern, int64_t itmax,           \
      const int64_t *rows, int64_t nrows, double *dX, int64_t lddx, double *X, int64_t ldx
#define GN_HESSVEC_ARGS                                                                                                                                             \
  hs_handle *F, int trans, int64_t n, int64_t nrhs, const hs_block_arg *B, const double *Xin, int64_t ldxin, const double *E, int pattern, int64_t itmax,           \
      const int64_t *rows, int64_t nrows, double *HE, double *JE, int64_t ldje, double *X, int64_t ldx
#define GN_DIAG_ARGS                                                                                                                                                \
  hs_handle *F, int trans, int64_t n, int64_t nrhs, const hs_block_arg *B, const double *Xin, int64_t ldxin, const int64_t *rows, int64_t nrows, int pattern,       \
      int64_t itmax, double *Hd, double *z2, double *x2

extern "C" int hs_tangent_d(GN_TANGENT_ARGS) { HS_GUARD(tangent_entry<double>(F, trans, n, nrhs, B, Xin, ldxin, E, pattern, itmax, rows, nrows, dX, lddx, X, ldx, false, nullptr)); }
extern "C" int hs_tangent_z(GN_TANGENT_ARGS) {
  HS_GUARD(tangent_entry<cplx>(F, trans, n, nrhs, B, (const cplx*)Xin, ldxin, (const cplx*)E, pattern, itmax, rows, nrows, (cplx*)dX, lddx, (cplx*)X, ldx, false, nullptr));
}
extern "C" int hs_tangent_dev_d(GN_TANGENT_ARGS, void* stream) {
  HS_GUARD(tangent_entry<double>(F, trans, n, nrhs, B, Xin, ldxin, E, pattern, itmax, rows, nrows, dX, lddx, X, ldx, true, stream));
}
extern "C" int hs_tangent_dev_z(GN_TANGENT_ARGS, void* stream) {
  HS_GUARD(tangent_entry<cplx>(F, trans, n, nrhs, B, (const cplx*)Xin, ldxin, (const cplx*)E, pattern, itmax, rows, nrows, (cplx*)dX, lddx, (cplx*)X, ldx, true, stream));
}
extern "C" int hs_gn_hessvec_d(GN_HESSVEC_ARGS) {
  HS_GUARD(hessvec_entry<double>(F, trans, n, nrhs, B, Xin, ldxin, E, pattern, itmax, rows, nrows, HE, JE, ldje, X, ldx, false, nullptr));
}
extern "C" int hs_gn_hessvec_z(GN_HESSVEC_ARGS) {
  HS_GUARD(hessvec_entry<cplx>(F, trans, n, nrhs, B, (const cplx*)Xin, ldxin, (const cplx*)E, pattern, itmax, rows, nrows, (cplx*)HE, (cplx*)JE, ldje, (cplx*)X, ldx, false,
                               nullptr));
}
extern "C" int hs_gn_hessvec_dev_d(GN_HESSVEC_ARGS, void* stream) {
  HS_GUARD(hessvec_entry<double>(F, trans, n, nrhs, B, Xin, ldxin, E, pattern, itmax, rows, nrows, HE, JE, ldje, X, ldx, true, stream));
}
extern "C" int hs_gn_hessvec_dev_z(GN_HESSVEC_ARGS, void* stream) {
  HS_GUARD(hessvec_entry<cplx>(F, trans, n, nrhs, B, (const cplx*)Xin, ldxin, (const cplx*)E, pattern, itmax, rows, nrows, (cplx*)HE, (cplx*)JE, ldje, (cplx*)X, ldx, true,
                               stream));
}
extern "C" int hs_gn_diag_d(GN_DIAG_ARGS) { HS_GUARD(diag_entry<double>(F, trans, n, nrhs, B, Xin, ldxin, rows, nrows, pattern, itmax, Hd, z2, x2, false, nullptr)); }
extern "C" int hs_gn_diag_z(GN_DIAG_ARGS) { HS_GUARD(diag_entry<cplx>(F, trans, n, nrhs, B, (const cplx*)Xin, ldxin, rows, nrows, pattern, itmax, Hd, z2, x2, false, nullptr)); }
extern "C" int hs_gn_diag_dev_d(GN_DIAG_ARGS, void* stream) { HS_GUARD(diag_entry<double>(F, trans, n, nrhs, B, Xin, ldxin, rows, nrows, pattern, itmax, Hd, z2, x2, true, stream)); }
extern "C" int hs_gn_diag_dev_z(GN_DIAG_ARGS, void* stream) {
  HS_GUARD(diag_entry<cplx>(F, trans, n, nrhs, B, (const cplx*)Xin, ldxin, rows, nrows, pattern, itmax, Hd, z2, x2, true, stream));
}
extern "C" int hs_gn_info(const hs_handle* F, double* out8) {
  if (!F || !out8) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_gn_info: null argument");
    return HS_ERR_ARGUMENT;
  }
  memcpy(out8, hs_handle_gn_info(const_cast<hs_handle*>(F)), 8 * sizeof(double));
  return HS_OK;
}
