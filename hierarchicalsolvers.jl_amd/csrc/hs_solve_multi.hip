// hs_solve_multi.hip -- ldiv!(C, F, B) for an n x nrhs block with the factors read once per chunk of columns (hs_ldiv_block_*), and the
// same for transpose(F) / adjoint(F) (hs_ldiv_block_t_*): one driver, hs_solve_multi_run, whose trans argument picks the direction.
//
// The single-vector sweeps (kernels_solve_wide.hip) run at the HBM roofline, so k looped solves read the factors k times.  Here a chunk of
// KC columns (HS_LDIV_BLOCK_COLS = 16 / 32 / 48 / 64, default 32; the last chunk may be ragged) travels through the tree together; every
// step is one tall-skinny product on the matrix pipe (kernels_solve_multi.hip), grouped over the fronts of the level.  Per chunk:
//
//   forward, leaves -> root, per level:   W = (P B)[int, :],  Xb = B[bnd, :];   per 256-column block j:  Y_j = inv256L_j W_j,
//                                         W[below j] -= L[below, j] Y_j;   Xb -= Lbi Y  (low-rank fronts: -= C_L (Z_L Y));   B[bnd, :] = Xb
//   backward, root -> leaves, per level:  Xb = B[bnd, :];  W = Y - Uib Xb   (low-rank: - G (Z_R Xb));
//                                         per block j, last first:  X_j = inv256U_j W_j,  W[above j] -= U[above, j] X_j;   B[int, :] = X
//
// The triangular sweeps are RIGHT-looking (everything below / above a block is updated as soon as the block is solved): a step's product
// has (ni - 256 j) / 256 independent row tiles, so the top fronts fill the machine, and every output row has one fixed summation order.  The
// left-looking order would read Y once more but write W only once per block -- half the work-block traffic -- at the price of a product with
// 256 rows and K up to ni: one workgroup per front and step on the root (or a split K with a second reduction pass).  The boundary rows are
// NOT updated step by step (the sweeps of one vector do that): they take one product with K = ni after the triangle.  The caller's matrix is
// column-major and reached through the fronts' index lists; the products never see it: its rows are copied into row-major work blocks
// before (multi_move_kernel) and back after, once per front and sweep, so that the 16 columns a lane group of an MFMA tile reads or
// writes are adjacent (fronts of one level are disjoint, boundaries included -- hs_analyze checks it -- so the copies cannot collide).
//
// Work blocks, all row-major with a pitch of KC: W (largest level's sum of ni), Y (sum of ni over all fronts: y of every level is needed
// again on the way down), Xb (largest level's sum of nb), T (largest rank) for the low-rank products.  Taken from the library's scratch cache on first use, kept in the handle, freed by hs_free.  The single-vector workspaces and the
// exchange vectors of the dataflow sweeps are not touched.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hs_solve_multi.h"
#include "hs_f32.h"
#include "hs_interface.h"
#include "hs_lowrank.h"
#include "../../include/hs_solver.h"
#include "hs_host.h"

int hs_ldiv_block_cols() {
  static const int kc = [] {
    const char* e = getenv("HS_LDIV_BLOCK_COLS");
    const int v = e ? atoi(e) : 32;
    return (v == 16 || v == 32 || v == 48 || v == 64) ? v : 32;
  }();
  return kc;
}

namespace {
struct MultiCache {
  void *W1 = nullptr, *W2 = nullptr, *T1 = nullptr, *XB = nullptr;
  size_t b1 = 0, b2 = 0, bt = 0, bx = 0;
  MultiAux* d_aux = nullptr;      // per front, level after level (root first)
  std::vector<size_t> aux_off;    // first entry of every level
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool pending = false;  // the events of the last call have not been read yet
  double info[6] = {0, 0, 0, 0, 0, 0};
  // the last product with the factors (hs_mul_run): its own events and figures, so that it never shows as the handle's last block solve
  hipEvent_t m0 = nullptr, m1 = nullptr;
  bool mpending = false;
  double minfo[6] = {0, 0, 0, 0, 0, 0};
  ~MultiCache() {
    if (e1 && pending) (void)hipEventSynchronize(e1);
    if (m1 && mpending) (void)hipEventSynchronize(m1);
    if (m0) (void)hipEventDestroy(m0);
    if (m1) (void)hipEventDestroy(m1);
    if (W1) hs_scratch_give(W1, b1);
    if (W2) hs_scratch_give(W2, b2);
    if (T1) hs_scratch_give(T1, bt);
    if (XB) hs_scratch_give(XB, bx);
    if (d_aux) (void)hipFree(d_aux);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};
void free_cache(void* p) { delete (MultiCache*)p; }
MultiCache* cache_of(const HsMultiView& v) {
  if (!*v.mx) {
    *v.mx = new MultiCache();
    *v.mx_free = free_cache;
  }
  return (MultiCache*)*v.mx;
}
void ensure(void** p, size_t* have, size_t need, const char* what) {
  if (need <= *have) return;
  if (*p) hs_scratch_give(*p, *have);
  *p = nullptr;
  *have = 0;
  *p = hs_scratch_take(need, what);
  *have = need;
}

long long boff_of(const HsMultiLevel& L, int pos) {
  long long b = 0;
  for (int i = 0; i < pos; ++i) b += L.fronts[i].nb;
  return b;
}

struct FlopCount {
  double exec = 0.0, useful = 0.0;
  int tr, cmul;
  void add(double M, double K, int kc, double useful_mk = -1.0) {
    if (M <= 0 || kc <= 0) return;
    const double nt16 = (double)((kc + 15) / 16 * 16);
    exec += 2.0 * cmul * (std::ceil(M / tr) * tr) * (std::ceil(K / 16.0) * 16.0) * nt16;
    useful += 2.0 * cmul * (useful_mk >= 0 ? useful_mk : M * K) * kc;
  }
};

// t = Z x (r x kc, in T1), then dst -= C t with C dense or the unit trapezoid of the packed sketch; x, dst: rows of the work blocks
template <class T, class S>
void lr_apply(const LowRank<S>& lr, const T* x, T* dst, T* tbuf, int kcw, int kc, FlopCount& fc, hipStream_t s) {
  MultiProb<T, S> p;
  memset(&p, 0, sizeof p);
  p.A = lr.Z; p.lda = lr.ldz; p.M = lr.r; p.K = lr.cols;
  p.X = x; p.xrs = kcw;
  p.C = tbuf; p.crs = kcw;
  launch_multi_prob<T, S>(p, kc, s);
  fc.add(lr.r, lr.cols, kc);
  memset(&p, 0, sizeof p);
  if (lr.Cd) {
    p.A = lr.Cd; p.lda = lr.ldc;
  } else {
    p.A = lr.Lp; p.lda = lr.ldp; p.trap = 1; p.cmap = lr.rperm;
  }
  p.M = lr.rows; p.K = lr.r;
  p.X = tbuf; p.xrs = kcw;
  p.Cin = dst; p.C = dst; p.crs = kcw;
  launch_multi_prob<T, S>(p, kc, s);
  fc.add(lr.rows, lr.r, kc);
}

// the work blocks and the boundary segments of the handle, sized for a chunk of kcw columns (shared by both directions of the block solve)
template <class T, class S>
MultiCache* multi_prepare(const HsMultiView& v, int kcw) {
  MultiCache* mc = cache_of(v);
  long long wmax = 1, rmax = 1, bmax = 1;
  if (mc->aux_off.empty()) {  // the boundary segments of every level's fronts: fixed by the tree, uploaded once
    std::vector<MultiAux> aux;
    for (const HsMultiLevel& L : v.levels) {
      mc->aux_off.push_back(aux.size());
      long long boff = 0;
      for (const HsMultiFront& f : L.fronts) {
        aux.push_back({boff, f.nb, 0});
        boff += f.nb;
      }
    }
    aux.push_back({0, 0, 0});
    HS_HIP(hipMalloc((void**)&mc->d_aux, aux.size() * sizeof(MultiAux)));
    HS_HIP(hipMemcpy(mc->d_aux, aux.data(), aux.size() * sizeof(MultiAux), hipMemcpyHostToDevice));
  }
  for (const HsMultiLevel& L : v.levels) {
    wmax = std::max(wmax, L.wrows);
    long long bsum = 0;
    for (const HsMultiFront& f : L.fronts) bsum += f.nb;
    bmax = std::max(bmax, bsum);
    for (const HsMultiLR& q : L.lr) {
      if (q.lrL) rmax = std::max<long long>(rmax, ((const LowRank<S>*)q.lrL)->r);
      if (q.lrR) rmax = std::max<long long>(rmax, ((const LowRank<S>*)q.lrR)->r);
    }
  }
  if (mc->pending && mc->e1) (void)hipEventSynchronize(mc->e1);  // a call on another stream may still use the work blocks
  if (mc->mpending && mc->m1) (void)hipEventSynchronize(mc->m1);
  mc->pending = false;
  ensure(&mc->W1, &mc->b1, (size_t)wmax * kcw * sizeof(T), "block solve work block");
  ensure(&mc->W2, &mc->b2, (size_t)std::max<long long>(v.wtotal, 1) * kcw * sizeof(T), "block solve work block");
  ensure(&mc->T1, &mc->bt, (size_t)rmax * kcw * sizeof(T), "block solve low-rank intermediate");
  ensure(&mc->XB, &mc->bx, (size_t)bmax * kcw * sizeof(T), "block solve boundary block");
  if (!mc->e0) {
    HS_HIP(hipEventCreate(&mc->e0));
    HS_HIP(hipEventCreate(&mc->e1));
  }
  return mc;
}
// closes the timed region of a block solve and files its figures (hs_ldiv_block_info)
void multi_finish(MultiCache* mc, const HsMultiView& v, const FlopCount& fc, int chunks, size_t esz, hipStream_t s) {
  HS_HIP(hipEventRecord(mc->e1, s));
  HS_HIP(hipGetLastError());
  mc->pending = true;
  mc->info[0] = 0.0;
  mc->info[1] = (double)chunks * v.sum_fac * esz;
  mc->info[2] = fc.exec;
  mc->info[3] = fc.useful;
  mc->info[4] = (double)chunks;
  mc->info[5] = (double)(mc->b1 + mc->b2 + mc->bt + mc->bx);
}

// dst -= op(Z)^T (op(C)^T x): the transposed low-rank transform.  C dense, or the unit trapezoid of the packed sketch: C = P' trap(Lp), so
// C^T x = trap(Lp)^T (P x) -- the INPUT rows are gathered through rperm, where lr_apply scatters its output
template <class T, class S>
void lr_apply_t(const LowRank<S>& lr, int conj, const T* x, T* dst, T* tbuf, int kcw, int kc, FlopCount& fc, hipStream_t s) {
  MultiProbT<T, S> p;
  memset(&p, 0, sizeof p);
  if (lr.Cd) {
    p.A = lr.Cd; p.lda = lr.ldc;
  } else {
    p.A = lr.Lp; p.lda = lr.ldp; p.trap = 1; p.xmap = lr.rperm;
  }
  p.M = lr.r; p.K = lr.rows; p.conj = conj;
  p.X = x; p.xrs = kcw;
  p.C = tbuf; p.crs = kcw;
  launch_multi_prob_t<T, S>(p, kc, s);
  fc.add(lr.r, lr.rows, kc);
  memset(&p, 0, sizeof p);
  p.A = lr.Z; p.lda = lr.ldz; p.M = lr.cols; p.K = lr.r; p.conj = conj;
  p.X = tbuf; p.xrs = kcw;
  p.Cin = dst; p.C = dst; p.crs = kcw;
  launch_multi_prob_t<T, S>(p, kc, s);
  fc.add(lr.cols, lr.r, kc);
}

// what a level's grouped launches run over: the level's own arrays, or the compacted ones of an active set (hs_solve_multi.h)
struct LevelSel {
  const void* sn;
  const MultiAux* aux;
  int nf, maxni, maxnb;
  const std::vector<int>* pos;  // null: every front of the level
  bool has(int p) const { return !pos || std::binary_search(pos->begin(), pos->end(), p); }
};
LevelSel level_sel(const HsMultiLevel& L, const MultiAux* aux, const HsMultiActive* act, int chunk, int lv, int sweep) {
  if (!act) return {L.sn, aux, L.nfronts, L.maxni, L.maxnb, nullptr};
  const HsMultiSubset& q = act->at(chunk, lv, sweep);
  return {q.sn, q.aux, (int)q.pos.size(), q.maxni, q.maxnb, &q.pos};
}
template <class F>
void each_front(const HsMultiLevel& L, const LevelSel& q, F f) {
  if (!q.pos) {
    for (const HsMultiFront& x : L.fronts) f(x);
  } else {
    for (int p : *q.pos) f(L.fronts[p]);
  }
}

// HS_LDIV_BLOCK_T_LOOK = left selects the left-looking triangular sweeps of the transposed solve (a measurement switch; default: right)
bool multi_t_left_looking() {
  static const bool left = [] {
    const char* e = getenv("HS_LDIV_BLOCK_T_LOOK");
    return e && (e[0] == 'l' || e[0] == 'L');
  }();
  return left;
}

// the grouped launches of either direction: trans = 0 runs kernels_solve_multi.hip (mode n), trans = 1, 2 kernels_solve_multi_t.hip (mode t)
template <class T, class S>
void level_move(int trans, const SolveNode<S>* sn, int nf, int what, int maxrows, const MultiArgs& a, hipStream_t s) {
  launch_multi_move<T, S>(sn, nf, what, maxrows, a, s, trans ? 2 : 0);
}
template <class T, class S>
void level_step(int trans, int cj, const SolveNode<S>* sn, int nf, int mode_n, int mode_t, int blk, int maxM, const MultiArgs& a, hipStream_t s) {
  if (trans)
    launch_multi_level_t<T, S>(sn, nf, mode_t, blk, cj, maxM, a, s);
  else
    launch_multi_level<T, S>(sn, nf, mode_n, blk, maxM, a, s);
}
template <class T, class S>
void lr_apply_op(int trans, int cj, const LowRank<S>& lr, const T* x, T* dst, T* tbuf, int kcw, int kc, FlopCount& fc, hipStream_t s) {
  if (trans)
    lr_apply_t<T, S>(lr, cj, x, dst, tbuf, kcw, kc, fc, s);
  else
    lr_apply<T, S>(lr, x, dst, tbuf, kcw, kc, fc, s);
}

// op(F) \ B with op = identity (trans = 0), transpose (1) or adjoint (2): the same chunks, work blocks and stored blocks.  trans = 0 is the
// schedule at the head of this file.  trans = 1, 2 run every product with the factor panel transposed (kernels_solve_multi_t.hip), U and L
// changing places; op(x) = x or conj(x) (trans = 2: the factor entries are conjugated as they are loaded).  Per chunk:
//
//   forward, leaves -> root, per level:   W = B[int, :] (no permutation),  Xb = B[bnd, :];   per 256-block j:  Z_j = op(inv256U_j)^T W_j,
//                                         W[below j] -= op(U11[j, below])^T Z_j;   Xb -= op(Uib)^T Z  (low-rank: -= op(Z_R)^T (op(G)^T Z));
//                                         B[bnd, :] = Xb
//   backward, root -> leaves, per level:  Xb = B[bnd, :];  W = Z - op(Lbi)^T Xb   (low-rank: - op(Z_L)^T (op(C_L)^T Xb));
//                                         per block j, last first:  X_j = op(inv256L_j)^T W_j,  W[above j] -= op(L11[j, above])^T X_j;
//                                         B[int[rperm[i]], :] = X[i, :]
//
// Right-looking like the forward solve: the update of a step reads the ROW panel U11[j, below] / L11[j, above] -- 256 contiguous doubles
// per output row -- and has (ni - 256 (j + 1)) / 64 workgroups.  The left-looking order (HS_LDIV_BLOCK_T_LOOK=left, trans = 1, 2 only) reads the
// column panel above / below the block with K up to ni and 256 outputs: W is written once per block, by four workgroups per front
// (DESIGN.md section 4a⁗″).
//
// S: the scalar the factors are stored in (hs_solve_multi.h).  A demoted copy (S != T) has no active set, no phases and no HSS fronts.
template <class T, class S>
void multi_run(const HsMultiView& v, int trans, T* dC, int64_t ldc, int64_t nrhs, hipStream_t s, const HsMultiActive* act, int phase) {
  constexpr bool OWN = std::is_same<T, S>::value;
  const int KC = hs_ldiv_block_cols();
  const int kcw = KC;
  const int cj = (trans == 2 && sizeof(T) == 16) ? 1 : 0;
  const bool left = trans && multi_t_left_looking();
  MultiCache* mc = multi_prepare<T, S>(v, kcw);
  FlopCount fc;
  fc.tr = hs_multi_rows_per_wg(sizeof(T) == 16);
  fc.cmul = sizeof(T) == 16 ? 4 : 1;
  const int nl = (int)v.levels.size();
  int chunks = 0;
  HS_HIP(hipEventRecord(mc->e0, s));
  for (int64_t c0 = 0; c0 < nrhs; c0 += KC, ++chunks) {
    const int kc = (int)std::min<int64_t>(KC, nrhs - c0);
    MultiArgs a;
    a.W1 = mc->W1; a.W2 = mc->W2; a.XB = mc->XB; a.kcw = kcw;
    a.B = act ? dC : dC + c0 * ldc; a.ldb = ldc; a.kc = kc;  // an active set keeps every chunk in the same block
    if (act && act->begin) act->begin(act->ctx, chunks, kc, s);
    for (int lv = nl - 1; lv >= 0; --lv) {  // leaves -> root
      if (phase == HS_MULTI_EXPAND || (phase == HS_MULTI_CONDENSE && lv == 0) || (phase == HS_MULTI_ROOT && lv != 0)) continue;
      const HsMultiLevel& L = v.levels[lv];
      if (v.hss_front && !act)  // fronts with an HSS interior block (disjoint from the level's other fronts): on the caller's block
        for (int id : L.hss) v.hss_front(v.hss_ctx, id, 0, trans, a.B, a.ldb, kc, s);
      if (L.nfronts == 0 || L.maxni == 0) continue;
      const LevelSel q_ = level_sel(L, mc->d_aux + mc->aux_off[lv], act, chunks, lv, 0);
      if (q_.nf == 0 || q_.maxni == 0) continue;
      const SolveNode<S>* sn = (const SolveNode<S>*)q_.sn;
      const int nf = q_.nf, maxni = q_.maxni, maxnb = q_.maxnb;
      a.wbase = L.wbase;
      a.aux = q_.aux;
      level_move<T, S>(trans, sn, nf, 0, maxni, a, s);
      level_move<T, S>(trans, sn, nf, 1, maxnb, a, s);
      const int nblk = (maxni + 255) / 256;
      for (int j = 0; j < nblk; ++j) {
        const int wl = std::min(256, maxni - j * 256);
        if (left && j > 0) launch_multi_level_t<T, S>(sn, nf, HSMT_LEFT_U, j, cj, wl, a, s);
        level_step<T, S>(trans, cj, sn, nf, HSM_DIAG_L, HSMT_DIAG_U, j, wl, a, s);
        if (!left) level_step<T, S>(trans, cj, sn, nf, HSM_BELOW_L, HSMT_BELOW_U, j, maxni - (j + 1) * 256, a, s);
      }
      level_step<T, S>(trans, cj, sn, nf, HSM_BND_L, HSMT_BND_U, 0, maxnb, a, s);
      each_front(L, q_, [&](const HsMultiFront& f) {
        for (int j = 0; j * 256 < f.ni; ++j) {
          const double wl = std::min(256, f.ni - j * 256);
          fc.add(wl, wl, kc, wl * (wl + 1) / 2);
          if (left)
            fc.add(wl, j * 256, kc);
          else
            fc.add(f.ni - (j + 1) * 256, 256, kc);
        }
        if (f.dense_bnd) fc.add(f.nb, f.ni, kc);
      });
      for (const HsMultiLR& q : L.lr) {  // the transform of this sweep: Lbi, transposed Uib
        const void* tr = trans ? q.lrR : q.lrL;
        if (!tr || !q_.has(q.pos)) continue;
        const LowRank<S>& lr = *(const LowRank<S>*)tr;
        if (lr.r == 0) continue;
        lr_apply_op<T, S>(trans, cj, lr, (const T*)mc->W2 + q.woff * kcw, (T*)mc->XB + boff_of(L, q.pos) * kcw, (T*)mc->T1, kcw, kc, fc, s);
      }
      level_move<T, S>(trans, sn, nf, 3, maxnb, a, s);
      if constexpr (OWN)
        if (phase == HS_MULTI_CONDENSE) launch_interface_park<T>(sn, nf, 0, maxni, a, s);  // C[int, :] = y
    }
    if (act && act->zoff[chunks + 1] > act->zoff[chunks])  // backward-only fronts: y = 0
      launch_sparse_zero<T>((T*)mc->W2, kcw, kc, act->zseg + act->zoff[chunks], (int)(act->zoff[chunks + 1] - act->zoff[chunks]), act->zmaxni[chunks], s);
    for (int lv = 0; lv < nl; ++lv) {  // root -> leaves
      if (phase == HS_MULTI_CONDENSE || (phase == HS_MULTI_EXPAND && lv == 0) || (phase == HS_MULTI_ROOT && lv != 0)) continue;
      const HsMultiLevel& L = v.levels[lv];
      if (v.hss_front && !act)
        for (int id : L.hss) v.hss_front(v.hss_ctx, id, 1, trans, a.B, a.ldb, kc, s);
      if (L.nfronts == 0 || L.maxni == 0) continue;
      const LevelSel q_ = level_sel(L, mc->d_aux + mc->aux_off[lv], act, chunks, lv, 1);
      if (q_.nf == 0 || q_.maxni == 0) continue;
      const SolveNode<S>* sn = (const SolveNode<S>*)q_.sn;
      const int nf = q_.nf, maxni = q_.maxni, maxnb = q_.maxnb;
      a.wbase = L.wbase;
      a.aux = q_.aux;
      if constexpr (OWN)
        if (phase == HS_MULTI_EXPAND) launch_interface_park<T>(sn, nf, 1, maxni, a, s);  // y = C[int, :]
      level_move<T, S>(trans, sn, nf, 1, maxnb, a, s);
      level_step<T, S>(trans, cj, sn, nf, HSM_UR, HSMT_LB, 0, maxni, a, s);
      for (const HsMultiLR& q : L.lr) {  // Uib, transposed Lbi
        const void* tr = trans ? q.lrL : q.lrR;
        if (!tr || !q_.has(q.pos)) continue;
        const LowRank<S>& lr = *(const LowRank<S>*)tr;
        if (lr.r == 0) continue;
        lr_apply_op<T, S>(trans, cj, lr, (const T*)mc->XB + boff_of(L, q.pos) * kcw, (T*)mc->W1 + (q.woff - L.wbase) * kcw, (T*)mc->T1, kcw, kc, fc, s);
      }
      const int nblk = (maxni + 255) / 256;
      for (int j = nblk - 1; j >= 0; --j) {
        const int wl = std::min(256, maxni - j * 256);
        if (left) launch_multi_level_t<T, S>(sn, nf, HSMT_LEFT_L, j, cj, 256, a, s);
        level_step<T, S>(trans, cj, sn, nf, HSM_DIAG_U, HSMT_DIAG_L, j, wl, a, s);
        if (!left) level_step<T, S>(trans, cj, sn, nf, HSM_ABOVE_U, HSMT_ABOVE_L, j, j * 256, a, s);
      }
      level_move<T, S>(trans, sn, nf, 2, maxni, a, s);
      each_front(L, q_, [&](const HsMultiFront& f) {
        if (f.dense_bnd) fc.add(f.ni, f.nb, kc);
        for (int j = 0; j * 256 < f.ni; ++j) {
          const double wl = std::min(256, f.ni - j * 256);
          fc.add(wl, wl, kc, wl * (wl + 1) / 2);
          if (left)
            fc.add(wl, std::max(f.ni - (j + 1) * 256, 0), kc);
          else
            fc.add(j * 256, wl, kc);
        }
      });
    }
    if (act && act->end) act->end(act->ctx, chunks, kc, s);
  }
  multi_finish(mc, v, fc, chunks, sizeof(S), s);
}

// ---- C = op(F) B: the stored factorization applied as an operator (hs_mul_*) ---------------------------------------------------------------
// F = P' L U front by front, so with Y_f an intermediate per front (work block 2 holds one segment per front) a chunk of columns takes two
// passes over the tree and no triangular solve:
//
//   trans = 0   U pass, every front on its own:   Y_f = triu(U11) X[int] + Uib X[bnd]                 (low-rank fronts: + G (Z_R X[bnd]))
//               L pass, root -> leaves:           B[int[rperm]] = unit-tril(L11) Y_f,  B[bnd] += Lbi Y_f      (+= C_L (Z_L Y_f))
//   trans = 1,2 first pass, every front:          Z_f = op(L11)^T X[int[rperm]] + op(Lbi)^T X[bnd]     (+ op(Z_L)^T (op(C_L)^T X[bnd]))
//               second pass, root -> leaves:      B[int] = op(U11)^T Z_f,  B[bnd] += op(Uib)^T Z_f            (+= op(Z_R)^T (op(G)^T Z_f))
//
// The first pass reads X only (it runs level by level on the stream because the levels share work block 1 and the boundary block, in the
// order of the loop below, but no level waits for another's result); it has consumed all of X before the second writes a row, so the
// product is in place.  The second pass sets the interior rows of a front and ADDS into its boundary rows, which are interior rows of its
// ancestors: root first, one stream, so every row is set once and then takes its additions in one fixed order.  Per level and pass: the two
// moves, the triangle, the boundary product (the trapezoid [L11; Lbi] is one product), the low-rank pairs.
template <class T>
void lr_mul(const LowRank<T>& lr, const T* x, T* dst, T* tbuf, int kcw, int kc, FlopCount& fc, hipStream_t s) {  // dst += C (Z x)
  MultiProb<T, T> q;
  memset(&q, 0, sizeof q);
  q.A = lr.Z; q.lda = lr.ldz; q.M = lr.r; q.K = lr.cols;
  q.X = x; q.xrs = kcw;
  q.C = tbuf; q.crs = kcw;
  launch_multi_prob<T, T>(q, kc, s);
  fc.add(lr.r, lr.cols, kc);
  MultiProbMul<T, T> p;
  memset(&p, 0, sizeof p);
  if (lr.Cd) {
    p.A = lr.Cd; p.lda = lr.ldc;
  } else {
    p.A = lr.Lp; p.lda = lr.ldp; p.trap = 1; p.cmap = lr.rperm;
  }
  p.M = lr.rows; p.K = lr.r;
  p.X = tbuf; p.xrs = kcw;
  p.Cin = dst; p.C = dst; p.crs = kcw;
  launch_mul_prob<T>(p, kc, s);
  fc.add(lr.rows, lr.r, kc);
}
template <class T>
void lr_mul_t(const LowRank<T>& lr, int conj, const T* x, T* dst, T* tbuf, int kcw, int kc, FlopCount& fc, hipStream_t s) {  // dst += op(Z)^T (op(C)^T x)
  MultiProbT<T, T> q;
  memset(&q, 0, sizeof q);
  if (lr.Cd) {
    q.A = lr.Cd; q.lda = lr.ldc;
  } else {
    q.A = lr.Lp; q.lda = lr.ldp; q.trap = 1; q.xmap = lr.rperm;
  }
  q.M = lr.r; q.K = lr.rows; q.conj = conj;
  q.X = x; q.xrs = kcw;
  q.C = tbuf; q.crs = kcw;
  launch_multi_prob_t<T, T>(q, kc, s);
  fc.add(lr.r, lr.rows, kc);
  MultiProbMulT<T, T> p;
  memset(&p, 0, sizeof p);
  p.A = lr.Z; p.lda = lr.ldz; p.M = lr.cols; p.K = lr.r; p.conj = conj;
  p.X = tbuf; p.xrs = kcw;
  p.Cin = dst; p.C = dst; p.crs = kcw;
  launch_mul_prob_t<T>(p, kc, s);
  fc.add(lr.cols, lr.r, kc);
}
// executed flops of a triangular ni x ni product whose workgroups read the chunks that meet their rows only
void add_tri(FlopCount& fc, int ni, int kc) {
  if (ni <= 0) return;
  const double nt16 = (double)((kc + 15) / 16 * 16);
  double cols = 0.0;
  for (int r0 = 0; r0 < ni; r0 += fc.tr) cols += std::min((r0 + fc.tr + 15) / 16 * 16, (ni + 15) / 16 * 16);
  fc.exec += 2.0 * fc.cmul * fc.tr * cols * nt16;
  fc.useful += 2.0 * fc.cmul * (0.5 * ni * (ni + 1.0)) * kc;
}

template <class T>
void mul_run(const HsMultiView& v, int trans, T* dC, int64_t ldc, int64_t nrhs, hipStream_t s) {
  const int KC = hs_ldiv_block_cols();
  const int kcw = KC;
  const int cj = (trans == 2 && sizeof(T) == 16) ? 1 : 0;
  if (*v.mx) (void)hs_solve_multi_seconds(*v.mx);  // the last block solve keeps its seconds: multi_prepare closes its events
  MultiCache* mc = multi_prepare<T, T>(v, kcw);
  if (!mc->m0) {
    HS_HIP(hipEventCreate(&mc->m0));
    HS_HIP(hipEventCreate(&mc->m1));
  }
  FlopCount fc;
  fc.tr = hs_multi_rows_per_wg(sizeof(T) == 16);
  fc.cmul = sizeof(T) == 16 ? 4 : 1;
  const int nl = (int)v.levels.size();
  int chunks = 0;
  HS_HIP(hipEventRecord(mc->m0, s));
  for (int64_t c0 = 0; c0 < nrhs; c0 += KC, ++chunks) {
    const int kc = (int)std::min<int64_t>(KC, nrhs - c0);
    MultiArgs a;
    a.W1 = mc->W1; a.W2 = mc->W2; a.XB = mc->XB; a.kcw = kcw;
    a.B = dC + c0 * ldc; a.ldb = ldc; a.kc = kc;
    for (int pass = 0; pass < 2; ++pass)
      for (int lv = 0; lv < nl; ++lv) {  // (the first pass may take its levels in any order; the second: root first)
        const HsMultiLevel& L = v.levels[lv];
        if (L.nfronts == 0 || L.maxni == 0) continue;
        const SolveNode<T>* sn = (const SolveNode<T>*)L.sn;
        const int nf = L.nfronts, maxni = L.maxni, maxnb = L.maxnb;
        a.wbase = L.wbase;
        a.aux = mc->d_aux + mc->aux_off[lv];
        T* w1 = (T*)mc->W1;
        T* w2 = (T*)mc->W2;
        T* xb = (T*)mc->XB;
        launch_multi_move<T, T>(sn, nf, 1, maxnb, a, s, 0);  // Xb = X[bnd] (first pass), B[bnd] as it stands (second)
        if (pass == 0) {
          // W = X[int] (trans = 0) or X[int[rperm]] (trans = 1, 2): move 0 goes through rperm when it is the permuted one
          launch_multi_move<T, T>(sn, nf, 0, maxni, a, s, trans ? 0 : 2);
          if (!trans) {
            launch_mul_level<T>(sn, nf, HSMM_TRIU, maxni, a, s);
            launch_mul_level<T>(sn, nf, HSMM_UR, maxni, a, s);
          } else {
            launch_mul_level_t<T>(sn, nf, HSMMT_TRAP, cj, maxni, a, s);
          }
          for (const HsMultiLR& q : L.lr) {
            const void* tr = trans ? q.lrL : q.lrR;
            if (!tr) continue;
            const LowRank<T>& lr = *(const LowRank<T>*)tr;
            if (lr.r == 0) continue;
            if (!trans)
              lr_mul<T>(lr, xb + boff_of(L, q.pos) * kcw, w2 + q.woff * kcw, (T*)mc->T1, kcw, kc, fc, s);
            else
              lr_mul_t<T>(lr, cj, xb + boff_of(L, q.pos) * kcw, w2 + q.woff * kcw, (T*)mc->T1, kcw, kc, fc, s);
          }
        } else {
          if (!trans) {
            launch_mul_level<T>(sn, nf, HSMM_TRAP, maxni + maxnb, a, s);
          } else {
            launch_mul_level_t<T>(sn, nf, HSMMT_TRIU, cj, maxni, a, s);
            launch_mul_level_t<T>(sn, nf, HSMMT_BND_U, cj, maxnb, a, s);
          }
          for (const HsMultiLR& q : L.lr) {
            const void* tr = trans ? q.lrR : q.lrL;
            if (!tr) continue;
            const LowRank<T>& lr = *(const LowRank<T>*)tr;
            if (lr.r == 0) continue;
            if (!trans)
              lr_mul<T>(lr, w2 + q.woff * kcw, xb + boff_of(L, q.pos) * kcw, (T*)mc->T1, kcw, kc, fc, s);
            else
              lr_mul_t<T>(lr, cj, w2 + q.woff * kcw, xb + boff_of(L, q.pos) * kcw, (T*)mc->T1, kcw, kc, fc, s);
          }
          // B[int[rperm]] (trans = 0) or B[int] = W: move 2 reads the segment at woff of "work block 2", which is given as the level's work
          // block 1 shifted back by the level's base
          MultiArgs m = a;
          m.W2 = w1 - L.wbase * kcw;
          launch_multi_move<T, T>(sn, nf, 2, maxni, m, s, trans ? 0 : 2);
          launch_multi_move<T, T>(sn, nf, 3, maxnb, a, s, 0);
        }
        for (const HsMultiFront& f : L.fronts) {
          add_tri(fc, f.ni, kc);
          if (f.dense_bnd) fc.add(pass == 0 ? f.ni : f.nb, pass == 0 ? f.nb : f.ni, kc);
        }
      }
  }
  HS_HIP(hipEventRecord(mc->m1, s));
  HS_HIP(hipGetLastError());
  mc->mpending = true;
  mc->minfo[0] = 0.0;
  mc->minfo[1] = (double)chunks * v.sum_fac * sizeof(T);
  mc->minfo[2] = fc.exec;
  mc->minfo[3] = fc.useful;
  mc->minfo[4] = (double)chunks;
  mc->minfo[5] = (double)(mc->b1 + mc->b2 + mc->bt + mc->bx);
}
}  // namespace

template <class T>
void hs_mul_run(const HsMultiView& v, int trans, T* dC, int64_t ldc, int64_t nrhs, hipStream_t s) {
  mul_run<T>(v, trans, dC, ldc, nrhs, s);
}
template void hs_mul_run<double>(const HsMultiView&, int, double*, int64_t, int64_t, hipStream_t);
template void hs_mul_run<cplx>(const HsMultiView&, int, cplx*, int64_t, int64_t, hipStream_t);
void hs_mul_figures(void* mx, double* out6) {
  MultiCache* mc = (MultiCache*)mx;
  if (mc && mc->mpending) {
    float ms = 0.f;
    if (hipEventSynchronize(mc->m1) == hipSuccess && hipEventElapsedTime(&ms, mc->m0, mc->m1) == hipSuccess) mc->minfo[0] = ms * 1e-3;
    mc->mpending = false;
  }
  for (int k = 0; k < 6; ++k) out6[k] = mc ? mc->minfo[k] : 0.0;
}

template <class T>
void hs_solve_multi_run(const HsMultiView& v, int trans, T* dC, int64_t ldc, int64_t nrhs, hipStream_t s, const HsMultiActive* act, int phase) {
  multi_run<T, T>(v, trans, dC, ldc, nrhs, s, act, phase);
}
template <class T>
void hs_solve_multi_run_f32(const HsMultiView& v, int trans, T* dC, int64_t ldc, int64_t nrhs, hipStream_t s) {
  multi_run<T, typename F32Of<T>::type>(v, trans, dC, ldc, nrhs, s, nullptr, HS_MULTI_ALL);
}
template void hs_solve_multi_run_f32<double>(const HsMultiView&, int, double*, int64_t, int64_t, hipStream_t);
template void hs_solve_multi_run_f32<cplx>(const HsMultiView&, int, cplx*, int64_t, int64_t, hipStream_t);
template void hs_solve_multi_run<double>(const HsMultiView&, int, double*, int64_t, int64_t, hipStream_t, const HsMultiActive*, int);
template void hs_solve_multi_run<cplx>(const HsMultiView&, int, cplx*, int64_t, int64_t, hipStream_t, const HsMultiActive*, int);

double hs_solve_multi_seconds(void* mx) {
  MultiCache* mc = (MultiCache*)mx;
  if (!mc) return 0.0;
  if (mc->pending) {
    float ms = 0.f;
    if (hipEventSynchronize(mc->e1) == hipSuccess && hipEventElapsedTime(&ms, mc->e0, mc->e1) == hipSuccess) mc->info[0] = ms * 1e-3;
    mc->pending = false;
  }
  return mc->info[0];
}
void hs_solve_multi_info(void* mx, double* out6) {
  MultiCache* mc = (MultiCache*)mx;
  if (mc) (void)hs_solve_multi_seconds(mx);
  for (int k = 0; k < 6; ++k) out6[k] = mc ? mc->info[k] : 0.0;
}
