// hs_selinv.hip -- log|det| and selected inversion from the stored factors (include/hs_solver.h: hs_logabsdet, hs_selinv, hs_selinv_info, hs_selinv_lr, hs_selinv_lr_info).
//
// det.  Every front keeps P Aii = L U, and the Gauss transforms between fronts are unit block-triangular, so
//   det(F) = prod over fronts of sign(P) * prod diag(U).
// One grouped launch (logdet_kernel, one workgroup per front) reduces log|u_kk|, the phase and the parity of P per front in a fixed order;
// the host adds the per-front results in post-order.  Nothing but the diagonals and the permutations is read.
//
// Selected inversion (exact factorizations: every front dense).  With Z = A^-1 and Zbb = Z[bnd, bnd] of a front known,
//   Z[int, bnd] = -R Zbb,   Z[bnd, int] = -Zbb Lm,   Z[int, int] = Aii^-1 + R Zbb Lm,      R = U^-1 Uib,  Lm = Lbi L^-1 P.
// A child's boundary is a subset of its parent's front, so its Zbb is a gather from the parent's finished block: the tree is walked from
// the root to the leaves, the fronts of a level batched like the factorization batches them.  Per batch, with m = ni + nb:
//   Vb  = -Uib Zbb                      (GEMM)            Z[int, bnd] = U^-1 Vb         (blocked back substitution, below)
//   Vi  = I                                               Tm[int, :]  = U^-1 Vi = U^-1  (the same launches; only the upper triangle is computed)
//   Tm -= Z[:, bnd] Lbi                 (GEMM, m x ni)    now Tm = [U^-1; 0] - [Zib; Zbb] Lbi
//   X2  = Tm L^-1                       (blocked substitution from the right)
//   Z[:, rperm[i]] = X2[:, i]           (zpermute_cols: the trailing P)  -> Z[:, int] = [Zii; Zbi]
// The triangular solves run over the stored inverses of the 256 x 256 diagonal blocks (inv256L / inv256U, which every factorization leaves
// behind for ldiv!): per block one product with the inverse and one update product, all of them GemmProb lists for launch_gemm_probs.
// About 4/3 ni^3 + 4 ni^2 nb + 4 ni nb^2 flops per front.  The stored factors are only read.
//
// Memory.  A batch holds the m x m blocks of its fronts and 2 m ni work elements per front (the Schur scratch of the handle serves as work
// space when it is idle).  A parent batch's blocks live until the last batch of its children has gathered from them; a level that does not
// fit the byte budget is cut into several batches of fronts, each followed by its own subtree before the next one starts.
//
// Compressed factorizations (hs_selinv_lr, hs_selinv_lr_info).  A compressed front keeps Uib ~= G Z_R and Lbi ~= C_L Z_L' (hs_compress.h) and
// the pivoted LU of Aii; the same recurrence runs through the r-wide factors (the comment at SelRun), the operator the block solves apply,
// so the result is F^-1 to rounding.  Dense and low-rank fronts share a batch's launches.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "../../include/hs_hss.h"
#include "../../include/hs_solver.h"
#include "hs_common.h"
#include "hs_host.h"
#include "hs_lowrank.h"
#include "hs_selinv.h"

namespace {

inline int rup2(int x) { return (std::max(x, 1) + 1) / 2 * 2; }
inline size_t rup32(size_t x) { return (x + 31) / 32 * 32; }

// What the first hs_selinv call of a handle builds and keeps: which front owns which stored entry of A, and where every front's boundary
// sits in its parent's front.  Both depend on the pattern and the tree only.
struct SelCache {
  bool built = false;
  long long hole = -1;      // first stored entry of A (CSC position) that lies in no front's [int; bnd] x [int; bnd] block, -1: none
  int hole_front = -1;      // first front with a boundary DOF its parent's front does not hold, -1: none
  std::vector<int64_t> eptr;   // per front: range of its entries in the three arrays below
  std::vector<size_t> cmoff;   // per front: offset of its cmap
  int* d_epr = nullptr;
  int* d_epc = nullptr;
  int64_t* d_ee = nullptr;
  int* d_cmap = nullptr;
  double info[4] = {0, 0, 0, 0};  // last call: seconds, flops, peak scratch bytes, batches
  double info_lr[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // last hs_selinv_lr call (hs_selinv_lr_info); neither call touches the other's figures
  ~SelCache() {
    if (d_epr) (void)hipFree(d_epr);
    if (d_epc) (void)hipFree(d_epc);
    if (d_ee) (void)hipFree(d_ee);
    if (d_cmap) (void)hipFree(d_cmap);
  }
};
void free_cache(void* p) { delete (SelCache*)p; }

SelCache* cache_of(const HsSelView& v) {
  if (!*v.sx) {
    *v.sx = new SelCache();
    *v.sx_free = free_cache;
  }
  return (SelCache*)*v.sx;
}

void build_cache(const HsSelView& v, SelCache* c) {
  const int nf = (int)v.fronts.size();
  const int64_t n = v.n, nnz = v.nnz;
  std::vector<int64_t> cp((size_t)n + 1);
  std::vector<int32_t> rv((size_t)std::max<int64_t>(nnz, 1));
  HS_HIP(hipMemcpy(cp.data(), v.colptr, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (nnz) HS_HIP(hipMemcpy(rv.data(), v.rowval, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
  // the front that eliminates each DOF
  std::vector<int> elim((size_t)n, -1);
  for (int f = 0; f < nf; ++f) {
    const HsSelFront& x = v.fronts[f];
    const int* ids = v.fidx_host + x.off_fidx_host;
    for (int i = 0; i < x.ni; ++i) elim[(size_t)ids[i]] = f;
  }
  // owner of a stored entry (r, c): the front that eliminates whichever of r, c goes first.  The two fronts lie on one path to the root
  // when the tree fits the pattern, and the deeper one is eliminated first.
  std::vector<int> owner((size_t)std::max<int64_t>(nnz, 1), -1);
  c->eptr.assign((size_t)nf + 1, 0);
  for (int64_t col = 0; col < n && c->hole < 0; ++col)
    for (int64_t e = cp[col]; e < cp[col + 1]; ++e) {
      const int fr = elim[(size_t)rv[e]], fc = elim[(size_t)col];
      if (fr < 0 || fc < 0 || (fr != fc && v.fronts[fr].level == v.fronts[fc].level)) {
        c->hole = e;
        break;
      }
      const int o = v.fronts[fr].level >= v.fronts[fc].level ? fr : fc;
      owner[(size_t)e] = o;
      c->eptr[(size_t)o + 1]++;
    }
  std::vector<int> epr((size_t)std::max<int64_t>(nnz, 1)), epc((size_t)std::max<int64_t>(nnz, 1));
  std::vector<int64_t> ee((size_t)std::max<int64_t>(nnz, 1));
  std::vector<int> pos((size_t)n, -1);
  if (c->hole < 0) {
    for (int f = 0; f < nf; ++f) c->eptr[(size_t)f + 1] += c->eptr[(size_t)f];
    std::vector<int64_t> fill(c->eptr.begin(), c->eptr.end() - 1);
    std::vector<int64_t> ecol((size_t)std::max<int64_t>(nnz, 1));
    for (int64_t col = 0; col < n; ++col)
      for (int64_t e = cp[col]; e < cp[col + 1]; ++e) {
        const int64_t k = fill[(size_t)owner[(size_t)e]]++;
        ee[(size_t)k] = e;
        ecol[(size_t)k] = col;
      }
    for (int f = 0; f < nf && c->hole < 0; ++f) {
      const HsSelFront& x = v.fronts[f];
      const int* ids = v.fidx_host + x.off_fidx_host;
      const int m = x.ni + x.nb;
      for (int i = 0; i < m; ++i) pos[(size_t)ids[i]] = i;
      for (int64_t k = c->eptr[f]; k < c->eptr[(size_t)f + 1]; ++k) {
        const int pr = pos[(size_t)rv[(size_t)ee[(size_t)k]]], pc = pos[(size_t)ecol[(size_t)k]];
        if (pr < 0 || pc < 0) {
          c->hole = ee[(size_t)k];
          break;
        }
        epr[(size_t)k] = pr;
        epc[(size_t)k] = pc;
      }
      for (int i = 0; i < m; ++i) pos[(size_t)ids[i]] = -1;
    }
  }
  // position of every front's boundary in its parent's front, by global id
  c->cmoff.assign((size_t)nf + 1, 0);
  for (int f = 0; f < nf; ++f) c->cmoff[(size_t)f + 1] = c->cmoff[(size_t)f] + (size_t)v.fronts[f].nb;
  std::vector<int> cm(std::max<size_t>(c->cmoff[(size_t)nf], 1), 0);
  std::vector<std::vector<int>> kids((size_t)nf);
  for (int f = 0; f < nf; ++f)
    if (v.fronts[f].parent >= 0) kids[(size_t)v.fronts[f].parent].push_back(f);
  for (int p = 0; p < nf; ++p) {
    if (kids[(size_t)p].empty()) continue;
    const HsSelFront& x = v.fronts[p];
    const int* ids = v.fidx_host + x.off_fidx_host;
    const int m = x.ni + x.nb;
    for (int i = 0; i < m; ++i) pos[(size_t)ids[i]] = i;
    for (int f : kids[(size_t)p]) {
      const HsSelFront& y = v.fronts[f];
      const int* cid = v.fidx_host + y.off_fidx_host + y.ni;
      for (int a = 0; a < y.nb; ++a) {
        const int q = pos[(size_t)cid[a]];
        if (q < 0 && c->hole_front < 0) c->hole_front = f;
        cm[c->cmoff[(size_t)f] + (size_t)a] = std::max(q, 0);
      }
    }
    for (int i = 0; i < m; ++i) pos[(size_t)ids[i]] = -1;
  }
  for (int f = 0; f < nf; ++f)  // only a root may keep a boundary nobody hands it
    if (v.fronts[f].parent < 0 && v.fronts[f].nb > 0 && c->hole_front < 0) c->hole_front = f;
  if (c->hole < 0 && c->hole_front < 0) {
    const size_t ne = (size_t)std::max<int64_t>(nnz, 1);
    HS_HIP(hipMalloc((void**)&c->d_epr, ne * sizeof(int)));
    HS_HIP(hipMalloc((void**)&c->d_epc, ne * sizeof(int)));
    HS_HIP(hipMalloc((void**)&c->d_ee, ne * sizeof(int64_t)));
    HS_HIP(hipMalloc((void**)&c->d_cmap, cm.size() * sizeof(int)));
    HS_HIP(hipMemcpy(c->d_epr, epr.data(), ne * sizeof(int), hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(c->d_epc, epc.data(), ne * sizeof(int), hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(c->d_ee, ee.data(), ne * sizeof(int64_t), hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(c->d_cmap, cm.data(), cm.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  c->built = true;
}

// ---- checks shared by the entry points: everything here happens before any device work ---------------------------------------------
// ulv_ok: the caller serves fronts whose D is an eliminated HSS matrix when the handle's hs_ulv_mode is 1 (hs_logabsdet only)
void check_common(hs_handle* F, HsSelView& v, const char* fn, bool ulv_ok = false) {
  if (!F) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null factorization handle", fn);
  hs_selinv_view(F, &v);
  if (v.nranks > 1)
    HS_FAIL(HS_ERR_UNSUPPORTED, v.nranks, "%s: the factorization is spread over %d ranks; this call needs all fronts in one process", fn, v.nranks);
  if (!v.device || !v.factored) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s needs a completed numeric factorization (the handle is a plan, or hs_numeric_end has not run)", fn);
  for (size_t i = 0; i < v.fronts.size(); ++i) {
    if (!(v.fronts[i].flags & HS_SEL_NOLU)) continue;
    if (ulv_ok && v.ulv_mode == 1) {
      if (!v.fronts[i].hss || (v.fronts[i].mfb && !v.fronts[i].hss2))
        HS_FAIL(HS_ERR_UNSUPPORTED, (long long)i, "%s: front %d has no eliminated interior block (incomplete factorization)", fn, (int)i);
      continue;
    }
    HS_FAIL(HS_ERR_UNSUPPORTED, (long long)i, "%s: front %d keeps its interior block D as an HSS matrix (ULV factors; hs_options.hss_d, mf = 2, 3): it has no pivoted LU whose diagonal could be read", fn, (int)i);
  }
}

// ---- log-determinant ------------------------------------------------------------------------------------------------------------------
template <class T>
void logabsdet_impl(const HsSelView& v, double* logabs, double* sign2) {
  std::vector<LogdetFront> lf;
  for (const HsSelFront& x : v.fronts)
    if (x.ni > 0 && !(x.flags & HS_SEL_NOLU)) lf.push_back(LogdetFront{x.LU, x.rperm, x.ni, x.ldlu});
  const int nf = (int)lf.size();
  LogdetAcc acc;
  if (nf > 0) {
    HsScratch din, dout;
    din.take(sizeof(LogdetFront) * (size_t)nf, "log-determinant descriptors");
    dout.take(sizeof(LogdetOut) * (size_t)nf, "log-determinant partial results");
    std::vector<LogdetOut> out((size_t)nf);
    HS_HIP(hipStreamSynchronize(v.stream));  // the factors are written on the handle's stream
    HS_HIP(hipMemcpy(din.p, lf.data(), sizeof(LogdetFront) * (size_t)nf, hipMemcpyHostToDevice));
    launch_logdet<T>((const LogdetFront*)din.p, nf, (LogdetOut*)dout.p, v.stream);
    HS_HIP(hipGetLastError());
    HS_HIP(hipStreamSynchronize(v.stream));
    HS_HIP(hipMemcpy(out.data(), dout.p, sizeof(LogdetOut) * (size_t)nf, hipMemcpyDeviceToHost));
    for (int i = 0; i < nf; ++i) acc.add(out[(size_t)i]);  // post-order, always the same
  }
  // hs_ulv_mode 1 (check_common let them through): a front whose D is an eliminated HSS matrix adds det D from its ULV factors, after the
  // fronts above and in post-order; the 2 x 2 block form of mf = 3 is det D = det(A11) det(S22)
  for (const HsSelFront& x : v.fronts) {
    if (!(x.flags & HS_SEL_NOLU) || x.ni <= 0) continue;
    for (const hs_hss* H : {x.hss, x.hss2}) {
      if (!H) continue;
      double l = 0.0, sr = 0.0, si = 0.0;
      HS_CHECK(hs_hss_logabsdet(H, &l, &sr, &si));
      acc.add(l, sr, si);
    }
  }
  acc.finish(sizeof(T) != sizeof(double), logabs, &sign2[0], &sign2[1]);
}

// ---- selected inversion ---------------------------------------------------------------------------------------------------------------
struct Launch {
  size_t off;
  int cnt, maxM, maxN, minus;
};
struct Fill {  // a block a low-rank front of rank 0 leaves unwritten: cleared before (Z[int, bnd]) or after (X2[bnd, :]) the products
  void* p;
  size_t pitch, width, height;
};

// Flops of the dense-form recurrence of one front, the products run_batch issues for a dense front (real flops, 256-blocks counted as
// they are launched); nothing is launched here
template <class T>
double dense_form_flops(int ni, int nb) {
  const double m = (double)ni + nb, n = (double)ni, b = (double)nb;
  double f = n * b * b + m * n * b;  // Vb = -Uib Zbb;  Tm -= Z[:, bnd] Lbi
  for (int kb = (ni + 255) / 256 - 1; kb >= 0; --kb) {
    const double k0 = (double)kb * 256, wk = std::min(256.0, n - k0);
    f += wk * b * wk + wk * (n - k0) * wk + k0 * b * wk + k0 * (n - k0) * wk;  // U^-1 [Vi | Vb]
    f += m * wk * wk + m * k0 * wk;                                            // Tm L^-1
  }
  return (sizeof(T) == 16 ? 8.0 : 2.0) * f;
}

// Selected inversion over the tree.  lrmode = false is hs_selinv: every front dense, the low-rank pointers of the view are never read.
// lrmode = true is hs_selinv_lr: a front with low-rank objects runs the rank-structured form below, every other front the dense one, in
// the same launches; on a handle without low-rank fronts the two modes issue the same launches.
//
// Low-rank front (Uib ~= G Z_R, Lbi ~= C_L Z_L'; W = U^-1 G, Y' = Z_L' L^-1):
//   T1 = -Z_R Zbb,  T2 = -Zbb C_L,  T3 = T1 C_L                         (products through r-wide blocks)
//   [Tm[int, :] | W] = U^-1 [Vi | Vg],  Vg a copy of G                   (the blocked back substitution, rR columns instead of nb)
//   [X2[int, :]; Y'] = [Tm[int, :]; Z_L' copy] L^-1                      (the right substitution on ni + rL rows, written as two row groups)
//   Z[int, bnd] = W T1,   X2[bnd, :] = T2 Y',   X2[int, :] -= (W T3) Y'
// No substitution and no product has an nb-wide or m-tall operand except T1, T2 and the writes into Z / X2.
template <class T>
struct SelRun {
  const HsSelView& v;
  SelCache* c;
  hipStream_t s;
  int trans;
  T* d_diag;
  T* d_zval;
  size_t budget;
  bool lrmode = false;
  std::vector<std::vector<int>> kids;
  size_t alive = 0, peak = 0;
  double flops = 0.0, flops_dense = 0.0;  // executed; what the dense form would execute on the same front shapes
  int batches = 0, lr_fronts = 0, max_rank = 0;
  HsScratch work, descs;  // work blocks and descriptors of the current batch (reused, grown on demand)

  struct Batch {
    std::vector<int> fronts;
    std::vector<size_t> zoff;  // element offset of every front's block
    HsScratch Z;
    int pending = 0;  // batches of children that still have to gather from Z
  };

  struct LrOf {  // the low-rank transforms of a front as this run sees them (on = false: dense recurrence)
    bool on = false;
    const LowRank<T>* R = nullptr;
    const LowRank<T>* L = nullptr;
    int rR = 0, rL = 0;
  };
  LrOf lr_of(const HsSelFront& x) const {
    LrOf o;
    if (!lrmode || (!x.lrL && !x.lrR) || x.nb <= 0 || x.ni <= 0) return o;
    o.on = true;
    o.R = (const LowRank<T>*)x.lrR;
    o.L = (const LowRank<T>*)x.lrL;
    o.rR = o.R ? o.R->r : 0;
    o.rL = o.L ? o.L->r : 0;
    return o;
  }
  struct Work {  // element counts of a front's work blocks, in the order they are laid out
    size_t r1 = 0, r2 = 0, wg = 0, yp = 0, t1 = 0, t2 = 0, t3 = 0, wt3 = 0;
    size_t total() const { return r1 + r2 + wg + yp + t1 + t2 + t3 + wt3; }
  };
  static size_t blk(int ld, int cols) { return cols > 0 ? rup32((size_t)ld * (size_t)cols + 32) : 0; }
  Work work_of(const HsSelFront& x) const {
    Work w;
    w.r1 = r1elems(x);
    const LrOf o = lr_of(x);
    if (!o.on) {
      w.r2 = r2elems(x);
      return w;
    }
    w.r1 = std::max(w.r1, rup32((size_t)rup2(x.ni) * (size_t)(x.ni + o.rR) + 32));  // [Vi | Vg] (a matrix-free front's rank is not bounded by nb)
    w.r2 = rup32((size_t)(rup2(x.ni) + rup2(o.rL)) * (size_t)x.ni + 32);
    w.wg = blk(rup2(x.ni), o.rR);
    w.yp = o.rL > 0 ? blk(rup2(o.rL), x.ni) : 0;
    w.t1 = o.rR > 0 ? blk(rup2(o.rR), x.nb) : 0;
    w.t2 = blk(rup2(x.nb), o.rL);
    w.t3 = o.rR > 0 ? blk(rup2(o.rR), o.rL) : 0;
    w.wt3 = o.rR > 0 ? blk(rup2(x.ni), o.rL) : 0;
    return w;
  }

  static size_t zelems(const HsSelFront& x) {
    const int m = x.ni + x.nb;
    return rup32((size_t)rup2(m) * (size_t)m + 32);
  }
  static size_t r1elems(const HsSelFront& x) {
    const int m = x.ni + x.nb;
    return rup32(std::max((size_t)rup2(m) * (size_t)x.ni, (size_t)rup2(x.ni) * (size_t)m) + 32);
  }
  static size_t r2elems(const HsSelFront& x) { return rup32((size_t)rup2(x.ni + x.nb) * (size_t)x.ni + 32); }
  size_t cost(const HsSelFront& x) const { return (zelems(x) + work_of(x).total()) * sizeof(T); }

  void note_alive(long long delta) {
    alive = (size_t)((long long)alive + delta);
    peak = std::max(peak, alive);
  }

  void add(std::vector<GemmProb<T>>& P, const T* A, int lda, const T* B, int ldb, T* C, int ldc, int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return;
    GemmProb<T> p;
    p.A = A; p.B = B; p.C = C;
    p.M = M; p.N = N; p.K = K;
    p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    P.push_back(p);
    flops += (sizeof(T) == 16 ? 8.0 : 2.0) * (double)M * (double)N * (double)K;
  }

  // the fronts of one level (all of them children of `parent`'s fronts, or the roots): cut into batches by the budget, every batch followed
  // by the batches of its own children
  void run_level(const std::vector<int>& fronts, Batch* parent, const std::vector<size_t>* pzoff_of_front) {
    std::vector<std::vector<int>> cuts;
    {
      const size_t room = budget > alive ? budget - alive : 0;
      size_t used = 0, pairs = 0;  // pairs: a front brings two GEMM problems to a launch, a low-rank front up to four; grid.y <= 65535
      for (int f : fronts) {
        const size_t cst = cost(v.fronts[f]), pr = lr_of(v.fronts[f]).on ? 2 : 1;
        if (cuts.empty() || (used + cst > room && !cuts.back().empty()) || pairs + pr > 16384) {
          cuts.emplace_back();
          used = pairs = 0;
        }
        cuts.back().push_back(f);
        used += cst;
        pairs += pr;
      }
    }
    if (parent) parent->pending = (int)cuts.size();
    for (auto& cut : cuts) {
      Batch b;
      b.fronts = cut;
      run_batch(b, parent, pzoff_of_front);
      if (parent && --parent->pending == 0) {  // (run_batch ended with a synchronisation: the gathers are done)
        note_alive(-(long long)parent->Z.bytes);
        parent->Z.give();
      }
      std::vector<int> ch;
      for (int f : b.fronts)
        for (int k : kids[(size_t)f]) ch.push_back(k);
      if (ch.empty()) {
        note_alive(-(long long)b.Z.bytes);
        b.Z.give();
      } else {
        std::vector<size_t> zof(v.fronts.size(), 0);
        for (size_t i = 0; i < b.fronts.size(); ++i) zof[(size_t)b.fronts[i]] = b.zoff[i];
        run_level(ch, &b, &zof);
      }
    }
  }

  void run_batch(Batch& b, Batch* parent, const std::vector<size_t>* pzoff) {
    const int nbt = (int)b.fronts.size();
    ++batches;
    size_t ztot = 0, wtot = 0;
    b.zoff.resize((size_t)nbt);
    std::vector<size_t> woff((size_t)nbt);
    for (int i = 0; i < nbt; ++i) {
      const HsSelFront& x = v.fronts[b.fronts[(size_t)i]];
      b.zoff[(size_t)i] = ztot;
      ztot += zelems(x);
      woff[(size_t)i] = wtot;
      wtot += work_of(x).total();
    }
    b.Z.take(ztot * sizeof(T), "blocks of the selected inverse");
    note_alive((long long)b.Z.bytes);
    T* W;
    if (v.sb && wtot * sizeof(T) <= v.sb_bytes) {
      W = (T*)v.sb;  // the Schur scratch of the factorization, idle now
    } else {
      if (work.bytes < wtot * sizeof(T)) {
        note_alive(-(long long)work.bytes);
        work.take(wtot * sizeof(T), "work blocks of the selected inversion");
        note_alive((long long)work.bytes);
      }
      W = (T*)work.p;
    }
    peak = std::max(peak, alive + (W == (T*)v.sb ? wtot * sizeof(T) : 0));

    std::vector<SelDesc<T>> D((size_t)nbt);
    std::vector<GemmProb<T>> P;
    std::vector<Launch> L;
    std::vector<Fill> fill_before, fill_after;
    std::vector<LrOf> lro((size_t)nbt);
    int maxni = 0, maxnb = 0, maxm = 0, maxe = 0, maxblk = 0, maxr = 0;
    for (int i = 0; i < nbt; ++i) {
      const int f = b.fronts[(size_t)i];
      const HsSelFront& x = v.fronts[f];
      SelDesc<T>& d = D[(size_t)i];
      memset(&d, 0, sizeof d);
      d.ni = x.ni; d.nb = x.nb; d.m = x.ni + x.nb;
      d.ldz = rup2(d.m);
      d.ldv = rup2(d.ni);
      d.Z = (T*)b.Z.p + b.zoff[(size_t)i];
      if (parent && x.parent >= 0 && x.nb > 0) {
        const HsSelFront& px = v.fronts[x.parent];
        d.Zp = (const T*)parent->Z.p + (*pzoff)[(size_t)x.parent];
        d.ldzp = rup2(px.ni + px.nb);
        d.cmap = c->d_cmap + c->cmoff[(size_t)f];
      }
      d.rperm = x.rperm;
      d.fidx = x.fidx;
      d.Vi = W + woff[(size_t)i];
      d.X2 = d.Vi;                            // (Vi and Vb are dead when X2 is written)
      const Work w = work_of(x);
      d.Tm = W + woff[(size_t)i] + w.r1;
      const LrOf o = lro[(size_t)i] = lr_of(x);
      if (o.on) {
        d.rR = o.rR; d.rL = o.rL;
        d.nit = rup2(d.ni);
        d.ldt = d.nit + rup2(o.rL);
        d.ld1 = rup2(o.rR); d.ld2 = rup2(d.nb); d.ldy = rup2(o.rL);
        if (o.rR > 0) { d.G = o.R->Cd; d.ldg = o.R->ldc; d.ZR = o.R->Z; d.ldzr = o.R->ldz; }
        if (o.rL > 0) { d.CL = o.L->Cd; d.ldcl = o.L->ldc; d.ZL = o.L->Z; d.ldzl = o.L->ldz; }
        d.Wg = d.Tm + w.r2;
        d.Yp = d.Wg + w.wg;
        d.T1 = d.Yp + w.yp;
        d.T2 = d.T1 + w.t1;
        d.T3 = d.T2 + w.t2;
        d.WT3 = d.T3 + w.t3;
        if (o.rR == 0) fill_before.push_back(Fill{d.Z + (size_t)d.ni * d.ldz, (size_t)d.ldz * sizeof(T), (size_t)d.ni * sizeof(T), (size_t)d.nb});  // Z[int, bnd] = 0
        if (o.rL == 0) fill_after.push_back(Fill{d.X2 + d.ni, (size_t)d.ldz * sizeof(T), (size_t)d.nb * sizeof(T), (size_t)d.ni});                  // Z[bnd, int] = 0
        ++lr_fronts;
        max_rank = std::max(max_rank, std::max(o.rR, o.rL));
        maxr = std::max(maxr, std::max(o.rR, o.rL));
      }
      flops_dense += dense_form_flops<T>(x.ni, x.nb);
      d.epr = c->d_epr + c->eptr[(size_t)f];
      d.epc = c->d_epc + c->eptr[(size_t)f];
      d.ee = c->d_ee + c->eptr[(size_t)f];
      d.ecnt = (int)(c->eptr[(size_t)f + 1] - c->eptr[(size_t)f]);
      maxni = std::max(maxni, d.ni); maxnb = std::max(maxnb, d.nb); maxm = std::max(maxm, d.m); maxe = std::max(maxe, d.ecnt);
      maxblk = std::max(maxblk, (d.ni + 255) / 256);
    }
    auto close = [&](size_t from, int minus) {
      if (P.size() == from) return;
      Launch l{from, (int)(P.size() - from), 0, 0, minus};
      for (size_t k = from; k < P.size(); ++k) {
        l.maxM = std::max(l.maxM, P[k].M);
        l.maxN = std::max(l.maxN, P[k].N);
      }
      L.push_back(l);
    };
    auto each = [&](auto&& body) {  // the dense fronts of the batch
      for (int i = 0; i < nbt; ++i) {
        if (lro[(size_t)i].on) continue;
        const HsSelFront& x = v.fronts[b.fronts[(size_t)i]];
        body(D[(size_t)i], x, (const T*)x.LU, (const T*)x.UR, D[(size_t)i].Vi + (size_t)D[(size_t)i].ldv * D[(size_t)i].ni);
      }
    };
    auto each_lr = [&](auto&& body) {  // its low-rank fronts; Vg sits where a dense front keeps Vb
      for (int i = 0; i < nbt; ++i) {
        if (!lro[(size_t)i].on) continue;
        const HsSelFront& x = v.fronts[b.fronts[(size_t)i]];
        body(D[(size_t)i], x, (const T*)x.LU, D[(size_t)i].Vi + (size_t)D[(size_t)i].ldv * D[(size_t)i].ni);
      }
    };
    size_t from = P.size();
    // Vb = -Uib Zbb
    each([&](SelDesc<T>& d, const HsSelFront& x, const T*, const T* UR, T* Vb) {
      add(P, UR, x.ldu, d.Z + d.ni + (size_t)d.ni * d.ldz, d.ldz, Vb, d.ldv, d.ni, d.nb, d.nb);
    });
    // T1 = -Z_R Zbb, T2 = -Zbb C_L
    each_lr([&](SelDesc<T>& d, const HsSelFront&, const T*, T*) {
      const T* Zbb = d.Z + d.ni + (size_t)d.ni * d.ldz;
      add(P, d.ZR, d.ldzr, Zbb, d.ldz, d.T1, d.ld1, d.rR, d.nb, d.nb);
      add(P, Zbb, d.ldz, d.CL, d.ldcl, d.T2, d.ld2, d.nb, d.rL, d.nb);
    });
    close(from, 1);
    // [Tm[int, :] | Z[int, bnd]] = U^-1 [Vi | Vb], the last 256-block of every front first; a low-rank front: [Tm[int, :] | W] = U^-1 [Vi | Vg]
    for (int st = 0; st < maxblk; ++st) {
      from = P.size();
      each([&](SelDesc<T>& d, const HsSelFront& x, const T*, const T*, T* Vb) {
        const int kb = (d.ni + 255) / 256 - 1 - st;
        if (kb < 0) return;
        const int k0 = kb * 256, wk = std::min(256, d.ni - k0);
        const T* iU = (const T*)x.inv256U + (size_t)kb * 65536;
        add(P, iU, 256, Vb + k0, d.ldv, d.Z + k0 + (size_t)d.ni * d.ldz, d.ldz, wk, d.nb, wk);
        add(P, iU, 256, d.Vi + k0 + (size_t)k0 * d.ldv, d.ldv, d.Tm + k0 + (size_t)k0 * d.ldz, d.ldz, wk, d.ni - k0, wk);
      });
      each_lr([&](SelDesc<T>& d, const HsSelFront& x, const T*, T* Vg) {
        if (st == 0) add(P, d.T1, d.ld1, d.CL, d.ldcl, d.T3, d.ld1, d.rR, d.rL, d.nb);  // T3 = T1 C_L rides in the first launch after T1
        const int kb = (d.ni + 255) / 256 - 1 - st;
        if (kb < 0) return;
        const int k0 = kb * 256, wk = std::min(256, d.ni - k0);
        const T* iU = (const T*)x.inv256U + (size_t)kb * 65536;
        add(P, iU, 256, Vg + k0, d.ldv, d.Wg + k0, d.ldv, wk, d.rR, wk);
        add(P, iU, 256, d.Vi + k0 + (size_t)k0 * d.ldv, d.ldv, d.Tm + k0 + (size_t)k0 * d.ldt, d.ldt, wk, d.ni - k0, wk);
      });
      close(from, 0);
      from = P.size();
      each([&](SelDesc<T>& d, const HsSelFront& x, const T* LU, const T*, T* Vb) {
        const int kb = (d.ni + 255) / 256 - 1 - st;
        if (kb <= 0) return;
        const int k0 = kb * 256, wk = std::min(256, d.ni - k0);
        const T* U01 = LU + (size_t)k0 * x.ldlu;  // rows 0:k0 of the block column
        add(P, U01, x.ldlu, d.Z + k0 + (size_t)d.ni * d.ldz, d.ldz, Vb, d.ldv, k0, d.nb, wk);
        add(P, U01, x.ldlu, d.Tm + k0 + (size_t)k0 * d.ldz, d.ldz, d.Vi + (size_t)k0 * d.ldv, d.ldv, k0, d.ni - k0, wk);
      });
      each_lr([&](SelDesc<T>& d, const HsSelFront& x, const T* LU, T* Vg) {
        const int kb = (d.ni + 255) / 256 - 1 - st;
        if (kb <= 0) return;
        const int k0 = kb * 256, wk = std::min(256, d.ni - k0);
        const T* U01 = LU + (size_t)k0 * x.ldlu;
        add(P, U01, x.ldlu, d.Wg + k0, d.ldv, Vg, d.ldv, k0, d.rR, wk);
        add(P, U01, x.ldlu, d.Tm + k0 + (size_t)k0 * d.ldt, d.ldt, d.Vi + (size_t)k0 * d.ldv, d.ldv, k0, d.ni - k0, wk);
      });
      close(from, 1);
    }
    // Tm -= Z[:, bnd] Lbi
    from = P.size();
    each([&](SelDesc<T>& d, const HsSelFront& x, const T* LU, const T*, T*) {
      add(P, d.Z + (size_t)d.ni * d.ldz, d.ldz, LU + d.ni, x.ldlu, d.Tm, d.ldz, d.m, d.ni, d.nb);
    });
    close(from, 1);
    // X2 = Tm L^-1; a low-rank front: [X2[int, :]; Y'] = [Tm[int, :]; Z_L' copy] L^-1, its two row groups as two problems
    for (int st = 0; st < maxblk; ++st) {
      from = P.size();
      each([&](SelDesc<T>& d, const HsSelFront& x, const T*, const T*, T*) {
        const int kb = (d.ni + 255) / 256 - 1 - st;
        if (kb < 0) return;
        const int k0 = kb * 256, wk = std::min(256, d.ni - k0);
        add(P, d.Tm + (size_t)k0 * d.ldz, d.ldz, (const T*)x.inv256L + (size_t)kb * 65536, 256, d.X2 + (size_t)k0 * d.ldz, d.ldz, d.m, wk, wk);
      });
      each_lr([&](SelDesc<T>& d, const HsSelFront& x, const T*, T*) {
        if (st == 0) {  // W is complete: Z[int, bnd] = W T1, WT3 = W T3
          add(P, d.Wg, d.ldv, d.T1, d.ld1, d.Z + (size_t)d.ni * d.ldz, d.ldz, d.ni, d.nb, d.rR);
          add(P, d.Wg, d.ldv, d.T3, d.ld1, d.WT3, d.ldv, d.ni, d.rL, d.rR);
        }
        const int kb = (d.ni + 255) / 256 - 1 - st;
        if (kb < 0) return;
        const int k0 = kb * 256, wk = std::min(256, d.ni - k0);
        const T* iL = (const T*)x.inv256L + (size_t)kb * 65536;
        add(P, d.Tm + (size_t)k0 * d.ldt, d.ldt, iL, 256, d.X2 + (size_t)k0 * d.ldz, d.ldz, d.ni, wk, wk);
        add(P, d.Tm + d.nit + (size_t)k0 * d.ldt, d.ldt, iL, 256, d.Yp + (size_t)k0 * d.ldy, d.ldy, d.rL, wk, wk);
      });
      close(from, 0);
      from = P.size();
      each([&](SelDesc<T>& d, const HsSelFront& x, const T* LU, const T*, T*) {
        const int kb = (d.ni + 255) / 256 - 1 - st;
        if (kb <= 0) return;
        const int k0 = kb * 256, wk = std::min(256, d.ni - k0);
        add(P, d.X2 + (size_t)k0 * d.ldz, d.ldz, LU + k0, x.ldlu, d.Tm, d.ldz, d.m, k0, wk);
      });
      each_lr([&](SelDesc<T>& d, const HsSelFront& x, const T* LU, T*) {
        const int kb = (d.ni + 255) / 256 - 1 - st;
        if (kb <= 0) return;
        const int k0 = kb * 256, wk = std::min(256, d.ni - k0);
        add(P, d.X2 + (size_t)k0 * d.ldz, d.ldz, LU + k0, x.ldlu, d.Tm, d.ldt, d.ni, k0, wk);
        add(P, d.Yp + (size_t)k0 * d.ldy, d.ldy, LU + k0, x.ldlu, d.Tm + d.nit, d.ldt, d.rL, k0, wk);
      });
      close(from, 1);
    }
    // X2[bnd, :] = T2 Y', then X2[int, :] -= (W T3) Y'
    from = P.size();
    each_lr([&](SelDesc<T>& d, const HsSelFront&, const T*, T*) { add(P, d.T2, d.ld2, d.Yp, d.ldy, d.X2 + d.ni, d.ldz, d.nb, d.ni, d.rL); });
    close(from, 0);
    from = P.size();
    each_lr([&](SelDesc<T>& d, const HsSelFront&, const T*, T*) {
      if (d.rR > 0) add(P, d.WT3, d.ldv, d.Yp, d.ldy, d.X2, d.ldz, d.ni, d.ni, d.rL);  // (rR = 0: there is no WT3 block)
    });
    close(from, 1);

    const size_t dbytes = sizeof(SelDesc<T>) * (size_t)nbt, pbytes = sizeof(GemmProb<T>) * std::max<size_t>(P.size(), 1);
    if (descs.bytes < dbytes + pbytes + 256) descs.take(2 * (dbytes + pbytes) + 256, "descriptors of the selected inversion");
    SelDesc<T>* dD = (SelDesc<T>*)descs.p;
    GemmProb<T>* dP = (GemmProb<T>*)((char*)descs.p + (dbytes + 255) / 256 * 256);
    HS_HIP(hipMemcpy(dD, D.data(), dbytes, hipMemcpyHostToDevice));  // (the stream is idle: every batch ends with a synchronisation)
    if (!P.empty()) HS_HIP(hipMemcpy(dP, P.data(), sizeof(GemmProb<T>) * P.size(), hipMemcpyHostToDevice));
    HS_HIP(hipMemsetAsync(W, 0, wtot * sizeof(T), s));
    launch_zinit<T>(dD, nbt, maxni, s);
    launch_zload_lr<T>(dD, nbt, maxni, maxr, s);  // (maxr = 0 without low-rank fronts: no launch)
    for (const Fill& f : fill_before) HS_HIP(hipMemset2DAsync(f.p, f.pitch, 0, f.width, f.height, s));
    if (parent) launch_zgather<T>(dD, nbt, maxnb, s);
    for (const Launch& l : L) launch_gemm_probs<T>(dP + l.off, l.cnt, l.maxM, l.maxN, l.minus, s);
    for (const Fill& f : fill_after) HS_HIP(hipMemset2DAsync(f.p, f.pitch, 0, f.width, f.height, s));
    launch_zpermute_cols<T>(dD, nbt, maxm, maxni, s);
    launch_zextract<T>(dD, nbt, maxni, maxe, trans, d_diag, d_zval, s);
    HS_HIP(hipGetLastError());
    HS_HIP(hipStreamSynchronize(s));
  }
};

template <class T>
void selinv_impl(const HsSelView& v, SelCache* c, bool lrmode, int trans, void* diag, void* zval, int where, int64_t budget_bytes, hipStream_t s) {
  const int nf = (int)v.fronts.size();
  HS_HIP(hipStreamSynchronize(v.stream));  // the factors are written on the handle's stream
  HsScratch odiag, ozval;
  T *d_diag = nullptr, *d_zval = nullptr;
  if (diag) {
    if (where) d_diag = (T*)diag;
    else {
      odiag.take(sizeof(T) * (size_t)std::max<int64_t>(v.n, 1), "diagonal of the inverse");
      d_diag = (T*)odiag.p;
    }
  }
  if (zval) {
    if (where) d_zval = (T*)zval;
    else {
      ozval.take(sizeof(T) * (size_t)std::max<int64_t>(v.nnz, 1), "pattern values of the inverse");
      d_zval = (T*)ozval.p;
    }
  }
  size_t budget = (size_t)std::max<int64_t>(budget_bytes, 0);
  if (budget == 0) {  // what the device can give right now, with a margin for the allocator
    size_t fr = 0, tot = 0;
    HS_HIP(hipMemGetInfo(&fr, &tot));
    budget = (size_t)((double)fr * 0.85) + (v.sb ? v.sb_bytes : 0);
  }
  SelRun<T> R{v, c, s, trans, d_diag, d_zval, budget, lrmode};
  R.kids.assign((size_t)nf, {});
  std::vector<int> roots;
  for (int f = 0; f < nf; ++f) {
    if (v.fronts[f].parent >= 0) R.kids[(size_t)v.fronts[f].parent].push_back(f);
    else roots.push_back(f);
  }
  HsEvents<2> ev;
  HsDrain drain{s};  // nothing may still be reading the blocks the unwinding gives back
  float ms = 0.f;
  HS_HIP(hipEventRecord(ev[0], s));
  R.run_level(roots, nullptr, nullptr);
  HS_HIP(hipEventRecord(ev[1], s));
  HS_HIP(hipEventSynchronize(ev[1]));
  HS_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  if (diag && !where) HS_HIP(hipMemcpy(diag, d_diag, sizeof(T) * (size_t)v.n, hipMemcpyDeviceToHost));
  if (zval && !where && v.nnz) HS_HIP(hipMemcpy(zval, d_zval, sizeof(T) * (size_t)v.nnz, hipMemcpyDeviceToHost));
  if (lrmode) {
    const double out[8] = {ms * 1e-3, R.flops, (double)R.peak, (double)R.batches, (double)R.lr_fronts, (double)R.max_rank, R.flops_dense, 0.0};
    std::copy(out, out + 8, c->info_lr);
    return;
  }
  c->info[0] = ms * 1e-3;
  c->info[1] = R.flops;
  c->info[2] = (double)R.peak;
  c->info[3] = (double)R.batches;
}

}  // namespace

extern "C" int hs_logabsdet(hs_handle* F, double* logabs, double* sign2) {
  HS_GUARD(HsSelView v; check_common(F, v, "hs_logabsdet", true);
           if (!logabs || !sign2) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_logabsdet: logabs and sign2 must not be NULL");
           if (v.is_complex) logabsdet_impl<cplx>(v, logabs, sign2); else logabsdet_impl<double>(v, logabs, sign2);
           // hs_options.equilibrate: det A_s = 2^(sum er + sum ec) det A, the exponent sum exact in int64
           if (hs_handle_equilibrated(F)) *logabs -= 0.6931471805599453094 * (double)hs_handle_equil_sum(F));
}

// hs_selinv (lrmode = false) and hs_selinv_lr (true): the same arguments, the same checks before any device work; they differ in what
// they do with a front that keeps low-rank Gauss transforms
static void selinv_entry(const char* fn, bool lrmode, hs_handle* F, int trans, void* diag, void* zval, int where, int64_t budget_bytes, void* stream) {
  HsSelView v;
  check_common(F, v, fn);
  hs_refuse_equilibrated(F, fn);
  if (trans != 0 && trans != 1) HS_FAIL(HS_ERR_ARGUMENT, trans, "ArgumentError: %s: trans = %d must be 0 (entries of A^-1) or 1 (of its transpose)", fn, trans);
  if (where != 0 && where != 1) HS_FAIL(HS_ERR_ARGUMENT, where, "ArgumentError: %s: where = %d must be 0 (host pointers) or 1 (device pointers)", fn, where);
  if (!diag && !zval) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: diag and zval are both NULL, nothing to compute", fn);
  if (budget_bytes < 0) HS_FAIL(HS_ERR_ARGUMENT, budget_bytes, "ArgumentError: %s: budget_bytes < 0", fn);
  for (size_t i = 0; i < v.fronts.size(); ++i) {
    const HsSelFront& x = v.fronts[i];
    const int fl = x.flags;
    if ((fl & HS_SEL_LOWRANK) && !lrmode)
      HS_FAIL(HS_ERR_UNSUPPORTED, (long long)i, "%s: front %d keeps low-rank Gauss transforms L / R (compressed factorization); selected inversion needs the exact path (swlevel = 0)", fn, (int)i);
    if (fl & HS_SEL_SLICE)
      HS_FAIL(HS_ERR_UNSUPPORTED, (long long)i, "%s: front %d is eliminated in slices (hs_options.split)", fn, (int)i);
    if (!(fl & HS_SEL_LOWRANK) || x.nb <= 0 || x.ni <= 0) continue;  // (without a boundary there are no transforms: the LU alone serves)
    if (!x.lrL && !x.lrR)
      HS_FAIL(HS_ERR_UNSUPPORTED, (long long)i, "%s: front %d is flagged for compression but holds no low-rank objects, and its dense panels Lbi / Uib do not survive the factorization", fn, (int)i);
    // (LowRank<double> and LowRank<cplx> share their layout: pointers and ints)
    for (const LowRank<double>* lr : {(const LowRank<double>*)x.lrL, (const LowRank<double>*)x.lrR}) {
      if (!lr || lr->r <= 0) continue;
      if (!lr->Cd || !lr->Z)
        HS_FAIL(HS_ERR_UNSUPPORTED, (long long)i, "%s: front %d holds a low-rank transform of rank %d without its dense factor (only the packed sketch is kept, HS_LR_QR=0 diagnostics)", fn, (int)i, lr->r);
    }
  }
  SelCache* c = cache_of(v);
  if (!c->built) build_cache(v, c);  // (host work and uploads of index lists only)
  if (c->hole >= 0)
    HS_FAIL(HS_ERR_UNSUPPORTED, c->hole, "%s: stored entry %lld of A (CSC order) lies outside every front's [int; bnd] block: the tree does not cover A's pattern, the pattern values of the inverse would have a hole", fn, c->hole);
  if (c->hole_front >= 0)
    HS_FAIL(HS_ERR_UNSUPPORTED, c->hole_front, "%s: the boundary of front %d is not contained in its parent's front (a root that keeps a boundary without a pseudo-root, or an inconsistent tree)", fn, c->hole_front);
  hipStream_t s = stream ? (hipStream_t)stream : v.stream;
  if (v.is_complex) selinv_impl<cplx>(v, c, lrmode, trans, diag, zval, where, budget_bytes, s);
  else selinv_impl<double>(v, c, lrmode, trans, diag, zval, where, budget_bytes, s);
}

extern "C" int hs_selinv(hs_handle* F, int trans, void* diag, void* zval, int where, int64_t budget_bytes, void* stream) {
  HS_GUARD(selinv_entry("hs_selinv", false, F, trans, diag, zval, where, budget_bytes, stream));
}

extern "C" int hs_selinv_lr(hs_handle* F, int trans, void* diag, void* zval, int where, int64_t budget_bytes, void* stream) {
  HS_GUARD(selinv_entry("hs_selinv_lr", true, F, trans, diag, zval, where, budget_bytes, stream));
}

extern "C" int hs_selinv_lr_info(const hs_handle* F, double* out8) {
  HS_GUARD(if (!F || !out8) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_selinv_lr_info: null argument");
           HsSelView v; hs_selinv_view(const_cast<hs_handle*>(F), &v);
           const SelCache* c = (const SelCache*)*v.sx;
           for (int k = 0; k < 8; ++k) out8[k] = c ? c->info_lr[k] : 0.0);
}

extern "C" int hs_selinv_info(const hs_handle* F, double* out4) {
  HS_GUARD(if (!F || !out4) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_selinv_info: null argument");
           HsSelView v; hs_selinv_view(const_cast<hs_handle*>(F), &v);
           const SelCache* c = (const SelCache*)*v.sx;
           for (int k = 0; k < 4; ++k) out4[k] = c ? c->info[k] : 0.0);
}
