// hs_f32.hip -- hs_f32_*: a stand-alone copy of a factorization with the stored factors in Float32 (ComplexF32 for ComplexF64 handles),
// its block solve for F, transpose(F) and adjoint(F), and the in-place rounding hook of the tests (include/hs_solver.h, hs_f32.h).
//
// The copy holds what hs_solve_multi_run dereferences and nothing else.  Per front: LF (mrows x ni), UR (ni x nb, where the Gauss transforms
// are dense), the 256 x 256 inverse diagonal blocks of L and U (of the last block its wl x wl corner: the rest is never read and never
// written), rperm and fidx; per low-rank transform: Lp[:, :r] with its row permutation or the dense C, and Z; per level a SolveNode<S>
// array, S = float / cplxf, with the host metadata of an HsMultiView around it.  One plan (f32_plan) lists these blocks from the handle's
// view; hs_f32_create gives every one a destination and demotes it (kernels_f32.hip, one grouped launch per level), hsk_round_factors_f32
// runs the same list with the source as its own destination.  Values and indices of a level live in one block of the library's scratch
// cache each; the object keeps no pointer into the handle.
//
// The solve is hs_solve_multi_run_f32 (hs_solve_multi.hip): the schedule of the FP64 block solve over kernels_solve_multi_f32.hip, work
// blocks, right-hand sides and results in Float64 / ComplexF64.  The work-block cache is the object's own.
#include <chrono>
#include <cstring>
#include <deque>
#include <vector>

#include "hs_f32.h"
#include "../../include/hs_solver.h"
#include "hs_host.h"

struct hs_f32 {
  int64_t n = 0;
  int cx = 0;
  HsMultiView v;  // sn, lrL, lrR: the object's own SolveNode<S> arrays (device) and LowRank<S> structs (host, below)
  void* mx = nullptr;
  void (*mx_free)(void*) = nullptr;
  std::vector<std::pair<void*, size_t>> blocks;  // scratch blocks: values and indices, one of each per level
  std::vector<void*> desc;                       // hipMalloc: the SolveNode<S> arrays
  std::deque<LowRank<float>> lrd;
  std::deque<LowRank<cplxf>> lrz;
  double value_bytes = 0.0, other_bytes = 0.0, flushed = 0.0, t_demote = 0.0;
  ~hs_f32() {
    if (mx && mx_free) mx_free(mx);  // waits for the last solve
    for (auto& b : blocks) hs_scratch_give(b.first, b.second);
    for (void* p : desc) (void)hipFree(p);
  }
};

namespace {

template <class S>
std::deque<LowRank<S>>& lr_store(hs_f32* G);
template <>
std::deque<LowRank<float>>& lr_store<float>(hs_f32* G) { return G->lrd; }
template <>
std::deque<LowRank<cplxf>>& lr_store<cplxf>(hs_f32* G) { return G->lrz; }

// one block of T elements the block solve reads, and where its copy is announced: *slot receives the copy's address, *ldslot its ld
struct F32Item {
  const void* src;
  long long lds;  // in T elements
  int rows, cols;
  void** slot;    // null: the item continues the region of the one before it (the inverse diagonal blocks of a front) at `off`
  int* ldslot;
  size_t off;     // elements from the region's start
  long long ldd;  // ld of the copy; 0: hs_f32_ld(rows)
};
struct F32Index {
  const int* src;
  int count;
  const int** slot;
};
template <class T>
struct F32Plan {
  typedef typename F32Of<T>::type S;
  std::vector<std::vector<SolveNode<S>>> sn;  // per level, pointers cleared
  std::deque<LowRank<S>> lr;
  std::vector<std::vector<F32Item>> items;    // per level
  std::vector<std::vector<F32Index>> index;
  HsMultiView v;  // the handle's view with lrL / lrR redirected to `lr`
};

template <class T, class S>
void plan_lowrank(const void* src, const void** out, std::deque<LowRank<S>>& store, std::vector<F32Item>& items, std::vector<F32Index>& index) {
  if (!src) return;
  const LowRank<T>& a = *(const LowRank<T>*)src;
  store.emplace_back();
  LowRank<S>& b = store.back();
  b.rows = a.rows; b.cols = a.cols; b.k = a.k; b.r = a.r; b.top = a.top;
  *out = &b;
  if (a.r <= 0) return;
  items.push_back({a.Z, a.ldz, a.r, a.cols, (void**)&b.Z, &b.ldz, 0, 0});
  if (a.Cd) {
    items.push_back({a.Cd, a.ldc, a.rows, a.r, (void**)&b.Cd, &b.ldc, 0, 0});
  } else {
    items.push_back({a.Lp, a.ldp, a.rows, a.r, (void**)&b.Lp, &b.ldp, 0, 0});
    index.push_back({a.rperm, a.rows, (const int**)&b.rperm});
  }
}

// what hs_solve_multi_run reads of the handle, block by block (the descriptors come down from the device once)
template <class T>
void f32_plan(hs_handle* F, F32Plan<T>& P) {
  typedef typename F32Of<T>::type S;
  hs_multi_view(F, &P.v);
  const size_t nl = P.v.levels.size();
  P.sn.resize(nl);
  P.items.resize(nl);
  P.index.resize(nl);
  for (size_t lv = 0; lv < nl; ++lv) {
    HsMultiLevel& L = P.v.levels[lv];
    if (!L.hss.empty()) HS_FAIL(HS_ERR_UNSUPPORTED, 0, "hs_f32_*: fronts with an HSS interior block are not demoted");
    if (L.nfronts <= 0 || !L.sn) continue;
    std::vector<SolveNode<T>> h((size_t)L.nfronts);
    HS_HIP(hipMemcpy(h.data(), L.sn, h.size() * sizeof(SolveNode<T>), hipMemcpyDeviceToHost));
    std::vector<SolveNode<S>>& g = P.sn[lv];
    g.resize(h.size());
    for (size_t i = 0; i < h.size(); ++i) {
      const SolveNode<T>& a = h[i];
      SolveNode<S>& b = g[i];
      memset(&b, 0, sizeof b);
      b.ni = a.ni; b.nb = a.nb; b.m = a.m; b.mrows = a.mrows; b.compressed = a.compressed; b.woff = a.woff; b.poff = a.poff;
      if (a.ni <= 0) continue;
      if (!a.LF || !a.inv256L || !a.inv256U || !a.rperm || !a.fidx) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_f32_*: a front of the handle holds no factors");
      P.items[lv].push_back({a.LF, a.ldl, std::max(a.mrows, a.ni), a.ni, (void**)&b.LF, &b.ldl, 0, 0});
      if (!a.compressed && a.nb > 0 && a.UR) P.items[lv].push_back({a.UR, a.ldu, a.ni, a.nb, (void**)&b.UR, &b.ldu, 0, 0});
      for (int u = 0; u < 2; ++u) {
        const T* inv = u ? a.inv256U : a.inv256L;
        for (int j = 0; j * 256 < a.ni; ++j) {
          const int wl = std::min(256, a.ni - j * 256);
          P.items[lv].push_back({inv + (size_t)j * 65536, 256, wl, wl, j == 0 ? (void**)(u ? &b.inv256U : &b.inv256L) : nullptr, nullptr, (size_t)j * 65536, 256});
        }
      }
      P.index[lv].push_back({a.rperm, a.ni, &b.rperm});
      P.index[lv].push_back({a.fidx, a.ni + (int)L.fronts[i].nb, &b.fidx});
    }
    for (HsMultiLR& q : L.lr) {
      const void *l = q.lrL, *r = q.lrR;
      q.lrL = q.lrR = nullptr;
      plan_lowrank<T, S>(l, &q.lrL, P.lr, P.items[lv], P.index[lv]);
      plan_lowrank<T, S>(r, &q.lrR, P.lr, P.items[lv], P.index[lv]);
    }
  }
}

struct DevCounts {
  unsigned long long* d = nullptr;
  DevCounts() {
    HS_HIP(hipMalloc((void**)&d, 2 * sizeof(unsigned long long)));
    if (hipMemset(d, 0, 2 * sizeof(unsigned long long)) != hipSuccess) {
      (void)hipFree(d);
      HS_FAIL(HS_ERR_DEVICE, 0, "hs_f32_*: hipMemset failed");
    }
  }
  ~DevCounts() { (void)hipFree(d); }
  void read(hipStream_t s, unsigned long long* out2) {
    HS_HIP(hipMemcpyAsync(out2, d, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HS_HIP(hipStreamSynchronize(s));
  }
};

// one grouped demotion over jobs (host), uploaded into a scratch block that lives until the stream has run it
void run_jobs(const std::vector<F32Job>& jobs, bool inplace, unsigned long long* counts, hipStream_t s) {
  if (jobs.empty()) return;
  int maxrows = 0, maxcols = 0;
  for (const F32Job& j : jobs) {
    maxrows = std::max(maxrows, j.rows);
    maxcols = std::max(maxcols, j.cols);
  }
  HsDevBuf buf("demotion job list");
  F32Job* d = buf.get<F32Job>(jobs.size());
  HS_HIP(hipMemcpyAsync(d, jobs.data(), jobs.size() * sizeof(F32Job), hipMemcpyHostToDevice, s));
  launch_f32_demote(d, (int)jobs.size(), maxrows, maxcols, inplace, counts, s);
  HS_HIP(hipStreamSynchronize(s));
  HS_HIP(hipGetLastError());
}

size_t up256(size_t b) { return (b + 255) / 256 * 256; }

template <class T>
void create(hs_handle* F, hipStream_t s, hs_f32* G) {
  typedef typename F32Of<T>::type S;
  constexpr int RE = sizeof(T) / 8;  // real scalars per element
  const auto t0 = std::chrono::steady_clock::now();
  F32Plan<T> P;
  f32_plan<T>(F, P);
  DevCounts cnt;
  double elems = 0.0, held = 0.0;
  for (size_t lv = 0; lv < P.items.size(); ++lv) {
    std::vector<F32Item>& items = P.items[lv];
    std::vector<F32Index>& index = P.index[lv];
    // the level's value block: every region starts at a multiple of 256 bytes
    size_t vbytes = 0;
    std::vector<size_t> at(items.size());
    size_t region = 0;
    for (size_t i = 0; i < items.size(); ++i) {
      F32Item& it = items[i];
      if (it.ldd == 0) it.ldd = (RE == 2) ? std::max<long long>(it.rows, 1) : hs_f32_ld(it.rows);
      if (it.slot) {
        region = up256(vbytes);
        vbytes = region;
      }
      at[i] = region + it.off * sizeof(S);
      vbytes = std::max(vbytes, at[i] + (size_t)it.ldd * it.cols * sizeof(S));
      elems += (double)it.rows * it.cols;
    }
    if (vbytes) {
      char* base = (char*)hs_scratch_take(vbytes, "Float32 factor copy");
      G->blocks.push_back({base, vbytes});
      held += (double)vbytes;
      std::vector<F32Job> jobs(items.size());
      for (size_t i = 0; i < items.size(); ++i) {
        const F32Item& it = items[i];
        jobs[i] = {(const double*)it.src, base + at[i], it.lds * RE, it.ldd * RE, it.rows * RE, it.cols};
        if (it.slot) *it.slot = base + at[i];
        if (it.ldslot) *it.ldslot = (int)it.ldd;
      }
      run_jobs(jobs, false, cnt.d, s);
    }
    size_t icount = 0;
    for (const F32Index& ix : index) icount += (size_t)(ix.count + 63) / 64 * 64;
    if (icount) {
      int* ibase = (int*)hs_scratch_take(icount * sizeof(int), "Float32 factor copy (indices)");
      G->blocks.push_back({ibase, icount * sizeof(int)});
      held += (double)icount * sizeof(int);
      std::vector<F32IntJob> jobs(index.size());
      size_t o = 0;
      int maxcount = 0;
      for (size_t i = 0; i < index.size(); ++i) {
        jobs[i] = {index[i].src, ibase + o, index[i].count, 0};
        *index[i].slot = ibase + o;
        o += (size_t)(index[i].count + 63) / 64 * 64;
        maxcount = std::max(maxcount, index[i].count);
      }
      HsDevBuf buf("demotion job list");
      F32IntJob* d = buf.get<F32IntJob>(jobs.size());
      HS_HIP(hipMemcpyAsync(d, jobs.data(), jobs.size() * sizeof(F32IntJob), hipMemcpyHostToDevice, s));
      launch_f32_copy_int(d, (int)jobs.size(), maxcount, s);
      HS_HIP(hipStreamSynchronize(s));
      HS_HIP(hipGetLastError());
    }
  }
  unsigned long long c2[2] = {0, 0};
  cnt.read(s, c2);
  if (c2[0] > 0)
    HS_FAIL(HS_ERR_UNSUPPORTED, (long long)c2[0],
            "hs_f32_create: %llu stored factor entries are finite in Float64 and overflow Float32 (|x| > 3.4e38): scale the matrix before factoring it", c2[0]);
  // the descriptors, now that every slot is filled; the view takes the object's own arrays
  lr_store<S>(G) = std::move(P.lr);  // (a deque keeps its elements where they are when it is moved: the view's lrL / lrR stay valid)
  G->v = P.v;
  G->v.mx = &G->mx;
  G->v.mx_free = &G->mx_free;
  G->v.hss_front = nullptr;
  G->v.hss_ctx = nullptr;
  for (size_t lv = 0; lv < P.sn.size(); ++lv) {
    HsMultiLevel& L = G->v.levels[lv];
    L.sn = nullptr;
    if (P.sn[lv].empty()) continue;
    void* d = nullptr;
    const size_t b = P.sn[lv].size() * sizeof(SolveNode<S>);
    if (hipMalloc(&d, b) != hipSuccess) HS_FAIL(HS_ERR_NOMEM, 0, "OutOfMemoryError: hs_f32_create: hipMalloc of %zu bytes failed", b);
    G->desc.push_back(d);
    HS_HIP(hipMemcpy(d, P.sn[lv].data(), b, hipMemcpyHostToDevice));
    L.sn = d;
    held += (double)b;
  }
  G->value_bytes = elems * sizeof(S);
  G->other_bytes = held - G->value_bytes;
  G->flushed = (double)c2[1];
  G->t_demote = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

int probe_block_solve(hs_handle* F) {  // zero columns: the checks of hs_ldiv_block_dev_t_* and nothing else
  const int64_t n = F ? hs_size(F) : 0;
  if (F && hs_is_complex(F)) return hs_ldiv_block_dev_t_z(F, 0, nullptr, n, nullptr, n, n, 0, nullptr);
  return hs_ldiv_block_dev_t_d(F, 0, nullptr, n, nullptr, n, n, 0, nullptr);
}

void create_entry(hs_handle* F, void* stream, hs_f32** out) {
  if (!out) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_f32_create: G == NULL");
  *out = nullptr;
  HsHandleView hv = hs_view_of(F, "hs_f32_create");
  hs_refuse_equilibrated(F, "hs_f32_create");
  // The handles the block solve never serves are named first, so that a host-side plan (which the probe below would only call unfactored)
  // hears the lasting reason; every other refusal is the probe's own status and message.
  if (hv.nranks > 1)
    HS_FAIL(HS_ERR_UNSUPPORTED, 0, "hs_f32_create: block solves of a factorization over %d ranks are not implemented (single-rank factorizations only)", hv.nranks);
  if (hv.t_refused_node >= 0)
    HS_FAIL(HS_ERR_UNSUPPORTED, hv.t_refused_node,
            "hs_f32_create: node %d keeps its interior block D as an HSS matrix (hs_options.hss_d / mf = 2, 3): block solves are not implemented, and HSS blocks are not demoted",
            hv.t_refused_node);
  HS_CHECK(probe_block_solve(F));
  if (!hv.device) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_f32_create: handle holds a host-side plan only (hs_plan); use hs_analyze");
  if (!hv.factored) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_f32_create: handle holds no numeric factorization");
  hs_f32* G = new hs_f32();
  G->n = hv.n;
  G->cx = hv.is_complex ? 1 : 0;
  try {
    HS_HIP(hipStreamSynchronize(hv.stream));  // the factors are complete
    if (G->cx)
      create<cplx>(F, (hipStream_t)stream, G);
    else
      create<double>(F, (hipStream_t)stream, G);
  } catch (...) {
    (void)hipStreamSynchronize((hipStream_t)stream);
    delete G;
    throw;
  }
  *out = G;
}

template <class T>
void check_ldiv(const char* fn, hs_f32* G, int trans, int64_t ldc, int64_t ldb, int64_t n, int64_t nrhs) {
  if (!G) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null hs_f32", fn);
  hs_check_trans(fn, trans);
  if ((G->cx != 0) != (sizeof(T) == 16)) HS_FAIL(HS_ERR_ARGUMENT, 0, "MethodError: %s: eltype of G and B differ", fn);
  if (n != G->n || nrhs < 0 || ldc < n || ldb < n)
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: B has %lld rows (ldc %lld, ldb %lld, nrhs %lld), F is %lld x %lld", fn, (long long)n, (long long)ldc, (long long)ldb,
            (long long)nrhs, (long long)G->n, (long long)G->n);
}
template <class T>
void ldiv_dev(hs_f32* G, int trans, T* dC, int64_t ldc, const T* dB, int64_t ldb, int64_t n, int64_t nrhs, void* stream) {
  const char* fn = "hs_f32_ldiv_dev_*";
  check_ldiv<T>(fn, G, trans, ldc, ldb, n, nrhs);
  if (nrhs == 0) return;
  if (!dC || !dB) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null block", fn);
  hipStream_t s = (hipStream_t)stream;
  if (dC != dB) HS_HIP(hipMemcpy2DAsync(dC, ldc * sizeof(T), dB, ldb * sizeof(T), n * sizeof(T), nrhs, hipMemcpyDeviceToDevice, s));
  hs_solve_multi_run_f32<T>(G->v, trans, dC, ldc, nrhs, s);
}
template <class T>
void ldiv_host(hs_f32* G, int trans, T* C, int64_t ldc, const T* B, int64_t ldb, int64_t n, int64_t nrhs) {
  const char* fn = "hs_f32_ldiv_*";
  check_ldiv<T>(fn, G, trans, ldc, ldb, n, nrhs);
  if (nrhs == 0) return;
  if (!C || !B) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null block", fn);
  hs_stage_block<T>((hipStream_t) nullptr, "block solve right-hand sides", C, ldc, B, ldb, n, nrhs,
                    [&](T* d, int64_t ld, hipStream_t s) { hs_solve_multi_run_f32<T>(G->v, trans, d, ld, nrhs, s); });
}

template <class T>
void round_in_place(hs_handle* F, hipStream_t s, unsigned long long* c2) {
  constexpr int RE = sizeof(T) / 8;
  F32Plan<T> P;
  f32_plan<T>(F, P);
  DevCounts cnt;
  for (const std::vector<F32Item>& items : P.items) {
    std::vector<F32Job> jobs(items.size());
    for (size_t i = 0; i < items.size(); ++i) jobs[i] = {(const double*)items[i].src, (void*)items[i].src, items[i].lds * RE, items[i].lds * RE, items[i].rows * RE, items[i].cols};
    run_jobs(jobs, true, cnt.d, s);
  }
  cnt.read(s, c2);
}

}  // namespace

void hs_f32_round_in_place(hs_handle* F, int64_t* counts2) {
  if (!counts2) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hsk_round_factors_f32: counts2 == NULL");
  HsHandleView hv = hs_view_of(F, "hsk_round_factors_f32");
  HS_CHECK(probe_block_solve(F));
  if (!hv.device || !hv.factored) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hsk_round_factors_f32: handle holds no numeric factorization");
  HS_HIP(hipStreamSynchronize(hv.stream));
  unsigned long long c2[2] = {0, 0};
  if (hv.is_complex)
    round_in_place<cplx>(F, hv.stream, c2);
  else
    round_in_place<double>(F, hv.stream, c2);
  counts2[0] = (int64_t)c2[0];
  counts2[1] = (int64_t)c2[1];
}

int hs_f32_apply_prec(hs_f32* G, int trans, void* dC, int64_t ldc, const void* dB, int64_t ldb, int64_t n, int64_t nrhs, hipStream_t s) {
  if (G && G->cx) return hs_f32_ldiv_dev_z(G, trans, (double*)dC, ldc, (const double*)dB, ldb, n, nrhs, (void*)s);
  return hs_f32_ldiv_dev_d(G, trans, (double*)dC, ldc, (const double*)dB, ldb, n, nrhs, (void*)s);
}
int64_t hs_f32_size(const hs_f32* G) { return G ? G->n : 0; }
int hs_f32_is_complex(const hs_f32* G) { return G ? G->cx : 0; }

extern "C" int hs_f32_create(hs_handle* F, void* stream, hs_f32** G) { HS_GUARD(create_entry(F, stream, G)); }
HS_LDIV_FAMILY(hs_f32, hs_f32_ldiv, hs_f32_ldiv_dev, ldiv_host, ldiv_dev)
extern "C" int hs_f32_info(hs_f32* G, double* out8) {
  if (!G || !out8) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_f32_info: null argument");
    return HS_ERR_ARGUMENT;
  }
  double m[6] = {0, 0, 0, 0, 0, 0};
  hs_solve_multi_info(G->mx, m);
  out8[0] = m[0];
  out8[1] = G->value_bytes;
  out8[2] = 2.0 * G->value_bytes;
  out8[3] = G->other_bytes;
  out8[4] = m[5];
  out8[5] = G->flushed;
  out8[6] = m[4];
  out8[7] = G->t_demote;
  return HS_OK;
}
extern "C" void hs_f32_free(hs_f32* G) { delete G; }
