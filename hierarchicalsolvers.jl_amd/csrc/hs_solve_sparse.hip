// hs_solve_sparse.hip -- X = (op(F)^-1 B)[rows, :] for a sparse B (CSC) and a list of wanted rows (hs_ldiv_sparse_*), on pruned tree paths.
//
// A column of B that is zero on the interior of a front and of all its descendants leaves that front's forward sweep with exactly zero
// input, and a front none of whose descendants (itself included) holds a wanted row is never needed by the backward sweep.  So, per chunk of
// KC columns (hs_ldiv_block_cols()):
//
//   forward set  = the fronts that own a stored row of the chunk's columns, and their ancestors
//   backward set = the fronts that own a wanted row, and their ancestors
//
// both closed on the handle's INTERNAL front graph (HsSparseTree: the slices of a split front are a chain, the pseudo-root is the root's
// parent), which is the graph the sweeps walk.  The two block-solve drivers of hs_solve_multi.hip take the sets as an HsMultiActive and run
// their grouped launches over compacted SolveNode / MultiAux arrays; the per-front arithmetic is that of the dense block solve, and what is
// skipped is exactly zero there, so the wanted rows carry the bits of hs_ldiv_block_t_* on the expanded block.
//
// A front in the backward set that was not in the forward set has y = 0 for this chunk: its segment of work block 2 (which holds the x of an
// earlier chunk or call) is cleared before the backward sweep, all such fronts of a chunk in one launch.
//
// Column order: a stable sort by the node id of the front that owns the column's first stored row, empty columns last -- a chunk's sources
// are then neighbours in the tree and its forward set is small.  The block solve is column-independent, so the order changes no bits;
// results go back to the caller's column positions.  A chunk whose columns are all empty launches nothing and returns zeros.
//
// Everything a call needs is built on the host before the first launch and uploaded once: the index lists of every (chunk, level, sweep)
// subset, their MultiAux entries, the zero segments, the entry lists of the scatter, the wanted rows and the column positions.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "hs_solve_multi.h"
#include "../../include/hs_solver.h"
#include "hs_host.h"

void hs_sparse_plan(const HsSparseTree& t, int64_t nrhs, const int64_t* bcolptr, const int64_t* browval, int64_t base, const int64_t* rows, int64_t nrows,
                    HsSparsePlan* p) {
  const int KC = hs_ldiv_block_cols();
  const int nn = (int)t.parent.size();
  p->KC = KC;
  p->nchunks = (int)((nrhs + KC - 1) / KC);
  p->order.resize((size_t)nrhs);
  std::vector<int> key((size_t)nrhs);
  for (int64_t j = 0; j < nrhs; ++j) {
    p->order[j] = j;
    if (bcolptr[j + 1] == bcolptr[j]) {
      key[j] = INT_MAX;
    } else {
      const int own = t.owner[browval[bcolptr[j] - base] - base];
      key[j] = own < 0 ? INT_MAX - 1 : t.user[own];
    }
  }
  std::stable_sort(p->order.begin(), p->order.end(), [&](int64_t a, int64_t b) { return key[a] < key[b]; });
  // marks own and its ancestors; the walk ends at the first node already marked (its ancestors are marked too)
  auto climb = [&](unsigned char* m, int own, unsigned char bit) {
    if (own < 0) {  // a row no front eliminates: nothing is known about it, every front is visited
      for (int i = 0; i < nn; ++i) m[i] |= bit;
      return;
    }
    for (int i = own; i >= 0 && !(m[i] & bit); i = t.parent[i]) m[i] |= bit;
  };
  std::vector<unsigned char> bm((size_t)nn, 0);  // the backward set is the same for every chunk
  if (!rows) {
    std::fill(bm.begin(), bm.end(), 2);
  } else {
    for (int64_t r = 0; r < nrows; ++r) climb(bm.data(), t.owner[rows[r] - base], 2);
  }
  p->act.assign((size_t)p->nchunks * nn, 0);
  p->visits[0] = p->visits[1] = 0.0;
  p->model = 0.0;
  for (int c = 0; c < p->nchunks; ++c) {
    unsigned char* m = p->act.data() + (size_t)c * nn;
    bool any = false;
    for (int64_t q = (int64_t)c * KC; q < std::min<int64_t>(nrhs, (int64_t)(c + 1) * KC); ++q) {
      const int64_t j = p->order[q];
      for (int64_t e = bcolptr[j] - base; e < bcolptr[j + 1] - base; ++e) {
        climb(m, t.owner[browval[e] - base], 1);
        any = true;
      }
    }
    if (!any) continue;  // zero columns only: zero solution, no sweep
    for (int i = 0; i < nn; ++i) {
      m[i] |= bm[i];
      const double w = 0.5 * t.ni[i] * (double)t.ni[i] + (double)t.ni[i] * t.nb[i];
      if (m[i] & 1) { p->visits[0] += 1.0; p->model += w; }
      if (m[i] & 2) { p->visits[1] += 1.0; p->model += w; }
    }
  }
}

namespace {
template <class T>
struct SparseCtx {
  T* W = nullptr;  // the chunk: n x KC, column-major
  int64_t n = 0;
  const T* bval = nullptr;
  const int *erow = nullptr, *ecol = nullptr;
  const long long* esrc = nullptr;
  const std::vector<long long>* eoff = nullptr;  // entries of chunk c: [eoff[c], eoff[c + 1])
  T* X = nullptr;
  int64_t ldx = 0, nout = 0;
  const int* rows = nullptr;        // device, 0-based; null: every row
  const long long* xcol = nullptr;  // device: caller's column of every processed column
  const int64_t* order = nullptr;   // the same on the host
  int KC = 0;
};
template <class T>
void chunk_begin(void* ctx, int c, int kc, hipStream_t s) {
  const SparseCtx<T>& x = *(const SparseCtx<T>*)ctx;
  const long long e0 = (*x.eoff)[c], e1 = (*x.eoff)[c + 1];
  if (e1 == e0) return;
  HS_HIP(hipMemsetAsync(x.W, 0, (size_t)x.n * kc * sizeof(T), s));
  launch_sparse_scatter<T>(x.W, x.n, x.bval, x.erow + e0, x.ecol + e0, x.esrc + e0, e1 - e0, s);
}
template <class T>
void chunk_end(void* ctx, int c, int kc, hipStream_t s) {
  const SparseCtx<T>& x = *(const SparseCtx<T>*)ctx;
  if ((*x.eoff)[c + 1] == (*x.eoff)[c]) {  // zero columns
    for (int j = 0; j < kc; ++j) HS_HIP(hipMemsetAsync(x.X + x.order[(int64_t)c * x.KC + j] * x.ldx, 0, (size_t)x.nout * sizeof(T), s));
    return;
  }
  launch_sparse_gather<T>(x.X, x.ldx, x.xcol + (long long)c * x.KC, x.W, x.n, x.rows, x.nout, kc, s);
}

struct Packer {  // the host image of the call's lists, every section 16-byte aligned
  std::vector<char> buf;
  size_t add(const void* p, size_t bytes) {
    const size_t off = (buf.size() + 15) / 16 * 16;
    buf.resize(off + bytes);
    if (bytes) memcpy(buf.data() + off, p, bytes);
    return off;
  }
};
}  // namespace

template <class T>
void hs_solve_sparse_run(const HsMultiView& v, const HsSparseTree& t, int trans, int64_t nrhs, const int64_t* bcolptr, const int64_t* browval, const T* d_bval,
                         const int64_t* rows, int64_t nrows, T* dX, int64_t ldx, hipStream_t s, double* out8) {
  HsSparsePlan p;
  hs_sparse_plan(t, nrhs, bcolptr, browval, 1, rows, nrows, &p);
  const int KC = p.KC, nn = (int)t.parent.size(), nl = (int)v.levels.size();
  const int64_t n = v.n, nout = rows ? nrows : n;

  // ---- the subsets of every (chunk, level, sweep), their index lists and MultiAux entries
  HsMultiActive A;
  A.nlevels = nl;
  A.sub.resize((size_t)p.nchunks * nl * 2);
  const char* base = nullptr;  // the handle's SolveNode array: the levels' arrays are ranges of it
  for (const HsMultiLevel& L : v.levels)
    if (L.sn && (!base || (const char*)L.sn < base)) base = (const char*)L.sn;
  std::vector<long long> idx;
  std::vector<MultiAux> aux;
  std::vector<size_t> sub_off(A.sub.size(), 0);
  std::vector<HsZeroSeg> zseg;
  A.zoff.assign((size_t)p.nchunks + 1, 0);
  A.zmaxni.assign((size_t)p.nchunks, 0);
  std::vector<std::vector<long long>> boff(nl);
  for (int lv = 0; lv < nl; ++lv) {
    long long b = 0;
    for (const HsMultiFront& f : v.levels[lv].fronts) {
      boff[lv].push_back(b);
      b += f.nb;
    }
  }
  for (int c = 0; c < p.nchunks; ++c) {
    const unsigned char* m = p.act.data() + (size_t)c * nn;
    for (int lv = 0; lv < nl; ++lv) {
      const HsMultiLevel& L = v.levels[lv];
      const long long first = L.sn ? ((const char*)L.sn - base) / (long long)sizeof(SolveNode<T>) : 0;
      for (int sweep = 0; sweep < 2; ++sweep) {
        HsMultiSubset& q = A.sub[((size_t)c * nl + lv) * 2 + sweep];
        sub_off[((size_t)c * nl + lv) * 2 + sweep] = idx.size();
        for (int i = 0; i < L.nfronts; ++i) {
          if (!(m[L.node[i]] & (1 << sweep))) continue;
          const HsMultiFront& f = L.fronts[i];
          q.pos.push_back(i);
          q.maxni = std::max(q.maxni, f.ni);
          q.maxnb = std::max(q.maxnb, f.nb);
          idx.push_back(first + i);
          aux.push_back({boff[lv][i], f.nb, 0});
          if (sweep == 1 && !(m[L.node[i]] & 1) && f.ni > 0) {
            zseg.push_back({f.woff, f.ni, 0});
            A.zmaxni[c] = std::max(A.zmaxni[c], f.ni);
          }
        }
      }
    }
    A.zoff[c + 1] = zseg.size();
  }

  // ---- the entry lists of the scatter, chunk after chunk in processing order
  const long long nnzb = nrhs > 0 ? bcolptr[nrhs] - bcolptr[0] : 0;
  std::vector<int> erow, ecol;
  std::vector<long long> esrc, eoff((size_t)p.nchunks + 1, 0);
  erow.reserve(nnzb); ecol.reserve(nnzb); esrc.reserve(nnzb);
  for (int c = 0; c < p.nchunks; ++c) {
    for (int64_t q = (int64_t)c * KC; q < std::min<int64_t>(nrhs, (int64_t)(c + 1) * KC); ++q) {
      const int64_t j = p.order[q];
      for (int64_t e = bcolptr[j] - 1; e < bcolptr[j + 1] - 1; ++e) {
        erow.push_back((int)(browval[e] - 1));
        ecol.push_back((int)(q - (int64_t)c * KC));
        esrc.push_back(e - (bcolptr[0] - 1));
      }
    }
    eoff[c + 1] = (long long)erow.size();
  }
  std::vector<int> rows0;
  if (rows) {
    rows0.resize((size_t)nrows);
    for (int64_t r = 0; r < nrows; ++r) rows0[r] = (int)(rows[r] - 1);
  }
  std::vector<long long> xcol(p.order.begin(), p.order.end());

  Packer pk;
  const size_t o_idx = pk.add(idx.data(), idx.size() * sizeof(long long));
  const size_t o_aux = pk.add(aux.data(), aux.size() * sizeof(MultiAux));
  const size_t o_zs = pk.add(zseg.data(), zseg.size() * sizeof(HsZeroSeg));
  const size_t o_er = pk.add(erow.data(), erow.size() * sizeof(int));
  const size_t o_ec = pk.add(ecol.data(), ecol.size() * sizeof(int));
  const size_t o_es = pk.add(esrc.data(), esrc.size() * sizeof(long long));
  const size_t o_rw = pk.add(rows0.data(), rows0.size() * sizeof(int));
  const size_t o_xc = pk.add(xcol.data(), xcol.size() * sizeof(long long));
  const size_t o_sn = pk.add(nullptr, 0);  // the compacted SolveNode array follows the lists
  const size_t lbytes = o_sn + std::max<size_t>(idx.size(), 1) * sizeof(SolveNode<T>);
  const size_t wbytes = (size_t)n * KC * sizeof(T);

  {
    HsScratch lists(lbytes, "sparse solve lists"), chunk(wbytes, "sparse solve chunk");
    HsDrain drain{s};
    char* dl = (char*)lists.p;
    T* W = (T*)chunk.p;
    if (!pk.buf.empty()) HS_HIP(hipMemcpy(dl, pk.buf.data(), pk.buf.size(), hipMemcpyHostToDevice));
    launch_sparse_compact<T>((SolveNode<T>*)(dl + o_sn), (const SolveNode<T>*)base, (const long long*)(dl + o_idx), (long long)idx.size(), s);
    for (size_t k = 0; k < A.sub.size(); ++k) {
      A.sub[k].sn = (const SolveNode<T>*)(dl + o_sn) + sub_off[k];
      A.sub[k].aux = (const MultiAux*)(dl + o_aux) + sub_off[k];
    }
    A.zseg = (const HsZeroSeg*)(dl + o_zs);
    SparseCtx<T> cx;
    cx.W = W; cx.n = n; cx.bval = d_bval;
    cx.erow = (const int*)(dl + o_er); cx.ecol = (const int*)(dl + o_ec); cx.esrc = (const long long*)(dl + o_es);
    cx.eoff = &eoff;
    cx.X = dX; cx.ldx = ldx; cx.nout = nout;
    cx.rows = rows ? (const int*)(dl + o_rw) : nullptr;
    cx.xcol = (const long long*)(dl + o_xc);
    cx.order = p.order.data();
    cx.KC = KC;
    A.ctx = &cx;
    A.begin = chunk_begin<T>;
    A.end = chunk_end<T>;
    hs_solve_multi_run<T>(v, trans, W, n, nrhs, s, &A);
    HS_HIP(hipStreamSynchronize(s));  // the lists and the chunk go back to the scratch cache
  }
  out8[0] = 0.0;
  out8[1] = p.model * sizeof(T);
  out8[2] = p.visits[0];
  out8[3] = p.visits[1];
  out8[4] = (double)nn * p.nchunks;
  out8[5] = (double)p.nchunks;
  out8[6] = 0.0;
  out8[7] = (double)(lbytes + wbytes);
}
#define INST(T)                                                                                                                                     \
  template void hs_solve_sparse_run<T>(const HsMultiView&, const HsSparseTree&, int, int64_t, const int64_t*, const int64_t*, const T*, const int64_t*, \
                                       int64_t, T*, int64_t, hipStream_t, double*);
INST(double)
INST(cplx)
