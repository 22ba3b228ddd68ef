// hs_normest.h -- the one block 1-norm estimator of the accuracy tools (Higham & Tisseur, SIAM J. Matrix Anal. Appl. 21(4), 2000, Algorithm
// 2.4): its kernels and its host engine.  Included by hs_condest.hip and hs_refine_block.hip only, after hs_condest.h with HS_CONDEST_KERNELS
// (fma contraction is off from there on).
//
// est_run advances `ne` estimators of B_e = diag(v_e) op(F)^-1 in lockstep, t columns each, and shares ONE application of op(F)^-1 and one of
// its adjoint per iteration among those still active; hs_normestinv, hs_condest and the ferr of hs_ldiv_refine_* are the case ne = 1, the
// ferr of hs_ldiv_refine_block_* runs a group of columns.  An estimator's X, S, S_old, v, index history and best index live at its own place
// e; Y and Z, which travel through the solve, are gathered into the leading slots, so a finished estimator costs nothing.  The host reads the
// scalars of all active estimators with one synchronisation per half-step (plus those of the redraw loop) and checks the dataflow flag after
// each.  tests/normest_mirror.py restates one estimator in NumPy step for step, tests/refine_block_mirror.py the lockstep schedule.
//
// The kernels are templated on MAXT, the compile-time bound on t that sizes the LDS and register arrays of the top-t selection: <2> serves
// the forward error bounds (t = min(2, n), 5 iterations), <8> hs_normestinv and hs_condest (t <= 8, at most 16 iterations).
//
// Determinism: the +-1 columns are the low bit of splitmix64 over (row, column, draw, hs_options.seed) -- no RNG state, no dependence on the
// right-hand side; every floating-point reduction is per (workgroup, column) partials of CE_ROWS rows in LDS and one ordered final pass per
// column; the only atomics are on integers (exact +-1 dot products).  An estimator's results depend on neither its slot, the other
// estimators nor ne, and two calls return the same bits.
#pragma once
#ifndef HS_CONDEST_KERNELS
#error "include hs_condest.h with HS_CONDEST_KERNELS defined before hs_normest.h"
#endif
#include <cmath>
#include <cstring>
#include <deque>
#include <utility>
#include <vector>

namespace hs_ce {

// The host <-> device traffic of a driver: small uploads whose host side lives until the next synchronisation, and the one synchronisation
// of a half-step, which reads `cnt` doubles into hd and checks the dataflow-sweep flag (a timed-out sweep is an error, never a result).
struct HostIo {
  hs_handle* F;
  hipStream_t s;
  std::vector<double> hd;                 // what the host read last
  std::deque<std::vector<char>> pending;  // host sides of uploads in flight
  ~HostIo() {
    if (!pending.empty()) (void)hipStreamSynchronize(s);  // an error path: no upload may outlive its host side
  }
  void upload(void* dst, const void* src, size_t bytes) {
    if (!bytes) return;
    pending.emplace_back((const char*)src, (const char*)src + bytes);
    HS_HIP(hipMemcpyAsync(dst, pending.back().data(), bytes, hipMemcpyHostToDevice, s));
  }
  void read(const void* d, size_t cnt) {
    if (hd.size() < cnt) hd.resize(cnt);
    HS_HIP(hipMemcpyAsync(hd.data(), d, sizeof(double) * cnt, hipMemcpyDeviceToHost, s));
    HS_HIP(hipStreamSynchronize(s));
    pending.clear();
    HS_CHECK(hs_handle_flow_check(F));
  }
};

// per MAXT: the index history of one estimator (t rows join it per iteration) and the doubles of its selection result
template <int MAXT>
struct EstDim {
  static constexpr int ITMAX = MAXT <= 2 ? 5 : 16;  // the most iterations a caller may ask for
  static constexpr int HIST = MAXT <= 2 ? MAXT * (ITMAX + 1) : MAXT * ITMAX;
  static constexpr int RES = 8 + MAXT;
};

namespace {

// ---- kernels ----------------------------------------------------------------------------------------------------------------------------
// An active estimator is one entry of the device list `act`: x = its place e (where its X, S, S_old, v and history live), y = its slot in
// Y / Z.  The list holds the active estimators only.  The estimator of list entry a is blockIdx.y (or blockIdx.y / columns).
#define EST_NONE_I 0x7fffffffffffffffll

// X[:, (e, 0)] = 1/n, X[:, (e, j)] = +-1/n for every estimator e   (grid: nb256 x ne)
template <class T>
__global__ __launch_bounds__(256) void est_init_kernel(T* __restrict__ X, int64_t n, int t, int64_t seed, double inv_n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  T* x = X + (size_t)blockIdx.y * t * n;
  x[i] = from_real<T>(inv_n);
  for (int j = 1; j < t; ++j) x[(size_t)j * n + i] = from_real<T>(pm1(col_key(seed, j, 0), i) * inv_n);
}
// Dst[:, (a, j)] = op(Src[:, (act[a].x, j)] (* v[:, act[a].x])), op = conj with cj: the input of an application, compacted   (grid: nb256 x nact)
template <class T>
__global__ __launch_bounds__(256) void est_gather_kernel(const T* __restrict__ Src, T* __restrict__ Dst, int64_t n, int t, const int2* __restrict__ act,
                                                         const double* __restrict__ v, int cj) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int a = blockIdx.y, e = act[a].x;
  const double sc = v ? v[(size_t)e * n + i] : 1.0;
  for (int j = 0; j < t; ++j) {
    T x = Src[((size_t)e * t + j) * n + i];
    if (v) x = scale_(x, sc);
    if (cj) x = cj_<true>(x);
    Dst[((size_t)a * t + j) * n + i] = x;
  }
}
// Y[:, (a, j)] = op(Y[:, (a, j)]) (* v[:, act[a].x]): the output of an application   (grid: nb256 x nact)
template <class T>
__global__ __launch_bounds__(256) void est_post_kernel(T* __restrict__ Y, int64_t n, int t, const int2* __restrict__ act, const double* __restrict__ v, int cj) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int a = blockIdx.y;
  const double sc = v ? v[(size_t)act[a].x * n + i] : 1.0;
  for (int j = 0; j < t; ++j) {
    T y = Y[((size_t)a * t + j) * n + i];
    if (cj) y = cj_<true>(y);
    if (v) y = scale_(y, sc);
    Y[((size_t)a * t + j) * n + i] = y;
  }
}
// part[q * nblk + b] = sum over the workgroup's rows of |Y[i, q]|, q = (a, j)   (grid: nblk x nact t)
template <class T>
__global__ __launch_bounds__(256) void est_colnorm_part_kernel(const T* __restrict__ Y, int64_t n, double* __restrict__ part) {
  __shared__ double sh[256];
  const int q = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * CE_ROWS;
  double acc = 0.0;
  for (int k = 0; k < CE_ROWS / 256; ++k) {
    const int64_t i = i0 + k * 256 + threadIdx.x;
    if (i < n) acc += abs_(Y[(size_t)q * n + i]);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)q * gridDim.x + blockIdx.x] = sh[0];
}
// res[2 a] = max_j ||Y[:, (a, j)]||_1, res[2 a + 1] = the first j that attains it   (one workgroup per estimator)
template <int MAXT>
__global__ __launch_bounds__(256) void est_colnorm_final_kernel(const double* __restrict__ part, int nblk, int t, double* __restrict__ res) {
  __shared__ double sh[256];
  __shared__ double nrm[MAXT];
  const int a = blockIdx.x;
  for (int j = 0; j < t; ++j) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) acc += part[((size_t)a * t + j) * nblk + b];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) nrm[j] = sh[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double est = nrm[0];
    int jm = 0;
    for (int j = 1; j < t; ++j)
      if (nrm[j] > est) {
        est = nrm[j];
        jm = j;
      }
    res[2 * a] = est;
    res[2 * a + 1] = (double)jm;
  }
}
// S[:, (act[a].x, j)] = sign(Y[:, (act[a].y, j)]) (sign(0) = 1; complex: Y / |Y|)   (grid: nb256 x t x nact)
template <class T>
__global__ __launch_bounds__(256) void est_sign_kernel(const T* __restrict__ Y, T* __restrict__ S, int64_t n, int t, const int2* __restrict__ act) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int2 a = act[blockIdx.z];
  const int j = blockIdx.y;
  S[((size_t)a.x * t + j) * n + i] = sign_(Y[((size_t)a.y * t + j) * n + i]);
}
// out[a np + p] += the workgroup's part of S_j . O_q for p = (j - j0) 2t + q, O = [S  S_old] of estimator act[a].x: exact integers (+-1
// entries) summed with integer atomics, so the result does not depend on their order   (grid: nblk x nact np, np = (j1 - j0) 2t)
__global__ __launch_bounds__(256) void est_pm_dots_kernel(const double* __restrict__ S, const double* __restrict__ So, int64_t n, int t, int j0, int np,
                                                          const int2* __restrict__ act, unsigned long long* __restrict__ out) {
  __shared__ long long sh[256];
  const int a = blockIdx.y / np, p = blockIdx.y % np;
  const int j = j0 + p / (2 * t), q = p % (2 * t);
  const size_t base = (size_t)act[a].x * t * n;
  const double* u = S + base + (size_t)j * n;
  const double* o = q < t ? S + base + (size_t)q * n : So + base + (size_t)(q - t) * n;
  const int64_t i0 = (int64_t)blockIdx.x * CE_ROWS;
  long long acc = 0;
  for (int k = 0; k < CE_ROWS / 256; ++k) {
    const int64_t i = i0 + k * 256 + threadIdx.x;
    if (i < n) acc += (u[i] == o[i]) ? 1 : -1;
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(out + (size_t)a * np + p, (unsigned long long)sh[0]);
}
// S[:, (act[a].x, j)] = the +-1 column of `key`   (grid: nb256 x nact)
__global__ __launch_bounds__(256) void est_resample_kernel(double* __restrict__ S, int64_t n, int t, int j, const int2* __restrict__ act, uint64_t key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) S[((size_t)act[blockIdx.y].x * t + j) * n + i] = pm1(key, i);
}

// top-t selection: order = h descending, ties by ascending index; the estimator's history is excluded
__device__ inline bool better(double ha, long long ia, double hb, long long ib) { return ha > hb || (ha == hb && ia < ib); }
__device__ inline bool in_hist(const long long* hs, int cnt, long long i) {
  for (int k = 0; k < cnt; ++k)
    if (hs[k] == i) return true;
  return false;
}
__device__ inline void list_insert(double* lh, long long* li, int t, double hv, long long iv) {
  if (!better(hv, iv, lh[t - 1], li[t - 1])) return;
  int k = t - 1;
  while (k > 0 && better(hv, iv, lh[k - 1], li[k - 1])) {
    lh[k] = lh[k - 1];
    li[k] = li[k - 1];
    --k;
  }
  lh[k] = hv;
  li[k] = iv;
}
// merge the sorted lists of LDS slots a and b (t entries each) into slot a
template <int MAXT>
__device__ inline void list_merge(double (*sh)[MAXT], long long (*si)[MAXT], int a, int b, int t) {
  double oh[MAXT];
  long long oi[MAXT];
  int x = 0, y = 0;
  for (int k = 0; k < t; ++k) {
    if (better(sh[a][x], si[a][x], sh[b][y], si[b][y])) {
      oh[k] = sh[a][x];
      oi[k] = si[a][x++];
    } else {
      oh[k] = sh[b][y];
      oi[k] = si[b][y++];
    }
  }
  for (int k = 0; k < t; ++k) {
    sh[a][k] = oh[k];
    si[a][k] = oi[k];
  }
}
// the 256 sorted lists and maxima of a workgroup -> slot 0, by a fixed tree
template <int MAXT>
__device__ inline void list_reduce(double (*sh)[MAXT], long long (*si)[MAXT], double* smax, int t) {
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      list_merge<MAXT>(sh, si, threadIdx.x, threadIdx.x + st, t);
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + st]);
    }
    __syncthreads();
  }
}
template <class T>
__device__ inline double rowmax_(const T* __restrict__ Z, int64_t n, int t, int64_t i) {  // h_i = max_j |Z[i, j]|
  double hv = 0.0;
  for (int j = 0; j < t; ++j) hv = fmax(hv, abs_(Z[(size_t)j * n + i]));
  return hv;
}
// per (workgroup, estimator): the best t rows of h outside the estimator's history, and the max of h   (grid: nblk x nact; Z in slot a)
template <class T, int MAXT>
__global__ __launch_bounds__(256) void est_rowmax_top_kernel(const T* __restrict__ Z, int64_t n, int t, const int2* __restrict__ act,
                                                             const long long* __restrict__ hist, const int* __restrict__ hcnt, double* __restrict__ cand_h,
                                                             long long* __restrict__ cand_i, double* __restrict__ bmax) {
  __shared__ double sh[256][MAXT];
  __shared__ long long si[256][MAXT];
  __shared__ double smax[256];
  const int a = blockIdx.y, e = act[a].x;
  const long long* hs = hist + (size_t)e * EstDim<MAXT>::HIST;
  const int hc = hcnt[e];
  const T* Za = Z + (size_t)a * t * n;
  double lh[MAXT];
  long long li[MAXT];
  for (int k = 0; k < MAXT; ++k) {
    lh[k] = -1.0;
    li[k] = EST_NONE_I;
  }
  double m = -1.0;
  const int64_t i0 = (int64_t)blockIdx.x * CE_ROWS;
  for (int q = 0; q < CE_ROWS / 256; ++q) {
    const int64_t i = i0 + q * 256 + threadIdx.x;
    if (i >= n) break;
    const double hv = rowmax_(Za, n, t, i);
    m = fmax(m, hv);
    if (better(hv, i, lh[t - 1], li[t - 1]) && !in_hist(hs, hc, i)) list_insert(lh, li, t, hv, i);
  }
  for (int k = 0; k < t; ++k) {
    sh[threadIdx.x][k] = lh[k];
    si[threadIdx.x][k] = li[k];
  }
  smax[threadIdx.x] = m;
  list_reduce<MAXT>(sh, si, smax, t);
  const size_t o = (size_t)a * gridDim.x + blockIdx.x;
  if ((int)threadIdx.x < t) {
    cand_h[o * MAXT + threadIdx.x] = sh[0][threadIdx.x];
    cand_i[o * MAXT + threadIdx.x] = si[0][threadIdx.x];
  }
  if (threadIdx.x == 0) bmax[o] = smax[0];
}
// one workgroup per estimator, r = res + a RES: r[2] = max h, r[3] = h[ind_best] (-1 when none), r[4] = 1 if the top t rows are all in the
// history, r[5] = rows selected, r[8 + j] = the j-th row outside the history
template <class T, int MAXT>
__global__ __launch_bounds__(256) void est_select_final_kernel(const T* __restrict__ Z, int64_t n, int t, const int2* __restrict__ act,
                                                               const long long* __restrict__ hist, const int* __restrict__ hcnt,
                                                               const double* __restrict__ cand_h, const long long* __restrict__ cand_i,
                                                               const double* __restrict__ bmax, int nblk, const long long* __restrict__ ind_best,
                                                               double* __restrict__ res) {
  __shared__ double sh[256][MAXT];
  __shared__ long long si[256][MAXT];
  __shared__ double smax[256];
  const int a = blockIdx.x, e = act[a].x;
  const T* Za = Z + (size_t)a * t * n;
  double lh[MAXT];
  long long li[MAXT];
  for (int k = 0; k < MAXT; ++k) {
    lh[k] = -1.0;
    li[k] = EST_NONE_I;
  }
  double m = -1.0;
  cand_h += (size_t)a * nblk * MAXT;
  cand_i += (size_t)a * nblk * MAXT;
  bmax += (size_t)a * nblk;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    for (int k = 0; k < t; ++k) list_insert(lh, li, t, cand_h[(size_t)b * MAXT + k], cand_i[(size_t)b * MAXT + k]);
    m = fmax(m, bmax[b]);
  }
  for (int k = 0; k < t; ++k) {
    sh[threadIdx.x][k] = lh[k];
    si[threadIdx.x][k] = li[k];
  }
  smax[threadIdx.x] = m;
  list_reduce<MAXT>(sh, si, smax, t);
  if (threadIdx.x == 0) {
    double* r = res + (size_t)a * EstDim<MAXT>::RES;
    int nsel = 0;
    for (int k = 0; k < t; ++k) {
      if (si[0][k] == EST_NONE_I) break;
      r[8 + k] = (double)si[0][k];
      ++nsel;
    }
    int above = 0;  // history rows that rank before the best row outside it
    const int hc = hcnt[e];
    for (int k = 0; k < hc; ++k) {
      const long long i = hist[(size_t)e * EstDim<MAXT>::HIST + k];
      if (nsel == 0 || better(rowmax_(Za, n, t, i), i, sh[0][0], si[0][0])) ++above;
    }
    const long long ib = ind_best[a];
    r[2] = smax[0];
    r[3] = ib >= 0 ? rowmax_(Za, n, t, ib) : -1.0;
    r[4] = above >= t ? 1.0 : 0.0;
    r[5] = (double)nsel;
  }
}
// X[:, (act[a].x, j)] = e_{sel[a t + j]}; the selection joins the estimator's history   (grid: nb256 x nact)
template <class T, int MAXT>
__global__ __launch_bounds__(256) void est_unit_kernel(T* __restrict__ X, int64_t n, int t, const int2* __restrict__ act, const long long* __restrict__ sel,
                                                       long long* __restrict__ hist, int* __restrict__ hcnt) {
  const int a = blockIdx.y, e = act[a].x;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int hc = hcnt[e];
    for (int j = 0; j < t; ++j) hist[(size_t)e * EstDim<MAXT>::HIST + hc + j] = sel[(size_t)a * t + j];
    hcnt[e] = hc + t;
  }
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (int j = 0; j < t; ++j) X[((size_t)e * t + j) * n + i] = from_real<T>(i == sel[(size_t)a * t + j] ? 1.0 : 0.0);
}

// ---- the workspace of ne estimators --------------------------------------------------------------------------------------------------
template <class T, int MAXT>
struct EstWork {
  using Dim = EstDim<MAXT>;
  int64_t n = 0;
  int t = 0, nblk = 0;
  T *X = nullptr, *Y = nullptr, *S = nullptr, *So = nullptr, *Z = nullptr;
  double *part = nullptr, *cand_h = nullptr, *bmax = nullptr, *res = nullptr;
  long long *cand_i = nullptr, *hist = nullptr, *ibest = nullptr, *sel = nullptr;
  unsigned long long* dots = nullptr;
  int* hcnt = nullptr;
  int2* act = nullptr;
  static size_t bytes_per_estimator(int64_t n) {
    const size_t t = (size_t)std::min<int64_t>(MAXT, n), nblk = (size_t)nbrows(n);
    return 5 * t * (size_t)n * sizeof(T) + nblk * (t * sizeof(double) + MAXT * (sizeof(double) + sizeof(long long)) + sizeof(double)) + Dim::RES * sizeof(double) +
           (Dim::HIST + 1 + MAXT) * sizeof(long long) + 2 * MAXT * MAXT * sizeof(unsigned long long) + sizeof(int) + sizeof(int2);
  }
  void alloc(HsDevBuf& buf, int64_t n_, int t_, size_t ne) {
    n = n_;
    t = t_;
    nblk = (int)nbrows(n);
    const size_t blk = ne * (size_t)n * t;
    X = buf.get<T>(blk);
    Y = buf.get<T>(blk);
    S = buf.get<T>(blk);
    So = buf.get<T>(blk);
    Z = buf.get<T>(blk);
    part = buf.get<double>(ne * nblk * t);
    cand_h = buf.get<double>(ne * nblk * MAXT);
    cand_i = buf.get<long long>(ne * nblk * MAXT);
    bmax = buf.get<double>(ne * nblk);
    res = buf.get<double>(ne * Dim::RES);
    hist = buf.get<long long>(ne * Dim::HIST);
    ibest = buf.get<long long>(ne);
    sel = buf.get<long long>(ne * MAXT);
    dots = buf.get<unsigned long long>(ne * 2 * MAXT * MAXT);
    hcnt = buf.get<int>(ne);
    act = buf.get<int2>(ne);
  }
};

// ---- the host engine -------------------------------------------------------------------------------------------------------------------
// est[e] = the estimate of || diag(v_e) op_fwd(F)^-1 ||_1 for e < ne (v_e = v[e n ..], v == nullptr: no scaling), t = w.t columns each, at
// most itmax iterations, on a workspace allocated for at least ne estimators.  solve(trans, blk, nc) applies F^-1 / F^-T / F^-H (trans 0,
// 1, 2) in place to the leading nc columns of blk (leading dimension n); the engine conjugates and scales around it.  The steps are numbered
// as in tests/normest_mirror.py.
template <class T, int MAXT, class Solve>
void est_run(HostIo& io, EstWork<T, MAXT> w, int64_t seed, int fwd, const double* v, int ne, int itmax, Solve&& solve, double* est) {
  using Dim = EstDim<MAXT>;
  const int64_t n = w.n;
  const int t = w.t, nblk = w.nblk;
  if (t < 1 || t > MAXT || t > n || itmax < 1 || itmax > Dim::ITMAX)
    HS_FAIL(HS_ERR_ARGUMENT, t, "ArgumentError: the 1-norm estimator takes t in 1:min(%d, n) and itmax in 1:%d, got t = %d, itmax = %d", MAXT, Dim::ITMAX, t, itmax);
  hipStream_t s = io.s;
  const unsigned gn = nb256(n);
  const bool real = sizeof(T) == 8;
  const long long nn = (long long)n;
  const OpDir df = op_dir<T>(fwd), da = op_dir<T>(adj(fwd));
  struct Est {
    int id, ys = 0;
    double est = 0.0, est_old = 0.0;
    long long ind[MAXT] = {};
    long long ind_best = -1;
  };
  std::vector<Est> E((size_t)ne);
  std::vector<int> A((size_t)ne);  // the active estimators
  for (int c = 0; c < ne; ++c) {
    E[(size_t)c].id = c;
    A[(size_t)c] = c;
  }
  std::vector<int2> hact((size_t)ne);
  std::vector<long long> hll((size_t)ne * MAXT);
  std::vector<long long> D;
  auto set_act = [&](const std::vector<int>& L) {
    for (size_t a = 0; a < L.size(); ++a) hact[a] = make_int2(E[(size_t)L[a]].id, E[(size_t)L[a]].ys);
    io.upload(w.act, hact.data(), sizeof(int2) * L.size());
  };
  // exact +-1 dot products of the sign columns j0 .. j1-1 with [S  S_old] for the estimators of L: D[a np + (j - j0) 2t + q]
  auto pm_dots = [&](const std::vector<int>& L, int j0, int j1) {
    const int np = (j1 - j0) * 2 * t;
    const size_t cnt = L.size() * (size_t)np;
    set_act(L);
    HS_HIP(hipMemsetAsync(w.dots, 0, sizeof(unsigned long long) * cnt, s));
    hipLaunchKernelGGL(est_pm_dots_kernel, dim3(nblk, (unsigned)cnt), dim3(256), 0, s, (const double*)w.S, (const double*)w.So, n, t, j0, np, (const int2*)w.act,
                       w.dots);
    io.read(w.dots, cnt);
    D.resize(cnt);
    std::memcpy(D.data(), io.hd.data(), sizeof(long long) * cnt);
    return np;
  };
  // 1. start
  hipLaunchKernelGGL(est_init_kernel<T>, dim3(gn, ne), dim3(256), 0, s, w.X, n, t, seed, 1.0 / (double)n);
  HS_HIP(hipMemsetAsync(w.hcnt, 0, sizeof(int) * (size_t)ne, s));
  for (int k = 1; !A.empty(); ++k) {
    // 2. Y = B X, est = max_j ||Y[:, j]||_1, for every active estimator with one application
    int na = (int)A.size();
    set_act(A);
    hipLaunchKernelGGL(est_gather_kernel<T>, dim3(gn, na), dim3(256), 0, s, (const T*)w.X, w.Y, n, t, (const int2*)w.act, (const double*)nullptr, df.conj ? 1 : 0);
    solve(df.trans, w.Y, (int64_t)na * t);
    if (df.conj || v) hipLaunchKernelGGL(est_post_kernel<T>, dim3(gn, na), dim3(256), 0, s, w.Y, n, t, (const int2*)w.act, v, df.conj ? 1 : 0);
    hipLaunchKernelGGL(est_colnorm_part_kernel<T>, dim3(nblk, na * t), dim3(256), 0, s, (const T*)w.Y, n, w.part);
    hipLaunchKernelGGL(est_colnorm_final_kernel<MAXT>, dim3(na), dim3(256), 0, s, (const double*)w.part, nblk, t, w.res);
    io.read(w.res, (size_t)2 * na);
    std::vector<int> L;
    for (int a = 0; a < na; ++a) {
      Est& q = E[(size_t)A[(size_t)a]];
      q.ys = a;
      q.est = io.hd[(size_t)2 * a];
      const int jmax = (int)io.hd[(size_t)2 * a + 1];
      if ((q.est > q.est_old || k == 2) && k >= 2) q.ind_best = q.ind[jmax];
      if (k >= 2 && q.est <= q.est_old) {
        q.est = q.est_old;
        continue;
      }
      // 3. iteration limit
      q.est_old = q.est;
      if (k > itmax) continue;
      L.push_back(A[(size_t)a]);
    }
    A.swap(L);
    if (A.empty()) break;
    std::swap(w.S, w.So);  // S_old = S (every active estimator is at iteration k)
    const bool have_old = k >= 2;
    // 4. signs
    na = (int)A.size();
    set_act(A);
    hipLaunchKernelGGL(est_sign_kernel<T>, dim3(gn, t, na), dim3(256), 0, s, (const T*)w.Y, w.S, n, t, (const int2*)w.act);
    // 5. parallel columns (real only)
    if (real) {
      if (have_old) {
        const int np = pm_dots(A, 0, t);
        L.clear();
        for (int a = 0; a < na; ++a) {
          bool all_par = true;
          for (int j = 0; j < t && all_par; ++j) {
            bool par = false;
            for (int q = 0; q < t; ++q) par |= std::llabs(D[(size_t)a * np + (size_t)j * 2 * t + t + q]) == nn;
            all_par &= par;
          }
          if (!all_par) L.push_back(A[(size_t)a]);
        }
        A.swap(L);
        if (A.empty()) break;
      }
      if (t > 1) {
        for (int j = 0; j < t; ++j) {
          if (j == 0 && !have_old) continue;
          std::vector<int> need = A;
          for (int attempt = 1; !need.empty(); ++attempt) {  // runs while any estimator still needs a redraw
            const int np = pm_dots(need, j, j + 1);
            std::vector<int> again;
            for (size_t a = 0; a < need.size(); ++a) {
              bool par = false;
              for (int q = 0; q < j; ++q) par |= std::llabs(D[a * np + q]) == nn;
              if (have_old)
                for (int q = 0; q < t; ++q) par |= std::llabs(D[a * np + t + q]) == nn;
              if (par && attempt <= 32) again.push_back(need[a]);
            }
            if (!again.empty()) {
              set_act(again);
              hipLaunchKernelGGL(est_resample_kernel, dim3(gn, (unsigned)again.size()), dim3(256), 0, s, (double*)w.S, n, t, j, (const int2*)w.act,
                                 col_key(seed, j, k * 64 + attempt));
            }
            need.swap(again);
          }
        }
      }
    }
    // 6. Z = B^H S, h_i = max_j |Z[i, j]|, for every active estimator with one application
    na = (int)A.size();
    for (int a = 0; a < na; ++a) {
      E[(size_t)A[(size_t)a]].ys = a;
      hll[(size_t)a] = E[(size_t)A[(size_t)a]].ind_best;
    }
    set_act(A);
    io.upload(w.ibest, hll.data(), sizeof(long long) * (size_t)na);
    hipLaunchKernelGGL(est_gather_kernel<T>, dim3(gn, na), dim3(256), 0, s, (const T*)w.S, w.Z, n, t, (const int2*)w.act, v, da.conj ? 1 : 0);
    solve(da.trans, w.Z, (int64_t)na * t);
    if (da.conj) hipLaunchKernelGGL(est_post_kernel<T>, dim3(gn, na), dim3(256), 0, s, w.Z, n, t, (const int2*)w.act, (const double*)nullptr, 1);
    hipLaunchKernelGGL((est_rowmax_top_kernel<T, MAXT>), dim3(nblk, na), dim3(256), 0, s, (const T*)w.Z, n, t, (const int2*)w.act, (const long long*)w.hist,
                       (const int*)w.hcnt, w.cand_h, w.cand_i, w.bmax);
    hipLaunchKernelGGL((est_select_final_kernel<T, MAXT>), dim3(na), dim3(256), 0, s, (const T*)w.Z, n, t, (const int2*)w.act, (const long long*)w.hist,
                       (const int*)w.hcnt, (const double*)w.cand_h, (const long long*)w.cand_i, (const double*)w.bmax, nblk, (const long long*)w.ibest, w.res);
    io.read(w.res, (size_t)Dim::RES * na);
    L.clear();
    for (int a = 0; a < na; ++a) {
      Est& q = E[(size_t)A[(size_t)a]];
      const double* r = io.hd.data() + (size_t)Dim::RES * a;
      if (k >= 2 && r[2] == r[3]) continue;
      // 7. the next unit vectors: the t largest h_i outside the history
      if (t > 1 && r[4] != 0.0) continue;
      if ((int)r[5] < t) continue;  // fewer than t rows left outside the history
      for (int j = 0; j < t; ++j) {
        q.ind[j] = (long long)r[8 + j];
        hll[L.size() * (size_t)t + j] = q.ind[j];
      }
      L.push_back(A[(size_t)a]);
    }
    A.swap(L);
    if (A.empty()) break;
    na = (int)A.size();
    set_act(A);
    io.upload(w.sel, hll.data(), sizeof(long long) * (size_t)na * t);
    hipLaunchKernelGGL((est_unit_kernel<T, MAXT>), dim3(gn, na), dim3(256), 0, s, w.X, n, t, (const int2*)w.act, (const long long*)w.sel, w.hist, w.hcnt);
  }
  for (int c = 0; c < ne; ++c) est[c] = E[(size_t)c].est;
}

}  // namespace
}  // namespace hs_ce
