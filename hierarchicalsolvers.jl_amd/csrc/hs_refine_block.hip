// hs_refine_block.hip -- refined solves with error bounds for a block of right-hand sides in lockstep (hs_ldiv_refine_block_*,
// include/hs_solver.h).
//
// Column c gets the xGERFS iteration hs_ldiv_refine_* (hs_condest.hip) runs for B[:, c] alone -- the same start, residual, weights, guarded
// ratio, continuation rule and forward error bound -- but every application of op(F)^-1 is ONE hs_ldiv_block_dev_t_* call on all columns that
// are still active, so the factors are read once per chunk of columns and not once per column.
//
// Refinement: a correction is a gather of the residuals of the columns that go on into the leading slots of the correction block, one block
// solve, one axpy through the slot -> column map, one fused residual pass over op(A) for all active columns and one host synchronisation that
// reads nact ratios.  A column whose test ends is frozen: its x, berr and steps are no longer written.  X and B are never repacked.
//
// Forward error bound: after the refinement every column runs its own Higham-Tisseur Algorithm 2.4 (normest1 of hs_condest.hip,
// tests/normest_mirror.py) on diag(v) op(F)^-H with its own estimate, index history (device resident), best index and done flag; the active
// estimators advance together, t = min(2, n) columns each, and share one block application of op_fwd(F)^-1 and one of op_adj(F)^-1 per
// iteration.  The estimator's X, S and S_old live at the column's place in the group; Y and Z, which travel through the block solve, are
// gathered into the leading slots, so finished estimators cost nothing.  The host reads the scalars of all columns with one synchronisation
// per half-step and checks the dataflow flag after each.
//
// Determinism: no floating-point atomics; every reduction is per (workgroup, column) partials and one ordered final pass per column, so a
// column's results depend on neither its slot, the other columns, the group width nor compaction.  The +-1 columns use the keys of
// hs_condest.hip, col_key(seed, j, salt): they do not depend on the right-hand side.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <vector>

#include "../../include/hs_solver.h"
#include "hs_common.h"
#define HS_CONDEST_KERNELS
#include "hs_condest.h"  // switches fma contraction off for the rest of this file
#include "hs_solve_multi.h"

#define RB_T 2                          // estimator columns per right-hand side: t = min(2, n)
#define RB_ITMAX 5                      // estimator iterations
#define RB_HIST (RB_T * (RB_ITMAX + 1)) // index history of one estimator
#define RB_RES (8 + RB_T)               // doubles of one estimator's selection result

using namespace hs_ce;

namespace {

// ---- the fused block residual -----------------------------------------------------------------------------------------------------------
// For the nc active slots: R[:, s] = B[:, col[s]] - op(A) X[:, col[s]], W[:, s] = |B[:, col[s]]| + |op(A)| |X[:, col[s]]| (cabs1), with V:
// V[:, vcol[s]] = |r| + nz eps w (+ safe1 where w is tiny), and part[s * gridDim.x + blockIdx.x] = the workgroup's max of the guarded ratio.
// Row i of op(A) is row i of the CSR map (op = N) or column i of the CSC arrays (op = T, H: CJ conjugates on load).  A workgroup owns 256
// rows, lanes along rows, and walks the slots CB at a time: ptr / idx / val of the row tile are read once per CB columns; B, R, W, V are read
// and written contiguously per column; the gathers of x through idx are the uncoalesced part.  Per (row, column) the sum runs over the stored
// entries in order, without contraction: given the same x these are the bits of resid_kernel (hs_condest.hip).  One summation order serves
// every row length.
template <class T, bool CJ, int CB>
__global__ __launch_bounds__(256) void resid_block_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val,
                                                          const T* __restrict__ X, int64_t ldx, const T* __restrict__ B, int64_t ldb,
                                                          const int64_t* __restrict__ col, T* __restrict__ R, double* __restrict__ W, int64_t ldr,
                                                          double* __restrict__ V, const int* __restrict__ vcol, double* __restrict__ part, int64_t n,
                                                          int nc, ResidArgs g, double nzeps) {
  __shared__ double sh[CB][256];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const bool live = i < n;
  int64_t e0 = 0, e1 = 0;
  if (live) {
    e0 = ptr[i];
    e1 = ptr[i + 1];
  }
  for (int c0 = 0; c0 < nc; c0 += CB) {
    T acc[CB];
    double wa[CB];
    const T* xp[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const int cc = min(c0 + c, nc - 1);  // a ragged chunk recomputes its last column and does not store it
      xp[c] = X + (size_t)col[cc] * ldx;
      acc[c] = Scal<T>::zero();
      wa[c] = 0.0;
    }
    for (int64_t e = e0; e < e1; ++e) {
      const T a = cj_<CJ>(val[e]);
      const int32_t j = idx[e];
      const double aa = abs1_(a);
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const T xv = xp[c][j];
        acc[c] = add_(acc[c], mul_(a, xv));
        wa[c] += aa * abs1_(xv);
      }
    }
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const int cc = c0 + c;
      double ratio = 0.0;
      if (live && cc < nc) {
        const T bi = B[(size_t)col[cc] * ldb + i];
        const T ri = sub_(bi, acc[c]);
        const double wi = wa[c] + abs1_(bi);
        R[(size_t)cc * ldr + i] = ri;
        W[(size_t)cc * ldr + i] = wi;
        const double ra = abs1_(ri);
        ratio = berr_ratio(ra, wi, g);
        if (V) V[(size_t)vcol[cc] * ldr + i] = wi > g.safe2 ? ra + nzeps * wi : ra + nzeps * wi + g.safe1;
      }
      sh[c][tid] = ratio;
    }
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st) {
#pragma unroll
        for (int c = 0; c < CB; ++c) sh[c][tid] = fmax(sh[c][tid], sh[c][tid + st]);
      }
      __syncthreads();
    }
    if (tid < CB && c0 + tid < nc) part[(size_t)(c0 + tid) * gridDim.x + blockIdx.x] = sh[tid][0];
    __syncthreads();
  }
}
// out[c] = max of part[c * cnt .. (c + 1) * cnt)   (one workgroup per column, fixed order)
__global__ __launch_bounds__(256) void colmax_final_kernel(const double* __restrict__ part, int64_t cnt, double* __restrict__ out) {
  __shared__ double sh[256];
  const double* p = part + (size_t)blockIdx.x * cnt;
  double m = 0.0;
  for (int64_t b = threadIdx.x; b < cnt; b += 256) m = fmax(m, p[b]);
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}
// D[:, s] = R[:, src[s]]: the residuals of the columns that go on, compacted into the leading slots of the correction block
template <class T>
__global__ __launch_bounds__(256) void gather_kernel(const T* __restrict__ R, T* __restrict__ D, int64_t ld, const int* __restrict__ src, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) D[(size_t)blockIdx.y * ld + i] = R[(size_t)src[blockIdx.y] * ld + i];
}
// X[:, col[s]] += D[:, s]
template <class T>
__global__ __launch_bounds__(256) void axpy_map_kernel(T* __restrict__ X, int64_t ldx, const int64_t* __restrict__ col, const T* __restrict__ D, int64_t ld, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  T* x = X + (size_t)col[blockIdx.y] * ldx;
  x[i] = add_(x[i], D[(size_t)blockIdx.y * ld + i]);
}
// part[c * gridDim.x + b] = max over the workgroup's rows of cabs1(X[i, c])   (grid: nblk x columns)
template <class T>
__global__ __launch_bounds__(256) void absmax_cols_kernel(const T* __restrict__ X, int64_t ldx, int64_t n, double* __restrict__ part) {
  __shared__ double sh[256];
  const T* x = X + (size_t)blockIdx.y * ldx;
  double m = 0.0;
  for (int q = 0; q < CE_ROWS / 256; ++q) {
    const int64_t i = (int64_t)blockIdx.x * CE_ROWS + q * 256 + threadIdx.x;
    if (i < n) m = fmax(m, abs1_(x[i]));
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}

// ---- the batched estimator kernels --------------------------------------------------------------------------------------------------------
// An active estimator is one entry of the device list `act`: x = its column within the group (where its X, S, S_old, v and history live),
// y = its slot in Y / Z (the blocks that travel through the block solve).  The list holds the active estimators only: frozen ones are
// skipped because they are not in it.  The estimator of list entry a is blockIdx.y (or blockIdx.y / columns).
struct Keys2 {
  uint64_t k[RB_T];
};
// X[:, (c, 0)] = 1/n, X[:, (c, j)] = +-1/n for every column c of the group   (grid: nb256 x gc)
template <class T>
__global__ __launch_bounds__(256) void est_init_kernel(T* __restrict__ X, int64_t n, int t, Keys2 keys, double inv_n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  T* x = X + (size_t)blockIdx.y * t * n;
  x[i] = from_real<T>(inv_n);
  for (int j = 1; j < t; ++j) x[(size_t)j * n + i] = from_real<T>(pm1(keys.k[j], i) * inv_n);
}
// Dst[:, (a, j)] = op(Src[:, (act[a].x, j)]) (* v[:, act[a].x]), op = conj with cj: the input of a block application, compacted   (grid: nb256 x nact)
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
// Y[:, (a, j)] = op(Y[:, (a, j)]) * v[:, act[a].x]: the output of a block application   (grid: nb256 x nact)
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
__global__ __launch_bounds__(256) void est_colnorm_final_kernel(const double* __restrict__ part, int nblk, int t, double* __restrict__ res) {
  __shared__ double sh[256];
  __shared__ double nrm[RB_T];
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
// S[:, (act[a].x, j)] = sign(Y[:, (act[a].y, j)])   (grid: nb256 x nact)
template <class T>
__global__ __launch_bounds__(256) void est_sign_kernel(const T* __restrict__ Y, T* __restrict__ S, int64_t n, int t, const int2* __restrict__ act) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int2 a = act[blockIdx.y];
  for (int j = 0; j < t; ++j) S[((size_t)a.x * t + j) * n + i] = sign_(Y[((size_t)a.y * t + j) * n + i]);
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
#define RB_NONE_I 0x7fffffffffffffffll
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
__device__ inline void list_merge(double (*sh)[RB_T], long long (*si)[RB_T], int a, int b, int t) {
  double oh[RB_T];
  long long oi[RB_T];
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
template <class T>
__device__ inline double rowmax_(const T* __restrict__ Z, int64_t n, int t, int64_t i) {  // h_i = max_j |Z[i, j]|
  double hv = 0.0;
  for (int j = 0; j < t; ++j) hv = fmax(hv, abs_(Z[(size_t)j * n + i]));
  return hv;
}
// per (workgroup, estimator): the best t rows of h outside the estimator's history, and the max of h   (grid: nblk x nact; Z in slot a)
template <class T>
__global__ __launch_bounds__(256) void est_rowmax_top_kernel(const T* __restrict__ Z, int64_t n, int t, const int2* __restrict__ act,
                                                             const long long* __restrict__ hist, const int* __restrict__ hcnt, double* __restrict__ cand_h,
                                                             long long* __restrict__ cand_i, double* __restrict__ bmax) {
  __shared__ double sh[256][RB_T];
  __shared__ long long si[256][RB_T];
  __shared__ double smax[256];
  __shared__ long long hs[RB_HIST];
  const int a = blockIdx.y, e = act[a].x;
  const int hc = hcnt[e];
  if ((int)threadIdx.x < hc) hs[threadIdx.x] = hist[(size_t)e * RB_HIST + threadIdx.x];
  __syncthreads();
  const T* Za = Z + (size_t)a * t * n;
  double lh[RB_T];
  long long li[RB_T];
  for (int k = 0; k < RB_T; ++k) {
    lh[k] = -1.0;
    li[k] = RB_NONE_I;
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
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      list_merge(sh, si, threadIdx.x, threadIdx.x + st, t);
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + st]);
    }
    __syncthreads();
  }
  const size_t o = (size_t)a * gridDim.x + blockIdx.x;
  if ((int)threadIdx.x < t) {
    cand_h[o * RB_T + threadIdx.x] = sh[0][threadIdx.x];
    cand_i[o * RB_T + threadIdx.x] = si[0][threadIdx.x];
  }
  if (threadIdx.x == 0) bmax[o] = smax[0];
}
// one workgroup per estimator, r = res + a RB_RES: r[2] = max h, r[3] = h[ind_best] (-1 when none), r[4] = 1 if the top t rows are all in the
// history, r[5] = rows selected, r[8 + j] = the j-th row outside the history
template <class T>
__global__ __launch_bounds__(256) void est_select_final_kernel(const T* __restrict__ Z, int64_t n, int t, const int2* __restrict__ act,
                                                               const long long* __restrict__ hist, const int* __restrict__ hcnt,
                                                               const double* __restrict__ cand_h, const long long* __restrict__ cand_i,
                                                               const double* __restrict__ bmax, int nblk, const long long* __restrict__ ind_best,
                                                               double* __restrict__ res) {
  __shared__ double sh[256][RB_T];
  __shared__ long long si[256][RB_T];
  __shared__ double smax[256];
  const int a = blockIdx.x, e = act[a].x;
  const T* Za = Z + (size_t)a * t * n;
  double lh[RB_T];
  long long li[RB_T];
  for (int k = 0; k < RB_T; ++k) {
    lh[k] = -1.0;
    li[k] = RB_NONE_I;
  }
  double m = -1.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    const size_t o = (size_t)a * nblk + b;
    for (int k = 0; k < t; ++k) list_insert(lh, li, t, cand_h[o * RB_T + k], cand_i[o * RB_T + k]);
    m = fmax(m, bmax[o]);
  }
  for (int k = 0; k < t; ++k) {
    sh[threadIdx.x][k] = lh[k];
    si[threadIdx.x][k] = li[k];
  }
  smax[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      list_merge(sh, si, threadIdx.x, threadIdx.x + st, t);
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + st]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* r = res + (size_t)a * RB_RES;
    int nsel = 0;
    for (int k = 0; k < t; ++k) {
      if (si[0][k] == RB_NONE_I) break;
      r[8 + k] = (double)si[0][k];
      ++nsel;
    }
    int above = 0;  // history rows that rank before the best row outside it
    const int hc = hcnt[e];
    for (int k = 0; k < hc; ++k) {
      const long long i = hist[(size_t)e * RB_HIST + k];
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
template <class T>
__global__ __launch_bounds__(256) void est_unit_kernel(T* __restrict__ X, int64_t n, int t, const int2* __restrict__ act, const long long* __restrict__ sel,
                                                       long long* __restrict__ hist, int* __restrict__ hcnt) {
  const int a = blockIdx.y, e = act[a].x;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int hc = hcnt[e];
    for (int j = 0; j < t; ++j) hist[(size_t)e * RB_HIST + hc + j] = sel[(size_t)a * t + j];
    hcnt[e] = hc + t;
  }
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (int j = 0; j < t; ++j) X[((size_t)e * t + j) * n + i] = from_real<T>(i == sel[(size_t)a * t + j] ? 1.0 : 0.0);
}

// ---- the driver ------------------------------------------------------------------------------------------------------------------------
enum { RI_SECONDS = 0, RI_SOLVES, RI_COL_APPS, RI_RESID, RI_MAX_ACTIVE, RI_GROUPS, RI_WORK_BYTES, RI_EST_COL_APPS };
thread_local double g_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};

template <class T>
struct Work {
  int64_t n = 0, G = 0;
  int t = 0, nwg = 0, nblk = 0;
  T *R = nullptr, *D = nullptr;
  double *W = nullptr, *V = nullptr, *part = nullptr, *ratio = nullptr;
  int64_t* col = nullptr;
  int *src = nullptr, *vcol = nullptr;
  // the estimators (ferr)
  T *EX = nullptr, *EY = nullptr, *ES = nullptr, *ESo = nullptr, *EZ = nullptr;
  double *epart = nullptr, *cand_h = nullptr, *bmax = nullptr, *res = nullptr;
  long long *cand_i = nullptr, *hist = nullptr, *ibest = nullptr, *sel = nullptr;
  unsigned long long* dots = nullptr;
  int* hcnt = nullptr;
  int2* act = nullptr;
};
template <class T>
size_t bytes_per_column(int64_t n, bool ferr) {
  const size_t t = (size_t)std::min<int64_t>(RB_T, n), nwg = (size_t)nb256(n), nblk = (size_t)nbrows(n);
  size_t b = (size_t)n * (2 * sizeof(T) + 2 * sizeof(double)) + (nwg + 1) * sizeof(double) + sizeof(int64_t) + 2 * sizeof(int);
  if (ferr)
    b += 5 * t * (size_t)n * sizeof(T) + nblk * (t * sizeof(double) + RB_T * (sizeof(double) + sizeof(long long)) + sizeof(double)) + RB_RES * sizeof(double) +
         (RB_HIST + 1 + RB_T) * sizeof(long long) + 2 * RB_T * RB_T * sizeof(unsigned long long) + sizeof(int) + sizeof(int2);
  return b;
}

template <class T>
struct Driver {
  hs_handle* F;
  HsHandleView v;
  hipStream_t s;
  int trans;
  Work<T> ws;
  const int64_t* ptr;
  const int32_t* idx;
  const T* val;
  bool cj;  // conjugate op(A)'s entries on load
  double nz;
  ResidArgs g;
  std::vector<double> hd;                 // what the host reads
  std::deque<std::vector<char>> pending;  // host sides of uploads in flight: released after the next synchronisation

  void upload(void* dst, const void* src, size_t bytes) {
    if (!bytes) return;
    pending.emplace_back((const char*)src, (const char*)src + bytes);
    CE_HIP(hipMemcpyAsync(dst, pending.back().data(), bytes, hipMemcpyHostToDevice, s));
  }
  // the one host <-> device synchronisation of a half-step
  void read(const void* d, size_t cnt) {
    if (hd.size() < cnt) hd.resize(cnt);
    CE_HIP(hipMemcpyAsync(hd.data(), d, sizeof(double) * cnt, hipMemcpyDeviceToHost, s));
    CE_HIP(hipStreamSynchronize(s));
    pending.clear();
    CE_CHECK(hs_handle_flow_check(F));
  }
  // op(F)^-1 by code (hs_condest.hip): 0 = F^-1, 1 = F^-T, 2 = F^-H, 3 = conj(F)^-1 = conj(F^-1 conj(.)); returns the trans of the block solve
  // and whether the block is conjugated before and after it
  static int dir_of(int code, bool* conj) {
    if (sizeof(T) == 8) code = (code == 2) ? 1 : (code == 3 ? 0 : code);
    *conj = code == 3;
    return code == 3 ? 0 : code;
  }
  void bsolve(int tr, T* X, int64_t ld, int64_t nc) {
    if (sizeof(T) == 16)
      CE_CHECK(hs_ldiv_block_dev_t_z(F, tr, (double*)X, ld, (const double*)X, ld, v.n, nc, (void*)s));
    else
      CE_CHECK(hs_ldiv_block_dev_t_d(F, tr, (double*)X, ld, (const double*)X, ld, v.n, nc, (void*)s));
    g_info[RI_SOLVES] += 1;
    g_info[RI_COL_APPS] += (double)nc;
  }
  void residual(const T* X, int64_t ldx, const T* B, int64_t ldb, int nact, bool weights) {
    constexpr int CB = sizeof(T) == 16 ? 4 : 8;
    auto k = cj ? resid_block_kernel<T, true, CB> : resid_block_kernel<T, false, CB>;
    hipLaunchKernelGGL(k, dim3((unsigned)ws.nwg), dim3(256), 0, s, ptr, idx, val, X, ldx, B, ldb, (const int64_t*)ws.col, ws.R, ws.W, ws.n,
                       weights ? ws.V : (double*)nullptr, (const int*)ws.vcol, ws.part, ws.n, nact, g, nz * CE_EPS);
    hipLaunchKernelGGL(colmax_final_kernel, dim3(nact), dim3(256), 0, s, (const double*)ws.part, (int64_t)ws.nwg, ws.ratio);
    g_info[RI_RESID] += 1;
  }

  // the columns g0 .. g0 + gc of the caller's block from start to finish
  void group(T* X, int64_t ldx, const T* B, int64_t ldb, int64_t g0, int gc, int64_t itmax, double* berr, double* ferr, int64_t* steps) {
    const int64_t n = ws.n;
    const unsigned gn = nb256(n);
    struct Col {
      int id;  // column within the group
      double lst = 3.0;
      int64_t cnt = 0;
    };
    std::vector<Col> cur((size_t)gc);
    std::vector<int64_t> hcol((size_t)gc);
    std::vector<int> hsrc((size_t)gc), hv((size_t)gc);
    for (int c = 0; c < gc; ++c) {
      cur[(size_t)c].id = c;
      hcol[(size_t)c] = g0 + c;
      hv[(size_t)c] = c;
    }
    upload(ws.col, hcol.data(), sizeof(int64_t) * (size_t)gc);
    upload(ws.vcol, hv.data(), sizeof(int) * (size_t)gc);
    // x = op(F) \ b
    CE_HIP(hipMemcpy2DAsync(X + (size_t)g0 * ldx, sizeof(T) * (size_t)ldx, B + (size_t)g0 * ldb, sizeof(T) * (size_t)ldb, sizeof(T) * (size_t)n, (size_t)gc,
                            hipMemcpyDeviceToDevice, s));
    bsolve(trans, X + (size_t)g0 * ldx, ldx, gc);
    for (;;) {
      const int nact = (int)cur.size();
      g_info[RI_MAX_ACTIVE] = std::max(g_info[RI_MAX_ACTIVE], (double)nact);
      residual(X, ldx, B, ldb, nact, ferr != nullptr);
      read(ws.ratio, (size_t)nact);
      std::vector<Col> next;
      for (int c = 0; c < nact; ++c) {
        Col q = cur[(size_t)c];
        const double be = hd[(size_t)c];
        if (be > CE_EPS && 2.0 * be <= q.lst && q.cnt < itmax) {
          q.lst = be;
          ++q.cnt;
          hsrc[next.size()] = c;
          hcol[next.size()] = g0 + q.id;
          hv[next.size()] = q.id;
          next.push_back(q);
        } else {  // frozen: its x, berr and steps are final
          berr[g0 + q.id] = be;
          steps[g0 + q.id] = q.cnt;
        }
      }
      if (next.empty()) break;
      const int nn = (int)next.size();
      upload(ws.src, hsrc.data(), sizeof(int) * (size_t)nn);
      upload(ws.col, hcol.data(), sizeof(int64_t) * (size_t)nn);
      upload(ws.vcol, hv.data(), sizeof(int) * (size_t)nn);
      // d = op(F) \ r for the columns that go on, in the leading slots; x += d
      hipLaunchKernelGGL(gather_kernel<T>, dim3(gn, nn), dim3(256), 0, s, (const T*)ws.R, ws.D, n, (const int*)ws.src, n);
      bsolve(trans, ws.D, n, nn);
      hipLaunchKernelGGL(axpy_map_kernel<T>, dim3(gn, nn), dim3(256), 0, s, X, ldx, (const int64_t*)ws.col, (const T*)ws.D, n, n);
      cur.swap(next);
    }
    if (ferr) estimate(X, ldx, g0, gc, ferr);
  }

  // ferr of the group's columns: || |op(A)^-1| v ||_Inf = || diag(v) op(A)^-H ||_1, estimated on B = diag(v) op(F)^-H, B^H = op(F)^-1 diag(v)
  // (normest1 of hs_condest.hip with t = min(2, n), 5 iterations, per column), then / ||x||_Inf
  void estimate(const T* X, int64_t ldx, int64_t g0, int gc, double* ferr) {
    const int64_t n = ws.n;
    const int t = ws.t, nblk = ws.nblk;
    const unsigned gn = nb256(n);
    const bool real = sizeof(T) == 8;
    const long long nn = (long long)n;
    bool cjf = false, cja = false;
    const int trf = dir_of(trans == 0 ? 2 : trans == 1 ? 3 : 0, &cjf);  // adj(trans)
    const int tra = dir_of(trans, &cja);
    struct Est {
      int id, ys = 0;
      double est = 0.0, est_old = 0.0;
      long long ind[RB_T] = {0, 0};
      long long ind_best = -1;
    };
    std::vector<Est> E((size_t)gc);
    std::vector<int> A((size_t)gc);  // the active estimators
    for (int c = 0; c < gc; ++c) {
      E[(size_t)c].id = c;
      A[(size_t)c] = c;
    }
    std::vector<int2> hact((size_t)gc);
    std::vector<long long> hll((size_t)gc * RB_T);
    std::vector<long long> D;
    auto set_act = [&](const std::vector<int>& L) {
      for (size_t a = 0; a < L.size(); ++a) hact[a] = make_int2(E[(size_t)L[a]].id, E[(size_t)L[a]].ys);
      upload(ws.act, hact.data(), sizeof(int2) * L.size());
    };
    // exact +-1 dot products of the sign columns j0 .. j1-1 with [S  S_old] for the estimators of L: D[a np + (j - j0) 2t + q]
    auto pm_dots = [&](const std::vector<int>& L, int j0, int j1) {
      const int np = (j1 - j0) * 2 * t;
      const size_t cnt = L.size() * (size_t)np;
      set_act(L);
      CE_HIP(hipMemsetAsync(ws.dots, 0, sizeof(unsigned long long) * cnt, s));
      hipLaunchKernelGGL(est_pm_dots_kernel, dim3(nblk, (unsigned)cnt), dim3(256), 0, s, (const double*)ws.ES, (const double*)ws.ESo, n, t, j0, np,
                         (const int2*)ws.act, ws.dots);
      read(ws.dots, cnt);
      D.resize(cnt);
      std::memcpy(D.data(), hd.data(), sizeof(long long) * cnt);
      return np;
    };
    // 1. start
    Keys2 keys{};
    for (int j = 0; j < t; ++j) keys.k[j] = col_key(v.seed, j, 0);
    hipLaunchKernelGGL(est_init_kernel<T>, dim3(gn, gc), dim3(256), 0, s, ws.EX, n, t, keys, 1.0 / (double)n);
    CE_HIP(hipMemsetAsync(ws.hcnt, 0, sizeof(int) * (size_t)gc, s));
    for (int k = 1; !A.empty(); ++k) {
      // 2. Y = B X, est = max_j ||Y[:, j]||_1, for every active estimator with one block application
      int na = (int)A.size();
      set_act(A);
      hipLaunchKernelGGL(est_gather_kernel<T>, dim3(gn, na), dim3(256), 0, s, (const T*)ws.EX, ws.EY, n, t, (const int2*)ws.act, (const double*)nullptr, cjf ? 1 : 0);
      bsolve(trf, ws.EY, n, (int64_t)na * t);
      g_info[RI_EST_COL_APPS] += (double)na * t;
      hipLaunchKernelGGL(est_post_kernel<T>, dim3(gn, na), dim3(256), 0, s, ws.EY, n, t, (const int2*)ws.act, (const double*)ws.V, cjf ? 1 : 0);
      hipLaunchKernelGGL(est_colnorm_part_kernel<T>, dim3(nblk, na * t), dim3(256), 0, s, (const T*)ws.EY, n, ws.epart);
      hipLaunchKernelGGL(est_colnorm_final_kernel, dim3(na), dim3(256), 0, s, (const double*)ws.epart, nblk, t, ws.res);
      read(ws.res, (size_t)2 * na);
      std::vector<int> L;
      for (int a = 0; a < na; ++a) {
        Est& q = E[(size_t)A[(size_t)a]];
        q.ys = a;
        q.est = hd[(size_t)2 * a];
        const int jmax = (int)hd[(size_t)2 * a + 1];
        if ((q.est > q.est_old || k == 2) && k >= 2) q.ind_best = q.ind[jmax];
        if (k >= 2 && q.est <= q.est_old) {
          q.est = q.est_old;
          continue;
        }
        // 3. iteration limit
        q.est_old = q.est;
        if (k > RB_ITMAX) continue;
        L.push_back(A[(size_t)a]);
      }
      A.swap(L);
      if (A.empty()) break;
      std::swap(ws.ES, ws.ESo);  // S_old = S (every active estimator is at iteration k)
      const bool have_old = k >= 2;
      // 4. signs
      na = (int)A.size();
      set_act(A);
      hipLaunchKernelGGL(est_sign_kernel<T>, dim3(gn, na), dim3(256), 0, s, (const T*)ws.EY, ws.ES, n, t, (const int2*)ws.act);
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
                hipLaunchKernelGGL(est_resample_kernel, dim3(gn, (unsigned)again.size()), dim3(256), 0, s, (double*)ws.ES, n, t, j, (const int2*)ws.act,
                                   col_key(v.seed, j, k * 64 + attempt));
              }
              need.swap(again);
            }
          }
        }
      }
      // 6. Z = B^H S, h_i = max_j |Z[i, j]|, for every active estimator with one block application
      na = (int)A.size();
      for (int a = 0; a < na; ++a) {
        E[(size_t)A[(size_t)a]].ys = a;
        hll[(size_t)a] = E[(size_t)A[(size_t)a]].ind_best;
      }
      set_act(A);
      upload(ws.ibest, hll.data(), sizeof(long long) * (size_t)na);
      hipLaunchKernelGGL(est_gather_kernel<T>, dim3(gn, na), dim3(256), 0, s, (const T*)ws.ES, ws.EZ, n, t, (const int2*)ws.act, (const double*)ws.V, cja ? 1 : 0);
      bsolve(tra, ws.EZ, n, (int64_t)na * t);
      g_info[RI_EST_COL_APPS] += (double)na * t;
      if (cja) hipLaunchKernelGGL(est_post_kernel<T>, dim3(gn, na), dim3(256), 0, s, ws.EZ, n, t, (const int2*)ws.act, (const double*)nullptr, 1);
      hipLaunchKernelGGL(est_rowmax_top_kernel<T>, dim3(nblk, na), dim3(256), 0, s, (const T*)ws.EZ, n, t, (const int2*)ws.act, (const long long*)ws.hist,
                         (const int*)ws.hcnt, ws.cand_h, ws.cand_i, ws.bmax);
      hipLaunchKernelGGL(est_select_final_kernel<T>, dim3(na), dim3(256), 0, s, (const T*)ws.EZ, n, t, (const int2*)ws.act, (const long long*)ws.hist,
                         (const int*)ws.hcnt, (const double*)ws.cand_h, (const long long*)ws.cand_i, (const double*)ws.bmax, nblk, (const long long*)ws.ibest, ws.res);
      read(ws.res, (size_t)RB_RES * na);
      L.clear();
      for (int a = 0; a < na; ++a) {
        Est& q = E[(size_t)A[(size_t)a]];
        const double* r = hd.data() + (size_t)RB_RES * a;
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
      upload(ws.sel, hll.data(), sizeof(long long) * (size_t)na * t);
      hipLaunchKernelGGL(est_unit_kernel<T>, dim3(gn, na), dim3(256), 0, s, ws.EX, n, t, (const int2*)ws.act, (const long long*)ws.sel, ws.hist, ws.hcnt);
    }
    // ||x||_Inf of every column of the group
    hipLaunchKernelGGL(absmax_cols_kernel<T>, dim3(nblk, gc), dim3(256), 0, s, X + (size_t)g0 * ldx, ldx, n, ws.epart);
    hipLaunchKernelGGL(colmax_final_kernel, dim3(gc), dim3(256), 0, s, (const double*)ws.epart, (int64_t)nblk, ws.res);
    read(ws.res, (size_t)gc);
    for (int c = 0; c < gc; ++c) {
      const double xn = hd[(size_t)c], est = E[(size_t)c].est;
      ferr[g0 + c] = xn != 0.0 ? est / xn : est;
    }
  }
};

// G: the widest group (a multiple of the block solve's chunk width) whose workspace fits half of the free memory; HS_REFINE_BLOCK_GROUP overrides
int64_t group_width(size_t per_col, int64_t nrhs) {
  const int64_t KC = hs_ldiv_block_cols();
  const int64_t all = std::min<int64_t>((nrhs + KC - 1) / KC * KC, 4096);  // blockIdx.y carries up to 2 t^2 = 8 entries per column
  if (const char* e = getenv("HS_REFINE_BLOCK_GROUP")) {
    const long long w = atoll(e);
    if (w > 0) return std::min<int64_t>(all, (w + KC - 1) / KC * KC);
  }
  size_t fr = 0, tot = 0;
  CE_HIP(hipMemGetInfo(&fr, &tot));
  const int64_t fit = (int64_t)(fr / 2 / per_col);
  if (fit >= all) return all;
  const int64_t least = std::min<int64_t>(KC, nrhs);
  if (fit < least)
    CE_FAIL(HS_ERR_NOMEM, 0, "OutOfMemoryError: hs_ldiv_refine_block_* needs %zu bytes for one group of %lld columns, half of the free device memory is %zu bytes",
            per_col * (size_t)least, (long long)least, fr / 2);
  return std::max<int64_t>(fit / KC * KC, least);
}

template <class T>
void refine_block_dev(hs_handle* F, const HsHandleView& v, int trans, T* dX, int64_t ldx, const T* dB, int64_t ldb, int64_t nrhs, int64_t itmax, double* berr,
                      double* ferr, int64_t* steps, hipStream_t s, DevBuf& buf) {
  const int64_t n = v.n;
  Driver<T> d{F, v, s, trans};
  // rows of op(A): the CSR map (op = N) or the CSC arrays (op = T, H)
  int64_t maxlen;
  if (trans == 0) {
    CsrMap* m = csr_of<T>(v, s);
    d.ptr = m->rowptr;
    d.idx = m->colind;
    d.val = (const T*)m->valr;
    maxlen = m->maxrow;
  } else {
    d.ptr = v.colptr;
    d.idx = v.rowval;
    d.val = (const T*)v.nz;
    maxlen = max_col(v, s);
  }
  d.cj = trans == 2 && sizeof(T) == 16;
  d.nz = (double)(maxlen + 1);
  d.g = ResidArgs{d.nz * CE_SAFMIN, d.nz * CE_SAFMIN / CE_EPS};
  Work<T>& ws = d.ws;
  const size_t per_col = bytes_per_column<T>(n, ferr != nullptr);
  ws.n = n;
  ws.G = std::min<int64_t>(group_width(per_col, nrhs), nrhs);
  ws.t = (int)std::min<int64_t>(RB_T, n);
  ws.nwg = (int)nb256(n);
  ws.nblk = (int)nbrows(n);
  const size_t G = (size_t)ws.G, blk = G * (size_t)n, t = (size_t)ws.t;
  ws.R = buf.get<T>(blk);
  ws.D = buf.get<T>(blk);
  ws.W = buf.get<double>(blk);
  ws.V = buf.get<double>(blk);
  ws.part = buf.get<double>(G * ws.nwg);
  ws.ratio = buf.get<double>(G);
  ws.col = buf.get<int64_t>(G);
  ws.src = buf.get<int>(G);
  ws.vcol = buf.get<int>(G);
  if (ferr) {
    ws.EX = buf.get<T>(blk * t);
    ws.EY = buf.get<T>(blk * t);
    ws.ES = buf.get<T>(blk * t);
    ws.ESo = buf.get<T>(blk * t);
    ws.EZ = buf.get<T>(blk * t);
    ws.epart = buf.get<double>(G * ws.nblk * t);
    ws.cand_h = buf.get<double>(G * ws.nblk * RB_T);
    ws.cand_i = buf.get<long long>(G * ws.nblk * RB_T);
    ws.bmax = buf.get<double>(G * ws.nblk);
    ws.res = buf.get<double>(G * RB_RES);
    ws.hist = buf.get<long long>(G * RB_HIST);
    ws.ibest = buf.get<long long>(G);
    ws.sel = buf.get<long long>(G * RB_T);
    ws.dots = buf.get<unsigned long long>(G * 2 * RB_T * RB_T);
    ws.hcnt = buf.get<int>(G);
    ws.act = buf.get<int2>(G);
  }
  g_info[RI_WORK_BYTES] = (double)(per_col * G);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  try {
    CE_HIP(hipEventCreate(&e0));
    CE_HIP(hipEventCreate(&e1));
    CE_HIP(hipEventRecord(e0, s));
    for (int64_t g0 = 0; g0 < nrhs; g0 += ws.G) {
      d.group(dX, ldx, dB, ldb, g0, (int)std::min<int64_t>(ws.G, nrhs - g0), itmax, berr, ferr, steps);
      g_info[RI_GROUPS] += 1;
    }
    CE_HIP(hipEventRecord(e1, s));
    CE_HIP(hipEventSynchronize(e1));
    CE_CHECK(hs_handle_flow_check(F));
    float ms = 0.f;
    CE_HIP(hipEventElapsedTime(&ms, e0, e1));
    g_info[RI_SECONDS] = ms * 1e-3;
  } catch (...) {
    (void)hipStreamSynchronize(s);  // nothing in flight may outlive the workspace or the host sides of the uploads
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    throw;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
}

template <class T>
void refine_block_entry(hs_handle* F, int trans, T* X, int64_t ldx, const T* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax, double* berr, double* ferr,
                        int64_t* steps, bool on_device, void* stream) {
  const char* fn = on_device ? "hs_ldiv_refine_block_dev_*" : "hs_ldiv_refine_block_*";
  // refusals: before any device work, X untouched
  if (!F) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null factorization handle", fn);
  HsHandleView v;
  hs_handle_view(F, &v);
  if ((v.is_complex != 0) != (sizeof(T) == 16)) CE_FAIL(HS_ERR_ARGUMENT, 0, "MethodError: %s: eltype of F and B differ", fn);
  if (trans < 0 || trans > 2) CE_FAIL(HS_ERR_ARGUMENT, trans, "ArgumentError: %s: trans = %d (0: F, 1: transpose(F), 2: adjoint(F))", fn, trans);
  if (n != v.n || nrhs < 0 || ldx < n || ldb < n)
    CE_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: B has %lld rows (ldx %lld, ldb %lld, nrhs %lld), F is %lld x %lld", fn, (long long)n, (long long)ldx,
            (long long)ldb, (long long)nrhs, (long long)v.n, (long long)v.n);
  if (itmax < 0) CE_FAIL(HS_ERR_ARGUMENT, itmax, "ArgumentError: %s: itmax = %lld < 0", fn, (long long)itmax);
  if (nrhs > 0 && (!X || !B || !berr || !steps)) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: X, B, berr and steps must not be NULL", fn);
  if (nrhs > 0) {
    const T* xb = X;
    if (xb < B + (size_t)ldb * nrhs && B < xb + (size_t)ldx * nrhs) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: X may not alias B", fn);
  }
  // what hs_ldiv_block_t_* refuses, whatever trans and ferr are (a host-side plan names these too)
  if (v.nranks > 1)
    CE_FAIL(HS_ERR_UNSUPPORTED, v.nranks, "%s: a factorization over %d ranks is not supported (single-rank factorizations only)", fn, v.nranks);
  if (v.t_refused_node >= 0)
    CE_FAIL(HS_ERR_UNSUPPORTED, v.t_refused_node,
            "%s: node %d keeps its interior block D as an HSS matrix (hs_options.hss_d / mf = 2, 3): block solves and transposed ULV solves are not implemented; "
            "hs_ldiv_refine_* serves this handle with trans = 0 and without ferr",
            fn, v.t_refused_node);
  if (!v.device) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: handle holds a host-side plan only (hs_plan)", fn);
  if (!v.factored) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: factorization is not complete", fn);
  {  // whatever else the block solve refuses is refused here: nothing is silently looped
    const int st = sizeof(T) == 16 ? hs_ldiv_block_dev_t_z(F, trans, nullptr, n, nullptr, n, n, 0, nullptr) : hs_ldiv_block_dev_t_d(F, trans, nullptr, n, nullptr, n, n, 0, nullptr);
    if (st != HS_OK) {
      const std::string why = hs_last_error();
      hs_set_error(st, hs_last_error_info(), "%s: the block solve does not serve this handle (%s)", fn, why.c_str());
      throw st;
    }
  }
  for (double& x : g_info) x = 0.0;
  if (nrhs == 0) return;
  DevBuf buf;  // freed after the stream is drained, on every path
  if (on_device) return refine_block_dev<T>(F, v, trans, X, ldx, B, ldb, nrhs, itmax, berr, ferr, steps, (hipStream_t)stream, buf);
  hipStream_t s = v.stream;
  T* dX = buf.get<T>((size_t)n * nrhs);
  T* dB = buf.get<T>((size_t)n * nrhs);
  try {
    CE_HIP(hipMemcpy2DAsync(dB, sizeof(T) * n, B, sizeof(T) * ldb, sizeof(T) * n, nrhs, hipMemcpyHostToDevice, s));
    // results go to the caller's arrays only when the whole call succeeded
    std::vector<double> be((size_t)nrhs), fe((size_t)nrhs);
    std::vector<int64_t> st((size_t)nrhs);
    refine_block_dev<T>(F, v, trans, dX, n, dB, n, nrhs, itmax, be.data(), ferr ? fe.data() : nullptr, st.data(), s, buf);
    CE_HIP(hipMemcpy2DAsync(X, sizeof(T) * ldx, dX, sizeof(T) * n, sizeof(T) * n, nrhs, hipMemcpyDeviceToHost, s));
    CE_HIP(hipStreamSynchronize(s));
    std::copy(be.begin(), be.end(), berr);
    if (ferr) std::copy(fe.begin(), fe.end(), ferr);
    std::copy(st.begin(), st.end(), steps);
  } catch (...) {
    (void)hipStreamSynchronize(s);
    throw;
  }
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
extern "C" int hs_ldiv_refine_block_d(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                      double* berr, double* ferr, int64_t* steps) {
  CE_GUARD(refine_block_entry<double>(F, trans, X, ldx, B, ldb, n, nrhs, itmax, berr, ferr, steps, false, nullptr));
}
extern "C" int hs_ldiv_refine_block_z(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                      double* berr, double* ferr, int64_t* steps) {
  CE_GUARD(refine_block_entry<cplx>(F, trans, (cplx*)X, ldx, (const cplx*)B, ldb, n, nrhs, itmax, berr, ferr, steps, false, nullptr));
}
extern "C" int hs_ldiv_refine_block_dev_d(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                          double* berr, double* ferr, int64_t* steps, void* stream) {
  CE_GUARD(refine_block_entry<double>(F, trans, dX, ldx, dB, ldb, n, nrhs, itmax, berr, ferr, steps, true, stream));
}
extern "C" int hs_ldiv_refine_block_dev_z(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                          double* berr, double* ferr, int64_t* steps, void* stream) {
  CE_GUARD(refine_block_entry<cplx>(F, trans, (cplx*)dX, ldx, (const cplx*)dB, ldb, n, nrhs, itmax, berr, ferr, steps, true, stream));
}
extern "C" int hs_ldiv_refine_block_info(double* out8) {
  if (!out8) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_ldiv_refine_block_info: null argument");
    return HS_ERR_ARGUMENT;
  }
  for (int i = 0; i < 8; ++i) out8[i] = g_info[i];
  return HS_OK;
}
