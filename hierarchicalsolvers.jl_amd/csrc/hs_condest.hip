// hs_condest.hip -- the accuracy tools of a factorization behind the C ABI (include/hs_solver.h): ||A||_1 and ||A||_Inf of the handle's A,
// the Higham-Tisseur block 1-norm estimate of op(F)^-1 (Julia's opnormestinv, LAPACK xGECON), cond(A, p), and refined solves with the
// componentwise backward error berr and the forward error bound ferr of LAPACK xGERFS.
//
// One estimator engine (normest1 below; Higham & Tisseur, SIAM J. Matrix Anal. Appl. 21(4), 2000, Algorithm 2.4) serves both clients: it
// works on an operator B given by two solve callbacks, B X and B^H X, each a set of solves with the handle (hs_ldiv_dev_t_*) and optionally a
// diagonal scaling.  Every n-vector operation is a kernel here; the host reads a few scalars per iteration (like hs_gmres.hip) and checks the
// dataflow-sweep error flag after every synchronisation, so a timed-out sweep becomes an error and never an estimate.
//
// Determinism: the +-1 columns are the low bit of splitmix64 over (row, column, iteration, hs_options.seed) -- no RNG state; every floating-
// point reduction is per-workgroup partials in LDS and one ordered final pass; the only atomics are on integers (row counts, exact +-1 dot
// products).  Two calls on the same handle return the same bits.  tests/normest_mirror.py restates the engine in NumPy step for step.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/hs_solver.h"
#include "hs_common.h"
#define HS_CONDEST_KERNELS
#include "hs_condest.h"

// No contraction of a*b + c into an fma in this file: the residual r = b - op(A) x and the weights w are then the plain products and sums, row by
// row in column order, that scipy's CSR product computes -- a test can recompute berr from the returned X and compare (berr is ~eps, and the
// rounding of r is of the size of r itself).
#pragma clang fp contract(off)

#define CE_MAXT 8       // estimator columns
#define CE_MAXIT 16     // estimator iterations (the index history holds t * itmax entries)
#define CE_WAVE_ROW 64  // rows of op(A) longer than this are gathered by a whole wave (graphs from hs_symbolic_from_graph)

using namespace hs_ce;

namespace {

struct Keys {
  uint64_t k[CE_MAXT];
};
struct Hist {  // the estimator's index history, by value
  long long idx[CE_MAXT * CE_MAXIT];
  int cnt;
};
struct Sel {
  long long idx[CE_MAXT];
};

// ---- estimator kernels ---------------------------------------------------------------------------------------------------------
// X[:, 0] = 1/n, X[:, j] = +-1/n
template <class T>
__global__ __launch_bounds__(256) void init_x_kernel(T* __restrict__ X, int64_t n, int t, Keys keys, double inv_n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  X[i] = from_real<T>(inv_n);
  for (int j = 1; j < t; ++j) X[(size_t)j * n + i] = from_real<T>(pm1(keys.k[j], i) * inv_n);
}
// X[:, j] = e_{sel[j]}
template <class T>
__global__ __launch_bounds__(256) void unit_kernel(T* __restrict__ X, int64_t n, int t, Sel sel) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (int j = 0; j < t; ++j) X[(size_t)j * n + i] = from_real<T>(i == sel.idx[j] ? 1.0 : 0.0);
}
// part[j * nblk + b] = sum over the workgroup's rows of |Y[i, j]|   (grid: nblk x t)
template <class T>
__global__ __launch_bounds__(256) void colnorm_part_kernel(const T* __restrict__ Y, int64_t n, double* __restrict__ part) {
  __shared__ double sh[256];
  const int j = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * CE_ROWS;
  double acc = 0.0;
  for (int q = 0; q < CE_ROWS / 256; ++q) {
    const int64_t i = i0 + q * 256 + threadIdx.x;
    if (i < n) acc += abs_(Y[(size_t)j * n + i]);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)j * gridDim.x + blockIdx.x] = sh[0];
}
// res[0] = max_j ||Y[:, j]||_1, res[1] = the first j that attains it   (one workgroup)
__global__ __launch_bounds__(256) void est_final_kernel(const double* __restrict__ part, int nblk, int t, double* __restrict__ res) {
  __shared__ double sh[256];
  __shared__ double nrm[CE_MAXT];
  for (int j = 0; j < t; ++j) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) acc += part[(size_t)j * nblk + b];
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
    res[0] = est;
    res[1] = (double)jm;
  }
}
// S = sign(Y) (sign(0) = 1; complex: Y / |Y|)
template <class T>
__global__ __launch_bounds__(256) void sign_kernel(const T* __restrict__ Y, T* __restrict__ S, int64_t cnt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < cnt) S[i] = sign_(Y[i]);
}
__global__ __launch_bounds__(256) void resample_kernel(double* __restrict__ s, int64_t n, uint64_t key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) s[i] = pm1(key, i);
}
// out[p] += the workgroup's part of S[:, j] . O[:, q] for p = (j - j0) * 2t + q, O = [S  S_old]: exact integers (+-1 entries), summed with
// integer atomics -- the result does not depend on their order   (grid: nblk x (j1 - j0) * 2t)
__global__ __launch_bounds__(256) void pm_dots_kernel(const double* __restrict__ S, const double* __restrict__ So, int64_t n, int t, int j0,
                                                      unsigned long long* __restrict__ out) {
  __shared__ long long sh[256];
  const int p = blockIdx.y;
  const int j = j0 + p / (2 * t), q = p % (2 * t);
  const double* a = S + (size_t)j * n;
  const double* o = q < t ? S + (size_t)q * n : So + (size_t)(q - t) * n;
  const int64_t i0 = (int64_t)blockIdx.x * CE_ROWS;
  long long acc = 0;
  for (int k = 0; k < CE_ROWS / 256; ++k) {
    const int64_t i = i0 + k * 256 + threadIdx.x;
    if (i < n) acc += (a[i] == o[i]) ? 1 : -1;
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(out + p, (unsigned long long)sh[0]);
}

// top-t selection: order = h descending, ties by ascending index; the history is excluded
__device__ inline bool better(double ha, long long ia, double hb, long long ib) { return ha > hb || (ha == hb && ia < ib); }
__device__ inline bool in_hist(const Hist& hs, long long i) {
  for (int k = 0; k < hs.cnt; ++k)
    if (hs.idx[k] == i) return true;
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
__device__ inline void list_merge(double (*sh)[CE_MAXT], long long (*si)[CE_MAXT], int a, int b, int t) {
  double oh[CE_MAXT];
  long long oi[CE_MAXT];
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
#define CE_NONE_I 0x7fffffffffffffffll
// h[i] = max_j |Z[i, j]|; per workgroup: its best t rows outside the history and its max h   (grid: nblk)
template <class T>
__global__ __launch_bounds__(256) void rowmax_top_kernel(const T* __restrict__ Z, int64_t n, int t, double* __restrict__ h, Hist hs,
                                                         double* __restrict__ cand_h, long long* __restrict__ cand_i, double* __restrict__ bmax) {
  __shared__ double sh[256][CE_MAXT];
  __shared__ long long si[256][CE_MAXT];
  double lh[CE_MAXT];
  long long li[CE_MAXT];
  for (int k = 0; k < t; ++k) {
    lh[k] = -1.0;
    li[k] = CE_NONE_I;
  }
  double m = -1.0;
  const int64_t i0 = (int64_t)blockIdx.x * CE_ROWS;
  for (int q = 0; q < CE_ROWS / 256; ++q) {
    const int64_t i = i0 + q * 256 + threadIdx.x;
    if (i >= n) break;
    double hv = 0.0;
    for (int j = 0; j < t; ++j) hv = fmax(hv, abs_(Z[(size_t)j * n + i]));
    h[i] = hv;
    m = fmax(m, hv);
    if (better(hv, i, lh[t - 1], li[t - 1]) && !in_hist(hs, i)) list_insert(lh, li, t, hv, i);
  }
  for (int k = 0; k < t; ++k) {
    sh[threadIdx.x][k] = lh[k];
    si[threadIdx.x][k] = li[k];
  }
  __shared__ double smax[256];
  smax[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      list_merge(sh, si, threadIdx.x, threadIdx.x + st, t);
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + st]);
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < t) {
    cand_h[(size_t)blockIdx.x * CE_MAXT + threadIdx.x] = sh[0][threadIdx.x];
    cand_i[(size_t)blockIdx.x * CE_MAXT + threadIdx.x] = si[0][threadIdx.x];
  }
  if (threadIdx.x == 0) bmax[blockIdx.x] = smax[0];
}
// one workgroup: res[2] = max h, res[3] = h[ind_best] (-1 when none), res[4] = 1 if the top t rows are all in the history, res[5] = rows
// selected, res[8 + j] = the j-th row outside the history
__global__ __launch_bounds__(256) void select_final_kernel(const double* __restrict__ cand_h, const long long* __restrict__ cand_i,
                                                           const double* __restrict__ bmax, int nblk, int t, const double* __restrict__ h, Hist hs,
                                                           long long ind_best, double* __restrict__ res) {
  __shared__ double sh[256][CE_MAXT];
  __shared__ long long si[256][CE_MAXT];
  __shared__ double smax[256];
  for (int k = 0; k < t; ++k) {
    sh[threadIdx.x][k] = -1.0;
    si[threadIdx.x][k] = CE_NONE_I;
  }
  double m = -1.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    for (int k = 0; k < t; ++k) {
      double lh[CE_MAXT];
      long long li[CE_MAXT];
      for (int q = 0; q < t; ++q) {
        lh[q] = sh[threadIdx.x][q];
        li[q] = si[threadIdx.x][q];
      }
      list_insert(lh, li, t, cand_h[(size_t)b * CE_MAXT + k], cand_i[(size_t)b * CE_MAXT + k]);
      for (int q = 0; q < t; ++q) {
        sh[threadIdx.x][q] = lh[q];
        si[threadIdx.x][q] = li[q];
      }
    }
    m = fmax(m, bmax[b]);
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
    int nsel = 0;
    for (int k = 0; k < t; ++k) {
      if (si[0][k] == CE_NONE_I) break;
      res[8 + k] = (double)si[0][k];
      ++nsel;
    }
    int above = 0;  // history rows that rank before the best row outside it
    for (int k = 0; k < hs.cnt; ++k) {
      const long long i = hs.idx[k];
      if (nsel == 0 || better(h[i], i, sh[0][0], si[0][0])) ++above;
    }
    res[2] = smax[0];
    res[3] = ind_best >= 0 ? h[ind_best] : -1.0;
    res[4] = above >= t ? 1.0 : 0.0;
    res[5] = (double)nsel;
  }
}

template <class T>
__global__ __launch_bounds__(256) void conj_kernel(T* __restrict__ X, int64_t cnt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < cnt) X[i] = cj_<true>(X[i]);
}
// X[i, j] *= v[i]
template <class T>
__global__ __launch_bounds__(256) void scale_rows_kernel(T* __restrict__ X, const double* __restrict__ v, int64_t n, int t) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double s = v[i];
  for (int j = 0; j < t; ++j) X[(size_t)j * n + i] = scale_(X[(size_t)j * n + i], s);
}

// ---- residual, norms, CSR map ----------------------------------------------------------------------------------------------------
// Row i of op(A) is row i of the CSR map (op = N) or column i of the CSC arrays (op = T, H: CJ conjugates).  One pass reads A, x, b and
// writes r = b - op(A) x and w = |b| + |op(A)| |x| (cabs1), and the workgroup's max of the xGERFS ratio |r_i| / w_i (safe1 / safe2 guard).
template <class T, bool CJ>
__global__ __launch_bounds__(256) void resid_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val,
                                                    const T* __restrict__ x, const T* __restrict__ b, T* __restrict__ r, double* __restrict__ w,
                                                    double* __restrict__ part, int64_t n, ResidArgs g) {
  __shared__ double sh[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double ratio = 0.0;
  if (i < n) {
    T acc = Scal<T>::zero();
    double wa = 0.0;
    for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
      const T a = cj_<CJ>(val[e]);
      const T xv = x[idx[e]];
      acc = add_(acc, mul_(a, xv));
      wa += abs1_(a) * abs1_(xv);
    }
    const T bi = b[i];
    const T ri = sub_(bi, acc);
    wa += abs1_(bi);
    r[i] = ri;
    w[i] = wa;
    ratio = berr_ratio(abs1_(ri), wa, g);
  }
  sh[threadIdx.x] = ratio;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
// the same with one wave per row (rows longer than CE_WAVE_ROW entries): lanes stride the row, a fixed butterfly sums the lanes
template <class T>
__device__ inline T shfl_xor_(T v, int m);
template <>
__device__ inline double shfl_xor_<double>(double v, int m) { return __shfl_xor(v, m, 64); }
template <>
__device__ inline cplx shfl_xor_<cplx>(cplx v, int m) { return {__shfl_xor(v.re, m, 64), __shfl_xor(v.im, m, 64)}; }
template <class T, bool CJ>
__global__ __launch_bounds__(256) void resid_wave_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val,
                                                         const T* __restrict__ x, const T* __restrict__ b, T* __restrict__ r, double* __restrict__ w,
                                                         double* __restrict__ part, int64_t n, ResidArgs g) {
  __shared__ double sh[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + wv;
  double ratio = 0.0;
  if (i < n) {
    T acc = Scal<T>::zero();
    double wa = 0.0;
    for (int64_t e = ptr[i] + lane; e < ptr[i + 1]; e += 64) {
      const T a = cj_<CJ>(val[e]);
      const T xv = x[idx[e]];
      acc = add_(acc, mul_(a, xv));
      wa += abs1_(a) * abs1_(xv);
    }
    for (int m = 32; m > 0; m >>= 1) {
      acc = add_(acc, shfl_xor_<T>(acc, m));
      wa += __shfl_xor(wa, m, 64);
    }
    if (lane == 0) {
      const T bi = b[i];
      const T ri = sub_(bi, acc);
      wa += abs1_(bi);
      r[i] = ri;
      w[i] = wa;
      ratio = berr_ratio(abs1_(ri), wa, g);
    }
  }
  if (lane == 0) sh[wv] = ratio;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}
// out[0] = max of part[0..cnt)   (one workgroup)
__global__ __launch_bounds__(256) void max_final_kernel(const double* __restrict__ part, int64_t cnt, double* __restrict__ out) {
  __shared__ double sh[256];
  double m = 0.0;
  for (int64_t b = threadIdx.x; b < cnt; b += 256) m = fmax(m, part[b]);
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}
// part[b] = max over the workgroup's entries of cabs1(x)
template <class T>
__global__ __launch_bounds__(256) void absmax_part_kernel(const T* __restrict__ x, int64_t n, double* __restrict__ part) {
  __shared__ double sh[256];
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
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
// v = |r| + nz eps w (+ safe1 where w is tiny): the xGERFS weights of the forward error bound
template <class T>
__global__ __launch_bounds__(256) void ferr_weights_kernel(const T* __restrict__ r, const double* __restrict__ w, double* __restrict__ v, int64_t n,
                                                           double nzeps, ResidArgs g) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double wi = w[i];
  v[i] = wi > g.safe2 ? abs1_(r[i]) + nzeps * wi : abs1_(r[i]) + nzeps * wi + g.safe1;
}
template <class T>
__global__ __launch_bounds__(256) void axpy1_kernel(T* __restrict__ x, const T* __restrict__ d, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = add_(x[i], d[i]);
}
// sums[i] = sum_e |val[e]| over entry range i (a column of CSC or a row of CSR), in entry order
template <class T>
__global__ __launch_bounds__(256) void abssum_kernel(const int64_t* __restrict__ ptr, const T* __restrict__ val, int64_t n, double* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) acc += abs_(val[e]);
  sums[i] = acc;
}
__global__ __launch_bounds__(256) void dmax_part_kernel(const double* __restrict__ a, int64_t n, double* __restrict__ part) {
  __shared__ double sh[256];
  double m = 0.0;
  for (int q = 0; q < CE_ROWS / 256; ++q) {
    const int64_t i = (int64_t)blockIdx.x * CE_ROWS + q * 256 + threadIdx.x;
    if (i < n) m = fmax(m, a[i]);
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
// CSR map of the pattern: count entries per row, scan, place, sort each row by column
__global__ __launch_bounds__(256) void csr_count_kernel(const int32_t* __restrict__ rowval, int64_t nnz, unsigned long long* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < nnz) atomicAdd(cnt + rowval[e] + 1, 1ull);
}
// inclusive scan of a[0..len) in place (one workgroup of 1024: contiguous chunks, a scan of the chunk sums in LDS, then the chunks)
__global__ __launch_bounds__(1024) void scan_kernel(int64_t* __restrict__ a, int64_t len) {
  __shared__ int64_t sh[1024];
  const int64_t chunk = (len + 1023) / 1024;
  const int64_t lo = (int64_t)threadIdx.x * chunk, hi = min(len, lo + chunk);
  int64_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += a[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int st = 1; st < 1024; st <<= 1) {
    const int64_t v = (int)threadIdx.x >= st ? sh[threadIdx.x - st] : 0;
    __syncthreads();
    sh[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t run = sh[threadIdx.x] - s;  // exclusive prefix of this chunk
  for (int64_t i = lo; i < hi; ++i) {
    run += a[i];
    a[i] = run;
  }
}
__global__ __launch_bounds__(256) void csr_place_kernel(const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval, int64_t n,
                                                        unsigned long long* __restrict__ cursor, int32_t* __restrict__ colind, int64_t* __restrict__ tperm) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  for (int64_t e = colptr[c]; e < colptr[c + 1]; ++e) {
    const unsigned long long at = atomicAdd(cursor + rowval[e], 1ull);
    colind[at] = (int32_t)c;
    tperm[at] = e;
  }
}
__global__ __launch_bounds__(256) void csr_sort_kernel(const int64_t* __restrict__ rowptr, int32_t* __restrict__ colind, int64_t* __restrict__ tperm, int64_t n) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int64_t lo = rowptr[r], hi = rowptr[r + 1];
  for (int64_t a = lo + 1; a < hi; ++a) {  // insertion sort: stencil rows are short, the map is built once
    const int32_t c = colind[a];
    const int64_t p = tperm[a];
    int64_t k = a;
    while (k > lo && colind[k - 1] > c) {
      colind[k] = colind[k - 1];
      tperm[k] = tperm[k - 1];
      --k;
    }
    colind[k] = c;
    tperm[k] = p;
  }
}
__global__ __launch_bounds__(256) void seglen_max_kernel(const int64_t* __restrict__ ptr, int64_t n, unsigned long long* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) atomicMax(out, (unsigned long long)(ptr[i + 1] - ptr[i]));
}

// ---- device buffers, handle cache --------------------------------------------------------------------------------------------------
void csrmap_free(void* p) {
  CsrMap* m = (CsrMap*)p;
  if (m->owned)
    for (void* q : {(void*)m->rowptr, (void*)m->colind, (void*)m->tperm})
      if (q) (void)hipFree(q);
  if (m->valr) (void)hipFree(m->valr);
  delete m;
}
CsrMap* cache_of(const HsHandleView& v) {
  if (!*v.cx) {
    *v.cx = new CsrMap();
    *v.cx_free = csrmap_free;
  }
  return (CsrMap*)*v.cx;
}
int64_t seg_max(const int64_t* ptr, int64_t n, hipStream_t s) {
  DevBuf buf;
  unsigned long long* d = buf.get<unsigned long long>(1);
  CE_HIP(hipMemsetAsync(d, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(seglen_max_kernel, dim3(nb256(n)), dim3(256), 0, s, ptr, n, d);
  unsigned long long m = 0;
  CE_HIP(hipMemcpyAsync(&m, d, sizeof m, hipMemcpyDeviceToHost, s));
  CE_HIP(hipStreamSynchronize(s));
  return (int64_t)m;
}
}  // namespace
namespace hs_ce {
int64_t max_col(const HsHandleView& v, hipStream_t s) {
  CsrMap* m = cache_of(v);
  if (m->maxcol < 0) m->maxcol = seg_max(v.colptr, v.n, s);
  return m->maxcol;
}
// the CSR map (built on first use), its values gathered from the CSC values of the last hs_numeric_begin
template <class T>
CsrMap* csr_of(const HsHandleView& v, hipStream_t s) {
  CsrMap* m = cache_of(v);
  const int64_t n = v.n, nnz = v.nnz;
  if (!m->rowptr) {
    if (v.rowptr) {
      m->rowptr = (int64_t*)v.rowptr;
      m->colind = (int32_t*)v.colind;
      m->tperm = (int64_t*)v.tperm;
      m->owned = false;
    } else {
      int64_t* rp = nullptr;
      int32_t* ci = nullptr;
      int64_t* tp = nullptr;
      CE_HIP(hipMalloc((void**)&rp, sizeof(int64_t) * (size_t)(n + 1)));
      if (hipMalloc((void**)&ci, sizeof(int32_t) * (size_t)std::max<int64_t>(nnz, 1)) != hipSuccess ||
          hipMalloc((void**)&tp, sizeof(int64_t) * (size_t)std::max<int64_t>(nnz, 1)) != hipSuccess) {
        (void)hipFree(rp);
        if (ci) (void)hipFree(ci);
        CE_FAIL(HS_ERR_NOMEM, 0, "hipMalloc of the CSR map of A failed");
      }
      m->rowptr = rp;
      m->colind = ci;
      m->tperm = tp;
      m->owned = true;
      DevBuf buf;
      unsigned long long* cur = buf.get<unsigned long long>((size_t)n);
      CE_HIP(hipMemsetAsync(rp, 0, sizeof(int64_t) * (size_t)(n + 1), s));
      hipLaunchKernelGGL(csr_count_kernel, dim3(nb256(nnz)), dim3(256), 0, s, v.rowval, nnz, (unsigned long long*)rp);
      hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, rp, n + 1);
      CE_HIP(hipMemcpyAsync(cur, rp, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToDevice, s));
      hipLaunchKernelGGL(csr_place_kernel, dim3(nb256(n)), dim3(256), 0, s, v.colptr, v.rowval, n, cur, ci, tp);
      hipLaunchKernelGGL(csr_sort_kernel, dim3(nb256(n)), dim3(256), 0, s, (const int64_t*)rp, ci, tp, n);
      CE_HIP(hipStreamSynchronize(s));  // `cur` goes with buf
    }
    m->maxrow = seg_max(m->rowptr, n, s);
  }
  if (!m->valr) {
    void* q = nullptr;
    if (hipMalloc(&q, sizeof(T) * (size_t)std::max<int64_t>(nnz, 1)) != hipSuccess) CE_FAIL(HS_ERR_NOMEM, 0, "hipMalloc of the CSR values of A failed");
    m->valr = q;
  }
  launch_perm_gather<T>((const T*)v.nz, m->tperm, (T*)m->valr, nnz, s);
  return m;
}
template CsrMap* csr_of<double>(const HsHandleView&, hipStream_t);
template CsrMap* csr_of<cplx>(const HsHandleView&, hipStream_t);
}  // namespace hs_ce
namespace {

// ---- solves --------------------------------------------------------------------------------------------------------------------------
// op(F)^-1 by code: 0 = F^-1, 1 = F^-T, 2 = F^-H, 3 = conj(F)^-1 (= conj(F^-1 conj(.))); adj() gives the code of the adjoint
inline int adj(int code) { return code == 0 ? 2 : code == 1 ? 3 : code == 2 ? 0 : 1; }
template <class T>
struct Ctx {
  hs_handle* F;
  HsHandleView v;
  hipStream_t s;
  int64_t n;
  int64_t nsolves = 0;
  double* res = nullptr;  // device: the scalars the host reads
  void solve(int code, T* X, int t) {
    const bool cx = sizeof(T) == 16;
    if (!cx) code = (code == 2) ? 1 : (code == 3 ? 0 : code);
    if (code == 3) hipLaunchKernelGGL(conj_kernel<T>, dim3(nb256(n * t)), dim3(256), 0, s, X, n * t);
    const int tr = code == 3 ? 0 : code;
    if (cx)
      CE_CHECK(hs_ldiv_dev_t_z(F, tr, (double*)X, n, (const double*)X, n, n, t, (void*)s));
    else
      CE_CHECK(hs_ldiv_dev_t_d(F, tr, (double*)X, n, (const double*)X, n, n, t, (void*)s));
    if (code == 3) hipLaunchKernelGGL(conj_kernel<T>, dim3(nb256(n * t)), dim3(256), 0, s, X, n * t);
    nsolves += t;
  }
  void read(double* out, int cnt) {  // the only host <-> device synchronisation of the drivers
    CE_HIP(hipMemcpyAsync(out, res, sizeof(double) * cnt, hipMemcpyDeviceToHost, s));
    CE_HIP(hipStreamSynchronize(s));
    CE_CHECK(hs_handle_flow_check(F));
  }
};

// B X = diag(vf) op_fwd(F)^-1 X ;  B^H X = op_adj(F)^-1 diag(va) X   (vf, va may be null)
struct EstOp {
  int fwd, adj;
  const double* vf;
  const double* va;
};

// Higham & Tisseur, Algorithm 2.4 (the steps are numbered as in the issue of this feature and in tests/normest_mirror.py)
template <class T>
double normest1(Ctx<T>& c, const EstOp& op, int t, int itmax) {
  const int64_t n = c.n;
  const bool real = sizeof(T) == 8;
  hipStream_t s = c.s;
  DevBuf buf;
  T* X = buf.get<T>((size_t)n * t);
  T* Y = buf.get<T>((size_t)n * t);
  T* S = buf.get<T>((size_t)n * t);
  T* So = buf.get<T>((size_t)n * t);
  T* Z = buf.get<T>((size_t)n * t);
  double* h = buf.get<double>((size_t)n);
  const unsigned nblk = nbrows(n);
  double* part = buf.get<double>((size_t)nblk * CE_MAXT);
  double* cand_h = buf.get<double>((size_t)nblk * CE_MAXT);
  long long* cand_i = buf.get<long long>((size_t)nblk * CE_MAXT);
  double* bmax = buf.get<double>((size_t)nblk);
  unsigned long long* dots = buf.get<unsigned long long>((size_t)CE_MAXT * 2 * CE_MAXT);
  const size_t bytes = sizeof(T) * (size_t)n * t;
  auto applyB = [&](const T* in, T* out) {
    CE_HIP(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, s));
    c.solve(op.fwd, out, t);
    if (op.vf) hipLaunchKernelGGL(scale_rows_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, out, op.vf, n, t);
  };
  auto applyBH = [&](const T* in, T* out) {
    CE_HIP(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, s));
    if (op.va) hipLaunchKernelGGL(scale_rows_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, out, op.va, n, t);
    c.solve(op.adj, out, t);
  };
  // exact +-1 dot products of the sign columns j0.. j1-1 with [S  S_old]: D[(j - j0) * 2t + q]
  std::vector<long long> D((size_t)CE_MAXT * 2 * CE_MAXT);
  auto pm_dots = [&](int j0, int j1) {
    const int np = (j1 - j0) * 2 * t;
    CE_HIP(hipMemsetAsync(dots, 0, sizeof(unsigned long long) * np, s));
    hipLaunchKernelGGL(pm_dots_kernel, dim3(nblk, np), dim3(256), 0, s, (const double*)S, (const double*)So, n, t, j0, dots);
    CE_HIP(hipMemcpyAsync(D.data(), dots, sizeof(long long) * np, hipMemcpyDeviceToHost, s));
    CE_HIP(hipStreamSynchronize(s));
    CE_CHECK(hs_handle_flow_check(c.F));
  };
  const long long nn = (long long)n;

  // 1. start
  Keys keys{};
  for (int j = 0; j < t; ++j) keys.k[j] = col_key(c.v.seed, j, 0);
  hipLaunchKernelGGL(init_x_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, X, n, t, keys, 1.0 / (double)n);
  Hist hist{};
  hist.cnt = 0;
  Sel ind{};
  double est = 0.0, est_old = 0.0;
  long long ind_best = -1;
  double r[16];
  for (int k = 1;; ++k) {
    // 2. Y = B X, est = max_j ||Y[:, j]||_1
    applyB(X, Y);
    hipLaunchKernelGGL(colnorm_part_kernel<T>, dim3(nblk, t), dim3(256), 0, s, (const T*)Y, n, part);
    hipLaunchKernelGGL(est_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (int)nblk, t, c.res);
    c.read(r, 2);
    est = r[0];
    const int jmax = (int)r[1];
    if ((est > est_old || k == 2) && k >= 2) ind_best = ind.idx[jmax];
    if (k >= 2 && est <= est_old) {
      est = est_old;
      break;
    }
    // 3. iteration limit
    est_old = est;
    std::swap(S, So);  // S_old = S
    const bool have_old = k >= 2;
    if (k > itmax) break;
    // 4. signs
    hipLaunchKernelGGL(sign_kernel<T>, dim3(nb256(n * t)), dim3(256), 0, s, (const T*)Y, S, n * t);
    // 5. parallel columns (real only)
    if (real) {
      if (have_old) {
        pm_dots(0, t);
        bool all_par = true;
        for (int j = 0; j < t && all_par; ++j) {
          bool par = false;
          for (int q = 0; q < t; ++q) par |= std::llabs(D[(size_t)j * 2 * t + t + q]) == nn;
          all_par &= par;
        }
        if (all_par) break;
      }
      if (t > 1) {
        for (int j = 0; j < t; ++j) {
          if (j == 0 && !have_old) continue;
          for (int attempt = 1;; ++attempt) {
            pm_dots(j, j + 1);
            bool par = false;
            for (int q = 0; q < j; ++q) par |= std::llabs(D[q]) == nn;
            if (have_old)
              for (int q = 0; q < t; ++q) par |= std::llabs(D[t + q]) == nn;
            if (!par || attempt > 32) break;
            hipLaunchKernelGGL(resample_kernel, dim3(nb256(n)), dim3(256), 0, s, (double*)S + (size_t)j * n, n, col_key(c.v.seed, j, k * 64 + attempt));
          }
        }
      }
    }
    // 6. Z = B^H S, h_i = max_j |Z[i, j]|
    applyBH(S, Z);
    hipLaunchKernelGGL(rowmax_top_kernel<T>, dim3(nblk), dim3(256), 0, s, (const T*)Z, n, t, h, hist, cand_h, cand_i, bmax);
    hipLaunchKernelGGL(select_final_kernel, dim3(1), dim3(256), 0, s, (const double*)cand_h, (const long long*)cand_i, (const double*)bmax, (int)nblk, t,
                       (const double*)h, hist, ind_best, c.res);
    c.read(r, 8 + t);
    if (k >= 2 && r[2] == r[3]) break;
    // 7. the next unit vectors: the t largest h_i outside the history
    if (t > 1 && r[4] != 0.0) break;
    if ((int)r[5] < t) break;  // fewer than t rows left outside the history
    for (int j = 0; j < t; ++j) {
      ind.idx[j] = (long long)r[8 + j];
      hist.idx[hist.cnt++] = ind.idx[j];
    }
    hipLaunchKernelGGL(unit_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, X, n, t, ind);
  }
  return est;
}

// ---- argument checks: refuse, never drop ----------------------------------------------------------------------------------------------
HsHandleView checked_view(hs_handle* F, const char* fn) {
  if (!F) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null factorization handle", fn);
  HsHandleView v;
  hs_handle_view(F, &v);
  if (!v.device) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: handle holds a host-side plan only (hs_plan)", fn);
  if (v.nranks > 1) CE_FAIL(HS_ERR_UNSUPPORTED, v.nranks, "%s: a factorization over %d ranks is not supported (single-rank factorizations only)", fn, v.nranks);
  return v;
}
void check_factored(const HsHandleView& v, const char* fn) {
  if (!v.factored) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: factorization is not complete", fn);
}
void check_t_solves(const HsHandleView& v, const char* fn, const char* what) {
  if (v.t_refused_node >= 0)
    CE_FAIL(HS_ERR_UNSUPPORTED, v.t_refused_node, "%s: %s needs transposed solves, and node %d keeps its interior block D as an HSS matrix (hs_options.hss_d / mf = 2, 3): "
            "transposed ULV solves are not implemented", fn, what, v.t_refused_node);
}
void check_t(const HsHandleView& v, int64_t t, const char* fn) {
  const int64_t tmax = std::min<int64_t>(CE_MAXT, v.n);
  if (t < 1 || t > tmax) CE_FAIL(HS_ERR_ARGUMENT, t, "ArgumentError: %s: t = %lld outside 1:%lld (min(8, n))", fn, (long long)t, (long long)tmax);
}

// ---- drivers -------------------------------------------------------------------------------------------------------------------------
template <class T>
double opnorm_impl(hs_handle* F, const HsHandleView& v, int p, hipStream_t s) {
  DevBuf buf;
  const int64_t n = v.n;
  double* sums = buf.get<double>((size_t)n);
  double* part = buf.get<double>((size_t)nbrows(n));
  double* out = buf.get<double>(1);
  if (p == 1) {
    hipLaunchKernelGGL(abssum_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, v.colptr, (const T*)v.nz, n, sums);
  } else {
    CsrMap* m = csr_of<T>(v, s);
    hipLaunchKernelGGL(abssum_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, (const int64_t*)m->rowptr, (const T*)m->valr, n, sums);
  }
  hipLaunchKernelGGL(dmax_part_kernel, dim3(nbrows(n)), dim3(256), 0, s, (const double*)sums, n, part);
  hipLaunchKernelGGL(max_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (int64_t)nbrows(n), out);
  double r = 0.0;
  CE_HIP(hipMemcpyAsync(&r, out, sizeof r, hipMemcpyDeviceToHost, s));
  CE_HIP(hipStreamSynchronize(s));
  CE_CHECK(hs_handle_flow_check(F));
  return r;
}

template <class T>
double normestinv_impl(hs_handle* F, const HsHandleView& v, int trans, int t, int itmax, int64_t* nsolves, hipStream_t s) {
  DevBuf buf;
  Ctx<T> c{F, v, s, v.n};
  c.res = buf.get<double>(64);
  const double est = normest1<T>(c, EstOp{trans, adj(trans), nullptr, nullptr}, t, itmax);
  if (nsolves) *nsolves = c.nsolves;
  return est;
}

template <class T>
void refine_dev(hs_handle* F, const HsHandleView& v, int trans, T* dX, int64_t ldx, const T* dB, int64_t ldb, int64_t nrhs, int64_t itmax, double* berr,
                double* ferr, int64_t* steps, hipStream_t s) {
  const int64_t n = v.n;
  DevBuf buf;
  Ctx<T> c{F, v, s, n};
  c.res = buf.get<double>(64);
  T* r = buf.get<T>((size_t)n);
  T* d = buf.get<T>((size_t)n);
  double* w = buf.get<double>((size_t)n);
  double* wv = buf.get<double>((size_t)n);
  double* part = buf.get<double>((size_t)std::max<int64_t>(nb256(n), (n + 3) / 4));
  // rows of op(A): the CSR map (op = N) or the CSC arrays (op = T, H)
  const int64_t *ptr;
  const int32_t* idx;
  const T* val;
  int64_t maxlen;
  if (trans == 0) {
    CsrMap* m = csr_of<T>(v, s);
    ptr = m->rowptr;
    idx = m->colind;
    val = (const T*)m->valr;
    maxlen = m->maxrow;
  } else {
    ptr = v.colptr;
    idx = v.rowval;
    val = (const T*)v.nz;
    maxlen = max_col(v, s);
  }
  const bool cj = trans == 2 && sizeof(T) == 16;
  const bool wave = maxlen > CE_WAVE_ROW;
  const double nz = (double)(maxlen + 1);
  ResidArgs g{nz * CE_SAFMIN, nz * CE_SAFMIN / CE_EPS};
  const int64_t npart = wave ? (n + 3) / 4 : (int64_t)nb256(n);
  auto residual = [&](const T* x, const T* b) {
    if (wave) {
      auto k = cj ? resid_wave_kernel<T, true> : resid_wave_kernel<T, false>;
      hipLaunchKernelGGL(k, dim3((unsigned)npart), dim3(256), 0, s, ptr, idx, val, x, b, r, w, part, n, g);
    } else {
      auto k = cj ? resid_kernel<T, true> : resid_kernel<T, false>;
      hipLaunchKernelGGL(k, dim3((unsigned)npart), dim3(256), 0, s, ptr, idx, val, x, b, r, w, part, n, g);
    }
    hipLaunchKernelGGL(max_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, npart, c.res);
  };
  for (int64_t col = 0; col < nrhs; ++col) {
    T* x = dX + col * ldx;
    const T* b = dB + col * ldb;
    CE_HIP(hipMemcpyAsync(x, b, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, s));
    c.solve(trans, x, 1);
    double lst = 3.0, be = 0.0;
    int64_t cnt = 0;
    for (;;) {
      residual(x, b);
      c.read(&be, 1);
      if (!(be > CE_EPS && 2.0 * be <= lst && cnt < itmax)) break;
      CE_HIP(hipMemcpyAsync(d, r, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, s));
      c.solve(trans, d, 1);
      hipLaunchKernelGGL(axpy1_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, x, (const T*)d, n);
      lst = be;
      ++cnt;
    }
    berr[col] = be;
    steps[col] = cnt;
    if (ferr) {
      // || |op(A)^-1| v ||_Inf = || diag(v) op(A)^-H ||_1, estimated on diag(v) op(F)^-H
      hipLaunchKernelGGL(ferr_weights_kernel<T>, dim3(nb256(n)), dim3(256), 0, s, (const T*)r, (const double*)w, wv, n, nz * CE_EPS, g);
      const double est = normest1<T>(c, EstOp{adj(trans), trans, wv, wv}, (int)std::min<int64_t>(2, n), 5);
      hipLaunchKernelGGL(absmax_part_kernel<T>, dim3(nbrows(n)), dim3(256), 0, s, (const T*)x, n, part);
      hipLaunchKernelGGL(max_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (int64_t)nbrows(n), c.res);
      double xn = 0.0;
      c.read(&xn, 1);
      ferr[col] = xn != 0.0 ? est / xn : est;
    }
  }
  CE_HIP(hipStreamSynchronize(s));
  CE_CHECK(hs_handle_flow_check(F));
}

template <class T>
void refine_entry(hs_handle* F, int trans, T* X, int64_t ldx, const T* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax, double* berr, double* ferr,
                  int64_t* steps, bool on_device, void* stream) {
  const char* fn = on_device ? "hs_ldiv_refine_dev_*" : "hs_ldiv_refine_*";
  const HsHandleView v = checked_view(F, fn);
  check_factored(v, fn);
  if ((v.is_complex != 0) != (sizeof(T) == 16)) CE_FAIL(HS_ERR_ARGUMENT, 0, "MethodError: %s: eltype of F and B differ", fn);
  if (trans < 0 || trans > 2) CE_FAIL(HS_ERR_ARGUMENT, trans, "ArgumentError: %s: trans = %d (0: F, 1: transpose(F), 2: adjoint(F))", fn, trans);
  if (n != v.n || nrhs < 0 || ldx < n || ldb < n)
    CE_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: B has %lld rows (ldx %lld, ldb %lld, nrhs %lld), F is %lld x %lld", fn, (long long)n, (long long)ldx,
            (long long)ldb, (long long)nrhs, (long long)v.n, (long long)v.n);
  if (itmax < 0) CE_FAIL(HS_ERR_ARGUMENT, itmax, "ArgumentError: %s: itmax = %lld < 0", fn, (long long)itmax);
  if (nrhs > 0 && (!X || !B || !berr || !steps)) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: X, B, berr and steps must not be NULL", fn);
  if (trans != 0) check_t_solves(v, fn, "trans != 0");
  if (ferr) check_t_solves(v, fn, "the forward error bound ferr");
  if (nrhs == 0) return;
  if (on_device) {
    const T* xb = X;
    if (xb < B + (size_t)ldb * nrhs && B < xb + (size_t)ldx * nrhs) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: X may not alias B", fn);
    return refine_dev<T>(F, v, trans, X, ldx, B, ldb, nrhs, itmax, berr, ferr, steps, (hipStream_t)stream);
  }
  hipStream_t s = v.stream;
  DevBuf buf;
  T* dX = buf.get<T>((size_t)n * nrhs);
  T* dB = buf.get<T>((size_t)n * nrhs);
  CE_HIP(hipMemcpy2DAsync(dB, sizeof(T) * n, B, sizeof(T) * ldb, sizeof(T) * n, nrhs, hipMemcpyHostToDevice, s));
  refine_dev<T>(F, v, trans, dX, n, dB, n, nrhs, itmax, berr, ferr, steps, s);
  CE_HIP(hipMemcpy2DAsync(X, sizeof(T) * ldx, dX, sizeof(T) * n, sizeof(T) * n, nrhs, hipMemcpyDeviceToHost, s));
  CE_HIP(hipStreamSynchronize(s));
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
extern "C" int hs_opnorm(hs_handle* F, int p, double* norm) {
  CE_GUARD(const HsHandleView v = checked_view(F, "hs_opnorm"); if (p != 0 && p != 1) CE_FAIL(HS_ERR_ARGUMENT, p, "ArgumentError: hs_opnorm: p = %d (1 or 0 = Inf)", p);
           if (!norm) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_opnorm: norm == NULL");
           *norm = v.is_complex ? opnorm_impl<cplx>(F, v, p, v.stream) : opnorm_impl<double>(F, v, p, v.stream));
}

extern "C" int hs_normestinv(hs_handle* F, int trans, int64_t t, int64_t itmax, double* est, int64_t* nsolves, void* stream) {
  CE_GUARD(const HsHandleView v = checked_view(F, "hs_normestinv"); check_factored(v, "hs_normestinv");
           if (trans < 0 || trans > 2) CE_FAIL(HS_ERR_ARGUMENT, trans, "ArgumentError: hs_normestinv: trans = %d (0: F, 1: transpose(F), 2: adjoint(F))", trans);
           check_t(v, t, "hs_normestinv");
           if (itmax < 1 || itmax > CE_MAXIT) CE_FAIL(HS_ERR_ARGUMENT, itmax, "ArgumentError: hs_normestinv: itmax = %lld outside 1:%d", (long long)itmax, CE_MAXIT);
           if (!est) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_normestinv: est == NULL");
           check_t_solves(v, "hs_normestinv", "the estimator");
           hipStream_t s = (hipStream_t)stream;
           *est = v.is_complex ? normestinv_impl<cplx>(F, v, trans, (int)t, (int)itmax, nsolves, s) : normestinv_impl<double>(F, v, trans, (int)t, (int)itmax, nsolves, s));
}

extern "C" int hs_condest(hs_handle* F, int p, int64_t t, double* cond, double* normA, double* normFinv, void* stream) {
  CE_GUARD(const HsHandleView v = checked_view(F, "hs_condest"); check_factored(v, "hs_condest");
           if (p != 0 && p != 1) CE_FAIL(HS_ERR_ARGUMENT, p, "ArgumentError: hs_condest: p = %d (1 or 0 = Inf)", p);
           check_t(v, t, "hs_condest"); if (!cond) CE_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_condest: cond == NULL");
           check_t_solves(v, "hs_condest", "the estimator");
           hipStream_t s = (hipStream_t)stream;
           const int trans = p == 1 ? 0 : 1;  // ||F^-1||_Inf = ||F^-T||_1
           const double na = v.is_complex ? opnorm_impl<cplx>(F, v, p, s) : opnorm_impl<double>(F, v, p, s);
           const double ne = v.is_complex ? normestinv_impl<cplx>(F, v, trans, (int)t, 5, nullptr, s) : normestinv_impl<double>(F, v, trans, (int)t, 5, nullptr, s);
           *cond = na * ne; if (normA) *normA = na; if (normFinv) *normFinv = ne);
}

extern "C" int hs_ldiv_refine_d(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                double* berr, double* ferr, int64_t* steps) {
  CE_GUARD(refine_entry<double>(F, trans, X, ldx, B, ldb, n, nrhs, itmax, berr, ferr, steps, false, nullptr));
}
extern "C" int hs_ldiv_refine_z(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                double* berr, double* ferr, int64_t* steps) {
  CE_GUARD(refine_entry<cplx>(F, trans, (cplx*)X, ldx, (const cplx*)B, ldb, n, nrhs, itmax, berr, ferr, steps, false, nullptr));
}
extern "C" int hs_ldiv_refine_dev_d(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                    double* berr, double* ferr, int64_t* steps, void* stream) {
  CE_GUARD(refine_entry<double>(F, trans, dX, ldx, dB, ldb, n, nrhs, itmax, berr, ferr, steps, true, stream));
}
extern "C" int hs_ldiv_refine_dev_z(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                    double* berr, double* ferr, int64_t* steps, void* stream) {
  CE_GUARD(refine_entry<cplx>(F, trans, (cplx*)dX, ldx, (const cplx*)dB, ldb, n, nrhs, itmax, berr, ferr, steps, true, stream));
}
