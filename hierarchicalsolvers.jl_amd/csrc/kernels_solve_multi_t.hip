// kernels_solve_multi_t.hip -- the one operation of the transposed / adjoint block solve (hs_ldiv_block_t_*, hs_solve_multi.hip):
//
//   D[M x kc] = op(A)^T X[K x kc]      or      D = Cin - op(A)^T X,        A stored K x M column-major, op = identity or conj,
//
// A a stored factor panel read along its columns (a row panel of U11 / L11, Uib, Lbi, a 256 x 256 inverse diagonal block, a factor of a
// low-rank Gauss transform), X, Cin and D rows of the row-major work blocks of the driver, kc <= 64 right-hand sides.
//
// A translation unit of its own, with its own kernels: multi_level_kernel / multi_prob_kernel (kernels_solve_multi.hip) sit at their
// register limit and keep their allocation only as long as nothing else is compiled into their functions (DESIGN.md section 4a⁗″).  What
// the two products have in common -- the workgroup's body (accumulators, chunks in flight, LDS exchange, the read and the store of D), the
// complex MFMA chain, MultiX, the choice of NT -- is source shared through hs_multi_tile.h and instantiated here over MultiTr, this
// file's own operand loads, real MFMA chain, contiguous split of K and row map; the column-major <-> row-major copies of both directions
// are launch_multi_move of kernels_solve_multi.hip.
//
// The forward kernel reads A[M x K] with the OUTPUT rows contiguous; here the REDUCTION index k is the contiguous one.  The A operand of
// v_mfma_f64_16x16x4_f64 wants lane (m = lane & 15, group = lane >> 4) to hold op(A)^T[m, k] = A[k, m] for one k of the group's four per
// k-step; the natural k = kb + 4 ks + group makes every lane fetch isolated 8-byte words.  The sum over k does not care which k a (group,
// k-step) pair holds as long as the X operand uses the same assignment, so a lane owns PAIRS of consecutive k of its column:
//  * Float64:  k(ks) = kb + 8 (ks >> 1) + 2 group + (ks & 1): one 16-byte load per lane and pair of k-steps.  A load instruction covers 64
//    consecutive bytes (4 groups x 16 B) of each of 16 columns, the two loads of a 16-row chunk 128 bytes of each column.
//  * ComplexF64:  k(ks) = kb + 4 ks + group, one 16-byte element per lane: the same 64 bytes per column and instruction, 256 per chunk.
//    re and im are the two operands of the four real MFMAs of a complex product (conj: im is negated as it is loaded).
//  * A workgroup owns 64 (ComplexF64: 32) output rows = columns of A, as four (two) MFMA row tiles of 16 columns each; the four waves SPLIT
//    K into four CONTIGUOUS quarters (a wave streams 512 consecutive bytes of each of its columns when K = 256), 16 k at a time, two
//    chunks in flight in two register arrays, and the partial sums meet in LDS in the fixed order (w0 + w2) + (w1 + w3).
//  * A goes from global memory straight to the operand registers, is used for ceil(kc / 16) MFMAs and never touches LDS; X is the B
//    operand (16 adjacent doubles of a row-major work-block row per lane group), optionally gathered through a row map (the trapezoid
//    form of a low-rank C: C^T x = trap(Lp)^T (P x)).
//  * No atomics, one summation order per output element that depends on K alone, and a column of D depends on its own column of X and Cin
//    only, wherever it sits in the chunk.
// C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg; hsk_multi_prob_t_* (hs_testhooks.hip) checks the maps, xmap included,
// with exact integer data (tests/test_ldiv_block_t_gpu.py).
#include "hs_multi_tile.h"

// value of the unit lower trapezoid at (k, m) given the stored value
__device__ __forceinline__ double multi_t_trap(double v, int k, int m, double diag) { return k > m ? v : (k == m ? diag : 0.0); }

// The transposed side of the shared workgroup body (multi_tile_body, hs_multi_tile.h).
template <class T>
struct MultiTr {
  typedef MultiProbT<T> Prob;
  static __device__ __forceinline__ bool full(const Prob& p, int m0) { return false; }  // (the loads below decide per chunk: fullk)
  // wave wv takes the contiguous quarter [first, end) of the nch 16-row chunks of A
  static constexpr int STEP = 1;
  static __device__ __forceinline__ int first(int wv, int nch) { return wv * ((nch + 3) / 4); }
  static __device__ __forceinline__ int end(int wv, int nch) { return min(nch, first(wv, nch) + (nch + 3) / 4); }

  // the 16 rows kb .. kb + 15 of the workgroup's columns of A -> registers, and the matching rows of X (x[ct][ks]).
  // Float64: a[i * 4 + q] holds k-steps 2 i (.x) and 2 i + 1 (.y) of column tile q.  ComplexF64: a[ks * 2 + q] = (re, im).
  template <int NT>
  static __device__ __forceinline__ void load(const Prob& p, int kb, int m0, bool, int l15, int l4, hs_d2u (&a)[8], typename MultiX<T>::type (&x)[NT][HSM_KS]) {
    constexpr bool CX = sizeof(T) == 16;
    if constexpr (CX) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int m = m0 + 16 * q + l15;
        const T* ap = p.A + (size_t)min(m, p.M - 1) * p.lda;
#pragma unroll
        for (int ks = 0; ks < HSM_KS; ++ks) {
          const int k = kb + 4 * ks + l4;
          hs_d2u v = gld2(ap + min(k, p.K - 1));
          if (p.conj) v.y = -v.y;
          if (p.trap) {
            v.x = multi_t_trap(v.x, k, m, 1.0);
            v.y = multi_t_trap(v.y, k, m, 0.0);
          }
          if (k >= p.K) { v.x = 0.0; v.y = 0.0; }
          a[ks * 2 + q] = v;
        }
      }
    } else {
      const bool fullk = kb + 4 * HSM_KS <= p.K;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = m0 + 16 * q + l15;
        const T* ap = p.A + (size_t)min(m, p.M - 1) * p.lda;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int k = kb + 8 * i + 2 * l4;
          hs_d2u v;
          if (fullk) {
            v = gld2(ap + k);
          } else {
            v.x = gld(ap + min(k, p.K - 1));
            v.y = gld(ap + min(k + 1, p.K - 1));
          }
          if (p.trap) {
            v.x = multi_t_trap(v.x, k, m, 1.0);
            v.y = multi_t_trap(v.y, k + 1, m, 1.0);
          }
          if (k >= p.K) v.x = 0.0;
          if (k + 1 >= p.K) v.y = 0.0;
          a[i * 4 + q] = v;
        }
      }
    }
    // (columns past kc of a ragged chunk hold whatever the work block held: they stay in their own columns of D and are never stored)
#pragma unroll
    for (int ks = 0; ks < HSM_KS; ++ks) {
      const int k = CX ? kb + 4 * ks + l4 : kb + 8 * (ks >> 1) + 2 * l4 + (ks & 1);
      const int kk = min(k, p.K - 1);
      const T* xp = p.X + (long long)(p.xmap ? gld(p.xmap + kk) : kk) * p.xrs + l15;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        typename MultiX<T>::type v = MultiX<T>::load(xp + ct * 16);
        if (k >= p.K) v = (typename MultiX<T>::type)(0.0);
        x[ct][ks] = p.Cin ? -v : v;
      }
    }
  }

  // acc += op(A_chunk)^T X_chunk.  Float64: acc[q] is column tile q.  ComplexF64: acc[q] re, acc[2 + q] im of column tile q.
  template <int NT>
  static __device__ __forceinline__ void mfma(const hs_d2u (&a)[8], const typename MultiX<T>::type (&x)[NT][HSM_KS], v4d (&acc)[4][NT]) {
    if constexpr (sizeof(T) == 16) {
      multi_mfma_cplx<NT>(a, x, acc);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
          for (int ks = 0; ks < HSM_KS; ++ks)
            acc[q][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64((ks & 1) ? a[(ks >> 1) * 4 + q].y : a[(ks >> 1) * 4 + q].x, x[ct][ks], acc[q][ct], 0, 0, 0);
    }
  }

  // row of D (column of A) held in register g of column tile q
  static __device__ __forceinline__ int row(int m0, int q, int g, int l4) { return m0 + 16 * q + l4 + 4 * g; }
};

// the product of a step of the transposed sweeps for one front, from its solve descriptor (false: the front has no such step)
template <class T>
__device__ __forceinline__ bool multi_t_resolve(const SolveNode<T>& nd, const MultiAux& ax, int mode, int blk, int conj, const MultiArgs& a, MultiProbT<T>& p) {
  if (nd.ni <= 0) return false;
  T* w1 = (T*)a.W1 + (nd.woff - a.wbase) * a.kcw;
  T* w2 = (T*)a.W2 + nd.woff * a.kcw;
  T* xb = (T*)a.XB + ax.boff * a.kcw;
  const int c0 = blk * 256;
  const int wl = min(256, nd.ni - c0), c1 = c0 + 256;
  p.trap = 0;
  p.conj = conj;
  p.cmap = nullptr;
  p.xmap = nullptr;
  p.xrs = a.kcw;
  p.crs = a.kcw;
  p.Cin = nullptr;
  p.lda = nd.ldl;
  switch (mode) {
    case HSMT_DIAG_U:
    case HSMT_DIAG_L:
      if (c0 >= nd.ni) return false;
      p.A = (mode == HSMT_DIAG_U ? nd.inv256U : nd.inv256L) + (size_t)blk * 65536;
      p.lda = 256;
      p.M = p.K = wl;
      p.X = w1 + (long long)c0 * a.kcw;
      p.C = w2 + (long long)c0 * a.kcw;
      return true;
    case HSMT_BELOW_U:  // rows of block j, columns below it
      if (c1 >= nd.ni) return false;
      p.A = nd.LF + (size_t)c0 + (size_t)c1 * nd.ldl;
      p.M = nd.ni - c1;
      p.K = 256;
      p.X = w2 + (long long)c0 * a.kcw;
      p.C = w1 + (long long)c1 * a.kcw;
      p.Cin = p.C;
      return true;
    case HSMT_LEFT_U:  // columns of block j, rows above it
      if (c0 <= 0 || c0 >= nd.ni) return false;
      p.A = nd.LF + (size_t)c0 * nd.ldl;
      p.M = wl;
      p.K = c0;
      p.X = w2;
      p.C = w1 + (long long)c0 * a.kcw;
      p.Cin = p.C;
      return true;
    case HSMT_BND_U:
      p.A = nd.UR;
      p.lda = nd.ldu;
      p.M = nd.compressed ? 0 : nd.nb;
      if (p.M <= 0) return false;
      p.K = nd.ni;
      p.X = w2;
      p.C = xb;
      p.Cin = xb;
      return true;
    case HSMT_LB:
      p.A = nd.LF + (size_t)nd.ni;
      p.M = nd.ni;
      p.K = max(nd.mrows - nd.ni, 0);
      p.X = xb;
      p.Cin = w2;
      p.C = w1;
      return true;
    case HSMT_ABOVE_L:  // rows of block j, columns left of it
      if (c0 <= 0 || c0 >= nd.ni) return false;
      p.A = nd.LF + (size_t)c0;
      p.M = c0;
      p.K = wl;
      p.X = w2 + (long long)c0 * a.kcw;
      p.C = w1;
      p.Cin = w1;
      return true;
    case HSMT_LEFT_L:  // columns of block j, rows below it
      if (c1 >= nd.ni) return false;
      p.A = nd.LF + (size_t)c1 + (size_t)c0 * nd.ldl;
      p.M = 256;
      p.K = nd.ni - c1;
      p.X = w2 + (long long)c1 * a.kcw;
      p.C = w1 + (long long)c0 * a.kcw;
      p.Cin = p.C;
      return true;
  }
  return false;
}

template <class T, int NT>
__global__ __launch_bounds__(256) void multi_t_level_kernel(const SolveNode<T>* __restrict__ nodes, int mode, int blk, int conj, MultiArgs a) {
  __shared__ double red[2 * 16 * NT * 64];
  const SolveNode<T> nd = nodes[blockIdx.y];
  MultiProbT<T> p;
  if (!multi_t_resolve<T>(nd, a.aux[blockIdx.y], mode, blk, conj, a, p)) return;
  if ((int)blockIdx.x * hs_multi_rows_per_wg_c(sizeof(T) == 16) >= p.M) return;
  multi_tile_body<MultiTr<T>, T, NT>(p, a.kc, red);
}
template <class T, int NT>
__global__ __launch_bounds__(256) void multi_t_prob_kernel(MultiProbT<T> p, int kc) {
  __shared__ double red[2 * 16 * NT * 64];
  multi_tile_body<MultiTr<T>, T, NT>(p, kc, red);
}

template <class T>
void launch_multi_level_t(const SolveNode<T>* sn, int nfronts, int mode, int blk, int conj, int maxM, const MultiArgs& a, hipStream_t s) {
  if (nfronts <= 0 || maxM <= 0 || a.kc <= 0) return;
  const int tr = hs_multi_rows_per_wg_c(sizeof(T) == 16);
  const dim3 grid((maxM + tr - 1) / tr, nfronts);
  hs_with_nt((a.kc + 15) / 16, [&](auto nt) {
    hipLaunchKernelGGL((multi_t_level_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, sn, mode, blk, conj, a);
  });
}
template <class T>
void launch_multi_prob_t(const MultiProbT<T>& p, int kc, hipStream_t s) {
  if (p.M <= 0 || kc <= 0) return;
  const int tr = hs_multi_rows_per_wg_c(sizeof(T) == 16);
  const dim3 grid((p.M + tr - 1) / tr);
  hs_with_nt((kc + 15) / 16, [&](auto nt) {
    hipLaunchKernelGGL((multi_t_prob_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, p, kc);
  });
}
#define INST(T)                                                                                                         \
  template void launch_multi_level_t<T>(const SolveNode<T>*, int, int, int, int, int, const MultiArgs&, hipStream_t);  \
  template void launch_multi_prob_t<T>(const MultiProbT<T>&, int, hipStream_t);
INST(double)
INST(cplx)
