// kernels_solve_multi.hip -- the one operation of the blocked multi-right-hand-side ldiv! (hs_solve_multi.hip):
//
//   D[M x kc] = A[M x K] X[K x kc]      or      D = Cin - A X,        kc <= 64 right-hand sides,
//
// A a stored factor panel (a 256-column block of L11 / U11, Lbi, Uib, a 256 x 256 inverse diagonal block, or a factor of a low-rank Gauss
// transform), X, Cin and D rows of the row-major work blocks of the driver.
//
// A streaming kernel like the single-vector sweeps, with its FMAs on the FP64 matrix pipe.  2 kc / 8 flop per factor byte is below the
// machine balance up to kc = 32..48, so every factor element has to cross HBM once per call and cost nothing else:
//  * A goes from global memory straight into the registers v_mfma_f64_16x16x4_f64 reads it from (operand A: one f64 per lane, row lane & 15,
//    k = lane >> 4); it is used for ceil(kc / 16) MFMAs and never again, so it never touches LDS.
//    Float64: a workgroup owns 64 rows.  A lane loads the row PAIR (2 i, 2 i + 1), i = lane & 15, of each half of them as one 16-byte access,
//    and the even rows are one MFMA row tile, the odd rows another (the rows of a tile need not be adjacent): a load instruction covers 256
//    consecutive bytes of each of its 4 columns, the wave's two loads 512.  ComplexF64: 32 rows, a lane loads one element (16 bytes) per row
//    tile, re and im are the two operands of the four real MFMAs of a complex product: the same 256 / 512 bytes per column.
//  * The four waves of a workgroup SPLIT K: wave w takes the 16-column chunks w, w + 4, ... of the same rows and the four partial sums meet
//    in LDS in a fixed order ((w0 + w2) + (w1 + w3)).  The sweeps are chains of dependent launches with K = 256, so a step costs what its
//    slowest workgroup costs: with K split, a wave of such a step has four chunks, two in flight at a time (two register arrays: the 8 loads
//    of a chunk are all issued before the MFMAs of the previous one), i.e. two memory round trips and 4 x 16 NT MFMAs per step instead of
//    sixteen and 16 x 16 NT, and a step has four times as many workgroups.  The first form of this kernel -- 256 rows per workgroup, every
//    wave walking all of K in 32-column chunks, the X slab staged in LDS behind two barriers per chunk -- measured 22.9 ms for 32 columns at
//    Poisson 64^3, this one 9.1 ms (DESIGN.md section 4a⁗′).
//  * X is the B operand (k = lane >> 4, column lane & 15): with row-major work blocks a lane group reads 16 adjacent doubles, so X goes from
//    L2 straight to the operand registers as well (negated when the product is subtracted); with K split no two waves of a workgroup use
//    the same rows of X, so there is nothing to share through LDS.  LDS holds the partial sums only: 16 KB per 16 columns.
//  * D is accumulated in registers over the wave's share of K in a fixed order, read once from Cin and written once: no atomics, and a
//    column of D depends on its own column of X and Cin only (the MFMA keeps columns apart), whatever its position in the chunk.
// C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg -- not the f32 map; hsk_multi_prob_* (hs_testhooks.hip) checks it, and the
// row map cmap, with exact integer data (tests/test_ldiv_block_gpu.py).
//
// This file holds what is the forward product's own: MultiFwd (which k a lane loads, the real MFMA chain, the strided split of K, the row
// map of the row-pair tiles), the solve descriptors and the kernels.  The workgroup's body, the complex MFMA chain, the LDS exchange and the
// choice of NT are shared with kernels_solve_multi_t.hip through hs_multi_tile.h; the copy kernel multi_move_kernel serves both directions.
#include "hs_multi_tile.h"

// The forward side of the shared workgroup body (multi_tile_body, hs_multi_tile.h).
template <class T>
struct MultiFwd {
  typedef MultiProb<T> Prob;
  // every row of the workgroup's tile exists: the Float64 loads take whole row pairs then
  static __device__ __forceinline__ bool full(const Prob& p, int r0) { return r0 + hs_multi_rows_per_wg_c(sizeof(T) == 16) <= p.M; }
  // wave wv takes the chunks wv, wv + 4, ... of the nch 16-column chunks of A
  static constexpr int STEP = 4;
  static __device__ __forceinline__ int first(int wv, int nch) { return wv; }
  static __device__ __forceinline__ int end(int wv, int nch) { return nch; }

  // the chunk of A starting at column kb -> registers (a[2 ks + h]: k-step ks, row half / row tile h), and its rows of X (x[ct][ks])
  template <int NT>
  static __device__ __forceinline__ void load(const Prob& p, int kb, int r0, bool fullrows, int l15, int l4, hs_d2u (&a)[2 * HSM_KS], typename MultiX<T>::type (&x)[NT][HSM_KS]) {
    constexpr bool CX = sizeof(T) == 16;
#pragma unroll
    for (int ks = 0; ks < HSM_KS; ++ks) {
      const int col = kb + 4 * ks + l4;
      const T* ap = p.A + (size_t)min(col, p.K - 1) * p.lda;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        hs_d2u v;
        if constexpr (CX) {
          const int rr = r0 + 16 * h + l15;
          v = gld2(ap + min(rr, p.M - 1));
          if (p.trap) {
            if (col == rr) { v.x = 1.0; v.y = 0.0; }
            if (col > rr) { v.x = 0.0; v.y = 0.0; }
          }
        } else {
          const int rr = r0 + 32 * h + 2 * l15;
          if (fullrows) {
            v = gld2(ap + rr);
          } else {
            v.x = gld(ap + min(rr, p.M - 1));
            v.y = gld(ap + min(rr + 1, p.M - 1));
          }
          if (p.trap) {
            v.x = col < rr ? v.x : (col == rr ? 1.0 : 0.0);
            v.y = col < rr + 1 ? v.y : (col == rr + 1 ? 1.0 : 0.0);
          }
        }
        if (col >= p.K) { v.x = 0.0; v.y = 0.0; }
        a[2 * ks + h] = v;
      }
      // (columns past kc of a ragged chunk hold whatever the work block held: they stay in their own columns of D and are never stored)
      const T* xp = p.X + (long long)min(col, p.K - 1) * p.xrs + l15;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        typename MultiX<T>::type v = MultiX<T>::load(xp + ct * 16);
        if (col >= p.K) v = (typename MultiX<T>::type)(0.0);
        x[ct][ks] = p.Cin ? -v : v;
      }
    }
  }

  // acc += A_chunk * X_chunk.  Float64: acc[q] is row tile q = 2 h + parity.  ComplexF64: acc[q] re, acc[2 + q] im of row tile q.
  template <int NT>
  static __device__ __forceinline__ void mfma(const hs_d2u (&a)[2 * HSM_KS], const typename MultiX<T>::type (&x)[NT][HSM_KS], v4d (&acc)[4][NT]) {
    if constexpr (sizeof(T) == 16) {
      multi_mfma_cplx<NT>(a, x, acc);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
          for (int ks = 0; ks < HSM_KS; ++ks)
            acc[q][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64((q & 1) ? a[2 * ks + (q >> 1)].y : a[2 * ks + (q >> 1)].x, x[ct][ks], acc[q][ct], 0, 0, 0);
    }
  }

  // row of D held in register g of row tile q
  static __device__ __forceinline__ int row(int r0, int q, int g, int l4) {
    if constexpr (sizeof(T) == 16) return r0 + 16 * q + l4 + 4 * g;
    return r0 + 32 * (q >> 1) + 2 * (l4 + 4 * g) + (q & 1);
  }
};

// the product of a sweep step for one front, from its solve descriptor (false: the front has no such step)
template <class T>
__device__ __forceinline__ bool multi_resolve(const SolveNode<T>& nd, const MultiAux& ax, int mode, int blk, const MultiArgs& a, MultiProb<T>& p) {
  if (nd.ni <= 0) return false;
  T* w1 = (T*)a.W1 + (nd.woff - a.wbase) * a.kcw;
  T* w2 = (T*)a.W2 + nd.woff * a.kcw;
  T* xb = (T*)a.XB + ax.boff * a.kcw;
  const int c0 = blk * 256;
  p.trap = 0;
  p.cmap = nullptr;
  p.xrs = a.kcw;
  p.crs = a.kcw;
  p.Cin = nullptr;
  switch (mode) {
    case HSM_DIAG_L:
    case HSM_DIAG_U:
      if (c0 >= nd.ni) return false;
      p.A = (mode == HSM_DIAG_L ? nd.inv256L : nd.inv256U) + (size_t)blk * 65536;
      p.lda = 256;
      p.M = p.K = min(256, nd.ni - c0);
      p.X = w1 + (long long)c0 * a.kcw;
      p.C = w2 + (long long)c0 * a.kcw;
      return true;
    case HSM_BELOW_L:
      if (c0 + 256 >= nd.ni) return false;
      p.A = nd.LF + (size_t)(c0 + 256) + (size_t)c0 * nd.ldl;
      p.lda = nd.ldl;
      p.M = nd.ni - (c0 + 256);
      p.K = 256;
      p.X = w2 + (long long)c0 * a.kcw;
      p.C = w1 + (long long)(c0 + 256) * a.kcw;
      p.Cin = p.C;
      return true;
    case HSM_BND_L:
      if (nd.mrows <= nd.ni) return false;
      p.A = nd.LF + (size_t)nd.ni;
      p.lda = nd.ldl;
      p.M = nd.mrows - nd.ni;
      p.K = nd.ni;
      p.X = w2;
      p.C = xb;
      p.Cin = xb;
      return true;
    case HSM_UR:
      p.A = nd.UR;
      p.lda = nd.ldu;
      p.M = nd.ni;
      p.K = nd.compressed ? 0 : nd.nb;
      p.X = xb;
      p.Cin = w2;
      p.C = w1;
      return true;
    case HSM_ABOVE_U:
      if (c0 <= 0 || c0 >= nd.ni) return false;
      p.A = nd.LF + (size_t)c0 * nd.ldl;
      p.lda = nd.ldl;
      p.M = c0;
      p.K = min(256, nd.ni - c0);
      p.X = w2 + (long long)c0 * a.kcw;
      p.C = w1;
      p.Cin = w1;
      return true;
  }
  return false;
}

template <class T, int NT>
__global__ __launch_bounds__(256) void multi_level_kernel(const SolveNode<T>* __restrict__ nodes, int mode, int blk, MultiArgs a) {
  __shared__ double red[2 * 16 * NT * 64];
  const SolveNode<T> nd = nodes[blockIdx.y];
  MultiProb<T> p;
  if (!multi_resolve<T>(nd, a.aux[blockIdx.y], mode, blk, a, p)) return;
  if ((int)blockIdx.x * hs_multi_rows_per_wg_c(sizeof(T) == 16) >= p.M) return;
  multi_tile_body<MultiFwd<T>, T, NT>(p, a.kc, red);
}
template <class T, int NT>
__global__ __launch_bounds__(256) void multi_prob_kernel(MultiProb<T> p, int kc) {
  __shared__ double red[2 * 16 * NT * 64];
  multi_tile_body<MultiFwd<T>, T, NT>(p, kc, red);
}

// the caller's column-major block <-> the row-major work blocks of either direction (what, perm_what: hs_solve_multi.h).  perm_what is a
// template argument: as a kernel argument it cost nothing measurable, but the code of both directions' kernel was no longer the parent's
template <class T, int PERM_WHAT>
__global__ __launch_bounds__(256) void multi_move_kernel(const SolveNode<T>* __restrict__ nodes, int what, MultiArgs a) {
  const SolveNode<T> nd = nodes[blockIdx.y];
  const MultiAux ax = a.aux[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (nd.ni <= 0) return;
  const bool bnd = what & 1;
  if (i >= (bnd ? ax.nb : nd.ni)) return;
  T* b = (T*)a.B + gld(nd.fidx + (bnd ? nd.ni + i : (what == PERM_WHAT ? gld(nd.rperm + i) : i)));
  T* w = bnd ? (T*)a.XB + (ax.boff + i) * a.kcw : (what == 0 ? (T*)a.W1 + (nd.woff - a.wbase + i) * a.kcw : (T*)a.W2 + (nd.woff + i) * a.kcw);
  if (what < 2)
    for (int c = 0; c < a.kc; ++c) gst(w + c, gld(b + (long long)c * a.ldb));
  else
    for (int c = 0; c < a.kc; ++c) gst(b + (long long)c * a.ldb, gld(w + c));
}

int hs_multi_rows_per_wg(bool is_complex) { return hs_multi_rows_per_wg_c(is_complex); }

template <class T>
void launch_multi_level(const SolveNode<T>* sn, int nfronts, int mode, int blk, int maxM, const MultiArgs& a, hipStream_t s) {
  if (nfronts <= 0 || maxM <= 0 || a.kc <= 0) return;
  const int tr = hs_multi_rows_per_wg(sizeof(T) == 16);
  const dim3 grid((maxM + tr - 1) / tr, nfronts);
  hs_with_nt((a.kc + 15) / 16, [&](auto nt) {
    hipLaunchKernelGGL((multi_level_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, sn, mode, blk, a);
  });
}
template <class T>
void launch_multi_prob(const MultiProb<T>& p, int kc, hipStream_t s) {
  if (p.M <= 0 || kc <= 0) return;
  const int tr = hs_multi_rows_per_wg(sizeof(T) == 16);
  const dim3 grid((p.M + tr - 1) / tr);
  hs_with_nt((kc + 15) / 16, [&](auto nt) {
    hipLaunchKernelGGL((multi_prob_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, p, kc);
  });
}
template <class T>
void launch_multi_move(const SolveNode<T>* sn, int nfronts, int what, int maxrows, const MultiArgs& a, hipStream_t s, int perm_what) {
  if (nfronts <= 0 || maxrows <= 0 || a.kc <= 0) return;
  const dim3 grid((maxrows + 255) / 256, nfronts);
  if (perm_what == 0)
    hipLaunchKernelGGL((multi_move_kernel<T, 0>), grid, dim3(256), 0, s, sn, what, a);
  else
    hipLaunchKernelGGL((multi_move_kernel<T, 2>), grid, dim3(256), 0, s, sn, what, a);
}

#define INST(T)                                                                                                  \
  template void launch_multi_level<T>(const SolveNode<T>*, int, int, int, int, const MultiArgs&, hipStream_t);  \
  template void launch_multi_prob<T>(const MultiProb<T>&, int, hipStream_t);                                    \
  template void launch_multi_move<T>(const SolveNode<T>*, int, int, int, const MultiArgs&, hipStream_t, int);
INST(double)
INST(cplx)
