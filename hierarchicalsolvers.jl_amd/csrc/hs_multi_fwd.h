// hs_multi_fwd.h -- the forward product's own pieces, D = Cin - A X, over the factor scalar S (hs_solve_multi.h): MultiFwd<T, S>, the side
// of the shared workgroup body (which k a lane loads, the real MFMA chain, the strided split of K, the row map of the row-pair tiles), and
// multi_resolve<T, S>, a front's solve descriptor -> the product of a sweep step.  Device-side __forceinline__ pieces only, like
// hs_multi_tile.h; kernels_solve_multi.hip (S = T) and kernels_solve_multi_f32.hip (S = F32Of<T>::type) instantiate the kernels over them
// (hs_multi_kernels.h).  The operand layout and the reasons for it are at the head of kernels_solve_multi.hip.
#pragma once
#include "hs_multi_tile.h"

// The forward side of the shared workgroup body (multi_tile_body, hs_multi_tile.h).
// MULV = 1: the side of hs_mul_*'s products (MultiProbMul, hs_solve_multi.h); 0: the solves', whose code does not change with it.
template <class T, class S, int MULV = 0>
struct MultiFwd {
  static constexpr bool MUL = MULV != 0, SPLITC = MULV != 0;
  typedef typename std::conditional<MUL, MultiProbMul<T, S>, MultiProb<T, S>>::type Prob;
  typedef MultiElem<S> E;
  typedef typename E::real R;
  // every row of the workgroup's tile exists: the real loads take whole row pairs then
  static __device__ __forceinline__ bool full(const Prob& p, int r0) { return r0 + hs_multi_rows_per_wg_c(sizeof(T) == 16) <= p.M; }
  // wave wv takes the chunks wv, wv + 4, ... of the nch 16-column chunks of A
  static constexpr int STEP = 4;
  static __device__ __forceinline__ int first(int wv, int nch) { return wv; }
  static __device__ __forceinline__ int end(int wv, int nch) { return nch; }
  static __device__ __forceinline__ bool cin(const Prob& p) {
    if constexpr (MUL)
      return p.Cin || p.C2;
    else
      return p.Cin;
  }
  // MUL: the chunks of A's columns that meet rows r0 .. r0 + RW - 1 of a triangular operand.  trap = 1 keeps col <= row: columns below
  // min(K, r0 + RW); trap = 2 keeps col >= row: columns from r0 on
  static __device__ __forceinline__ int lo(const Prob& p, int r0, int nch) { return p.trap == 2 ? min(r0 / (4 * HSM_KS), nch) : 0; }
  static __device__ __forceinline__ int hi(const Prob& p, int r0, int nch) {
    return p.trap == 1 ? min((r0 + hs_multi_rows_per_wg_c(sizeof(T) == 16) + 4 * HSM_KS - 1) / (4 * HSM_KS), nch) : nch;
  }

  // the chunk of A starting at column kb -> registers (a[2 ks + h]: k-step ks, row half / row tile h), and its rows of X (x[ct][ks])
  template <int NT>
  static __device__ __forceinline__ void load(const Prob& p, int kb, int r0, bool fullrows, int l15, int l4, hs_d2u (&a)[2 * HSM_KS], typename MultiX<T>::type (&x)[NT][HSM_KS]) {
    constexpr bool CX = sizeof(T) == 16;
#pragma unroll
    for (int ks = 0; ks < HSM_KS; ++ks) {
      const int col = kb + 4 * ks + l4;
      const S* ap = p.A + (size_t)min(col, p.K - 1) * p.lda;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        typename E::pair v;
        if constexpr (CX) {
          const int rr = r0 + 16 * h + l15;
          v = E::ld2(ap + min(rr, p.M - 1));
          if constexpr (MUL) {
            if (p.trap == 1) {
              if (col == rr) { v.x = R(1); v.y = R(0); }
              if (col > rr) { v.x = R(0); v.y = R(0); }
            } else if (p.trap == 2) {
              if (col < rr) { v.x = R(0); v.y = R(0); }
            }
          } else if (p.trap) {
            if (col == rr) { v.x = R(1); v.y = R(0); }
            if (col > rr) { v.x = R(0); v.y = R(0); }
          }
        } else {
          const int rr = r0 + 32 * h + 2 * l15;
          if (fullrows) {
            v = E::ld2(ap + rr);
          } else {
            v.x = gld(ap + min(rr, p.M - 1));
            v.y = gld(ap + min(rr + 1, p.M - 1));
          }
          if constexpr (MUL) {
            if (p.trap == 1) {
              v.x = col < rr ? v.x : (col == rr ? R(1) : R(0));
              v.y = col < rr + 1 ? v.y : (col == rr + 1 ? R(1) : R(0));
            } else if (p.trap == 2) {
              v.x = col >= rr ? v.x : R(0);
              v.y = col >= rr + 1 ? v.y : R(0);
            }
          } else if (p.trap) {
            v.x = col < rr ? v.x : (col == rr ? R(1) : R(0));
            v.y = col < rr + 1 ? v.y : (col == rr + 1 ? R(1) : R(0));
          }
        }
        if (col >= p.K) { v.x = R(0); v.y = R(0); }
        a[2 * ks + h] = E::pack(v);
      }
      // (columns past kc of a ragged chunk hold whatever the work block held: they stay in their own columns of D and are never stored)
      const T* xp = p.X + (long long)min(col, p.K - 1) * p.xrs + l15;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        typename MultiX<T>::type v = MultiX<T>::load(xp + ct * 16);
        if (col >= p.K) v = (typename MultiX<T>::type)(0.0);
        if constexpr (MUL)
          x[ct][ks] = p.minus ? -v : v;
        else
          x[ct][ks] = p.Cin ? -v : v;
      }
    }
  }

  // acc += A_chunk * X_chunk.  Float64: acc[q] is row tile q = 2 h + parity.  ComplexF64: acc[q] re, acc[2 + q] im of row tile q.
  template <int NT>
  static __device__ __forceinline__ void mfma(const hs_d2u (&af)[2 * HSM_KS], const typename MultiX<T>::type (&x)[NT][HSM_KS], v4d (&acc)[4][NT]) {
    hs_d2u a[2 * HSM_KS];
#pragma unroll
    for (int i = 0; i < 2 * HSM_KS; ++i) a[i] = E::widen(af[i]);
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
template <class T, class S>
__device__ __forceinline__ bool multi_resolve(const SolveNode<S>& nd, const MultiAux& ax, int mode, int blk, const MultiArgs& a, MultiProb<T, S>& p) {
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

// the product of a step of hs_mul_run (trans = 0) for one front, from its solve descriptor (false: the front has no such step)
template <class T>
__device__ __forceinline__ bool mul_resolve(const SolveNode<T>& nd, const MultiAux& ax, int mode, const MultiArgs& a, MultiProbMul<T, T>& p) {
  if (nd.ni <= 0) return false;
  T* w1 = (T*)a.W1 + (nd.woff - a.wbase) * a.kcw;
  T* w2 = (T*)a.W2 + nd.woff * a.kcw;
  T* xb = (T*)a.XB + ax.boff * a.kcw;
  p.trap = 0;
  p.cmap = nullptr;
  p.xrs = a.kcw;
  p.crs = a.kcw;
  p.Cin = nullptr;
  p.minus = 0;
  p.split = 0;
  p.C2 = nullptr;
  p.lda = nd.ldl;
  switch (mode) {
    case HSMM_TRIU:
      p.A = nd.LF;
      p.M = p.K = nd.ni;
      p.trap = 2;
      p.X = w1;
      p.C = w2;
      return true;
    case HSMM_UR:
      if (nd.compressed || nd.nb <= 0) return false;
      p.A = nd.UR;
      p.lda = nd.ldu;
      p.M = nd.ni;
      p.K = nd.nb;
      p.X = xb;
      p.Cin = w2;
      p.C = w2;
      return true;
    case HSMM_TRAP:
      p.A = nd.LF;
      p.M = max(nd.mrows, nd.ni);
      p.K = nd.ni;
      p.trap = 1;
      p.X = w2;
      p.C = w1;
      p.split = nd.ni;
      p.C2 = xb;
      return true;
  }
  return false;
}
