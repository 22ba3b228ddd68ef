// hs_multi_tr.h -- the transposed / adjoint product's own pieces, D = Cin - op(A)^T X, over the factor scalar S (hs_solve_multi.h):
// MultiTr<T, S>, the side of the shared workgroup body (the k pairs a lane loads, conj, the real MFMA chain, the contiguous split of K, the
// row map), and multi_t_resolve<T, S>, a front's solve descriptor -> the product of a step of the transposed sweeps.  Device-side
// __forceinline__ pieces only, like hs_multi_tile.h; kernels_solve_multi_t.hip (S = T) and kernels_solve_multi_f32.hip (S = F32Of<T>::type)
// instantiate the kernels over them (hs_multi_kernels.h).  The operand layout and the reasons for it are at the head of
// kernels_solve_multi_t.hip.
#pragma once
#include "hs_multi_tile.h"

// value of the unit lower trapezoid at (k, m) given the stored value
template <class R>
__device__ __forceinline__ R multi_trap(R v, int k, int m, R diag) { return k > m ? v : (k == m ? diag : R(0)); }

// The transposed side of the shared workgroup body (multi_tile_body, hs_multi_tile.h).
// MULV = 1: the side of hs_mul_*'s products (MultiProbMulT, hs_solve_multi.h); 0: the solves', whose code does not change with it.
template <class T, class S, int MULV = 0>
struct MultiTr {
  static constexpr bool MUL = MULV != 0, SPLITC = false;
  typedef typename std::conditional<MUL, MultiProbMulT<T, S>, MultiProbT<T, S>>::type Prob;
  typedef MultiElem<S> E;
  typedef typename E::real R;
  static __device__ __forceinline__ bool full(const Prob& p, int m0) { return false; }  // (the loads below decide per chunk: fullk)
  // wave wv takes the contiguous quarter [first, end) of the nch 16-row chunks of A
  static constexpr int STEP = 1;
  static __device__ __forceinline__ int first(int wv, int nch) { return wv * ((nch + 3) / 4); }
  static __device__ __forceinline__ int end(int wv, int nch) { return min(nch, first(wv, nch) + (nch + 3) / 4); }
  static __device__ __forceinline__ bool cin(const Prob& p) { return p.Cin; }
  // MUL: the chunks of A's rows that meet columns m0 .. m0 + RW - 1 of a triangular operand.  trap = 1 keeps k >= m: rows from m0 on;
  // trap = 2 keeps k <= m: rows below min(K, m0 + RW)
  static __device__ __forceinline__ int lo(const Prob& p, int m0, int nch) { return p.trap == 1 ? min(m0 / (4 * HSM_KS), nch) : 0; }
  static __device__ __forceinline__ int hi(const Prob& p, int m0, int nch) {
    return p.trap == 2 ? min((m0 + hs_multi_rows_per_wg_c(sizeof(T) == 16) + 4 * HSM_KS - 1) / (4 * HSM_KS), nch) : nch;
  }

  // the 16 rows kb .. kb + 15 of the workgroup's columns of A -> registers, and the matching rows of X (x[ct][ks]).
  // Float64: a[i * 4 + q] holds k-steps 2 i (.x) and 2 i + 1 (.y) of column tile q.  ComplexF64: a[ks * 2 + q] = (re, im).
  template <int NT>
  static __device__ __forceinline__ void load(const Prob& p, int kb, int m0, bool, int l15, int l4, hs_d2u (&a)[8], typename MultiX<T>::type (&x)[NT][HSM_KS]) {
    constexpr bool CX = sizeof(T) == 16;
    if constexpr (CX) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int m = m0 + 16 * q + l15;
        const S* ap = p.A + (size_t)min(m, p.M - 1) * p.lda;
#pragma unroll
        for (int ks = 0; ks < HSM_KS; ++ks) {
          const int k = kb + 4 * ks + l4;
          typename E::pair v = E::ld2(ap + min(k, p.K - 1));
          if (p.conj) v.y = -v.y;
          if constexpr (MUL) {
            if (p.trap == 1) {
              v.x = multi_trap<R>(v.x, k, m, R(1));
              v.y = multi_trap<R>(v.y, k, m, R(0));
            } else if (p.trap == 2) {
              if (k > m) { v.x = R(0); v.y = R(0); }
            }
          } else if (p.trap) {
            v.x = multi_trap<R>(v.x, k, m, R(1));
            v.y = multi_trap<R>(v.y, k, m, R(0));
          }
          if (k >= p.K) { v.x = R(0); v.y = R(0); }
          a[ks * 2 + q] = E::pack(v);
        }
      }
    } else {
      const bool fullk = kb + 4 * HSM_KS <= p.K;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = m0 + 16 * q + l15;
        const S* ap = p.A + (size_t)min(m, p.M - 1) * p.lda;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int k = kb + 8 * i + 2 * l4;
          typename E::pair v;
          if (fullk) {
            v = E::ld2(ap + k);
          } else {
            v.x = gld(ap + min(k, p.K - 1));
            v.y = gld(ap + min(k + 1, p.K - 1));
          }
          if constexpr (MUL) {
            if (p.trap == 1) {
              v.x = multi_trap<R>(v.x, k, m, R(1));
              v.y = multi_trap<R>(v.y, k + 1, m, R(1));
            } else if (p.trap == 2) {
              v.x = k <= m ? v.x : R(0);
              v.y = k + 1 <= m ? v.y : R(0);
            }
          } else if (p.trap) {
            v.x = multi_trap<R>(v.x, k, m, R(1));
            v.y = multi_trap<R>(v.y, k + 1, m, R(1));
          }
          if (k >= p.K) v.x = R(0);
          if (k + 1 >= p.K) v.y = R(0);
          a[i * 4 + q] = E::pack(v);
        }
      }
    }
    // (columns past kc of a ragged chunk hold whatever the work block held: they stay in their own columns of D and are never stored)
#pragma unroll
    for (int ks = 0; ks < HSM_KS; ++ks) {
      const int k = CX ? kb + 4 * ks + l4 : kb + 8 * (ks >> 1) + 2 * l4 + (ks & 1);
      const int kk = min(k, p.K - 1);
      const T* xp;
      if constexpr (MUL)
        xp = ((p.X2 && kk >= p.split) ? p.X2 + (long long)(kk - p.split) * p.xrs : p.X + (long long)(p.xmap ? gld(p.xmap + kk) : kk) * p.xrs) + l15;
      else
        xp = p.X + (long long)(p.xmap ? gld(p.xmap + kk) : kk) * p.xrs + l15;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        typename MultiX<T>::type v = MultiX<T>::load(xp + ct * 16);
        if (k >= p.K) v = (typename MultiX<T>::type)(0.0);
        if constexpr (MUL)
          x[ct][ks] = p.minus ? -v : v;
        else
          x[ct][ks] = p.Cin ? -v : v;
      }
    }
  }

  // acc += op(A_chunk)^T X_chunk.  Float64: acc[q] is column tile q.  ComplexF64: acc[q] re, acc[2 + q] im of column tile q.
  template <int NT>
  static __device__ __forceinline__ void mfma(const hs_d2u (&af)[8], const typename MultiX<T>::type (&x)[NT][HSM_KS], v4d (&acc)[4][NT]) {
    hs_d2u a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = E::widen(af[i]);
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
template <class T, class S>
__device__ __forceinline__ bool multi_t_resolve(const SolveNode<S>& nd, const MultiAux& ax, int mode, int blk, int conj, const MultiArgs& a, MultiProbT<T, S>& p) {
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

// the product of a step of hs_mul_run (trans = 1, 2) for one front, from its solve descriptor (false: the front has no such step)
template <class T>
__device__ __forceinline__ bool mul_t_resolve(const SolveNode<T>& nd, const MultiAux& ax, int mode, int conj, const MultiArgs& a, MultiProbMulT<T, T>& p) {
  if (nd.ni <= 0) return false;
  T* w1 = (T*)a.W1 + (nd.woff - a.wbase) * a.kcw;
  T* w2 = (T*)a.W2 + nd.woff * a.kcw;
  T* xb = (T*)a.XB + ax.boff * a.kcw;
  p.trap = 0;
  p.conj = conj;
  p.cmap = nullptr;
  p.xmap = nullptr;
  p.xrs = a.kcw;
  p.crs = a.kcw;
  p.Cin = nullptr;
  p.minus = 0;
  p.split = 0;
  p.X2 = nullptr;
  p.lda = nd.ldl;
  switch (mode) {
    case HSMMT_TRAP:
      p.A = nd.LF;
      p.M = nd.ni;
      p.K = max(nd.mrows, nd.ni);
      p.trap = 1;
      p.X = w1;
      p.split = nd.ni;
      p.X2 = xb;
      p.C = w2;
      return true;
    case HSMMT_TRIU:
      p.A = nd.LF;
      p.M = p.K = nd.ni;
      p.trap = 2;
      p.X = w2;
      p.C = w1;
      return true;
    case HSMMT_BND_U:
      if (nd.compressed || nd.nb <= 0) return false;
      p.A = nd.UR;
      p.lda = nd.ldu;
      p.M = nd.nb;
      p.K = nd.ni;
      p.X = w2;
      p.Cin = xb;
      p.C = xb;
      return true;
  }
  return false;
}
