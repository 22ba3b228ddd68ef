// kernels_solve_multi_f32.hip -- the two panel products of the block solves with the factor panel stored in Float32 / ComplexF32
// (hs_f32_*, hs_f32.hip):
//
//   D = Cin - A X   (MultiFwdF32, the product of kernels_solve_multi.hip)        D = Cin - op(A)^T X   (MultiTrF32, kernels_solve_multi_t.hip)
//
// A is read as S = float / cplxf, carried through the hs_d2u operand registers of the shared workgroup body, multi_tile_body
// (hs_multi_tile.h), and widened in registers (v_cvt_f64_f32, exact) in front of the MFMAs that consume it; X, Cin, D and the
// accumulators are Float64 / ComplexF64 and every FMA is v_mfma_f64_16x16x4_f64.
// Two new kernel SIDES for that body and nothing else of it: the MFMA chains, the split of K over the four waves (forward: chunks w, w + 4,
// ...; transposed: contiguous quarters), the two chunks in flight, the LDS meeting order (w0 + w2) + (w1 + w3), Cin in wave 0's
// accumulators first and the single read and write of D are the body's.  A lane holds the element the FP64 side holds for it, so every
// output element has the summation order of the FP64 kernels: on values that Float32 represents exactly the two give the same bits
// (tests/test_f32_gpu.py compares them so).
//
// Loads.  Float64 handles: the lane's row pair (forward) / k pair (transposed) is 8 bytes, one load; a wave load covers 128 contiguous
// bytes of each of its 4 columns (forward) or 32 bytes of each of 16 columns (transposed).  The copies have even leading dimensions
// (hs_f32_ld), but a panel may start at an odd row (the boundary rows of LF start at ni), so the pair type is 4-byte aligned.  ComplexF64
// handles: one cplxf (8 bytes) per lane and row tile.  Ragged M, K, kc, the clamped edge loads, trap, cmap, xmap and conj are those of the
// FP64 sides.  (A lane taking FOUR rows, 16 bytes, with the row map changed to match, is the wider alternative; not built: DESIGN.md 4m.)
//
// A translation unit of its own, for the reason kernels_solve_multi_t.hip is one: the FP64 kernels keep their register allocation only as
// long as nothing else is compiled into their functions.  The column-major <-> row-major copies are launch_multi_move of
// kernels_solve_multi.hip, unchanged: it reads ni, woff, rperm and fidx of a descriptor, which SolveNode<S> holds where SolveNode<T> does.
#include "hs_f32.h"
#include "hs_multi_tile.h"

typedef float hs_f2u __attribute__((ext_vector_type(2), aligned(4)));  // 8-byte access, 4-byte aligned
__device__ __forceinline__ hs_f2u gldf2(const float* p) { return *(const hs_f2u HS_AS_GLOBAL*)p; }
__device__ __forceinline__ hs_f2u gldf2(const cplxf* p) { return *(const hs_f2u HS_AS_GLOBAL*)p; }
// A loaded pair travels through the body's operand registers as its 8 raw bytes (in .x of the hs_d2u; .y is dead) and is widened where the
// MFMAs consume it.  Widening inside load would make every load's result due at once -- the convert depends on it -- and the loads of a
// chunk are issued before the MFMAs of the previous one precisely so that they are not.
__device__ __forceinline__ hs_d2u f32_pack(hs_f2u f) { return hs_d2u{__builtin_bit_cast(double, f), 0.0}; }
__device__ __forceinline__ hs_d2u f32_widen(hs_d2u a) {
  const hs_f2u f = __builtin_bit_cast(hs_f2u, (double)a.x);
  return hs_d2u{(double)f.x, (double)f.y};
}

// The forward side of the shared workgroup body over a Float32 panel: MultiFwd<T> (kernels_solve_multi.hip) with A loaded as S (load) and
// widened in front of the MFMA chain (mfma).
template <class T>
struct MultiFwdF32 {
  typedef MultiProbF32<T> Prob;
  typedef typename F32Of<T>::type S;
  static __device__ __forceinline__ bool full(const Prob& p, int r0) { return r0 + hs_multi_rows_per_wg_c(sizeof(T) == 16) <= p.M; }
  static constexpr int STEP = 4;
  static __device__ __forceinline__ int first(int wv, int nch) { return wv; }
  static __device__ __forceinline__ int end(int wv, int nch) { return nch; }

  template <int NT>
  static __device__ __forceinline__ void load(const Prob& p, int kb, int r0, bool fullrows, int l15, int l4, hs_d2u (&a)[2 * HSM_KS], typename MultiX<T>::type (&x)[NT][HSM_KS]) {
    constexpr bool CX = sizeof(T) == 16;
#pragma unroll
    for (int ks = 0; ks < HSM_KS; ++ks) {
      const int col = kb + 4 * ks + l4;
      const S* ap = p.A + (size_t)min(col, p.K - 1) * p.lda;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        hs_f2u v;
        if constexpr (CX) {
          const int rr = r0 + 16 * h + l15;
          v = gldf2(ap + min(rr, p.M - 1));
          if (p.trap) {
            if (col == rr) { v.x = 1.0f; v.y = 0.0f; }
            if (col > rr) { v.x = 0.0f; v.y = 0.0f; }
          }
        } else {
          const int rr = r0 + 32 * h + 2 * l15;
          if (fullrows) {
            v = gldf2(ap + rr);
          } else {
            v.x = gld(ap + min(rr, p.M - 1));
            v.y = gld(ap + min(rr + 1, p.M - 1));
          }
          if (p.trap) {
            v.x = col < rr ? v.x : (col == rr ? 1.0f : 0.0f);
            v.y = col < rr + 1 ? v.y : (col == rr + 1 ? 1.0f : 0.0f);
          }
        }
        if (col >= p.K) { v.x = 0.0f; v.y = 0.0f; }
        a[2 * ks + h] = f32_pack(v);
      }
      const T* xp = p.X + (long long)min(col, p.K - 1) * p.xrs + l15;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        typename MultiX<T>::type v = MultiX<T>::load(xp + ct * 16);
        if (col >= p.K) v = (typename MultiX<T>::type)(0.0);
        x[ct][ks] = p.Cin ? -v : v;
      }
    }
  }

  template <int NT>
  static __device__ __forceinline__ void mfma(const hs_d2u (&af)[2 * HSM_KS], const typename MultiX<T>::type (&x)[NT][HSM_KS], v4d (&acc)[4][NT]) {
    hs_d2u a[2 * HSM_KS];
#pragma unroll
    for (int i = 0; i < 2 * HSM_KS; ++i) a[i] = f32_widen(af[i]);
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

  static __device__ __forceinline__ int row(int r0, int q, int g, int l4) {
    if constexpr (sizeof(T) == 16) return r0 + 16 * q + l4 + 4 * g;
    return r0 + 32 * (q >> 1) + 2 * (l4 + 4 * g) + (q & 1);
  }
};

__device__ __forceinline__ float multi_f32_trap(float v, int k, int m, float diag) { return k > m ? v : (k == m ? diag : 0.0f); }

// The transposed side: MultiTr<T> (kernels_solve_multi_t.hip), A loaded as S and widened in front of the MFMA chain alike.
template <class T>
struct MultiTrF32 {
  typedef MultiProbTF32<T> Prob;
  typedef typename F32Of<T>::type S;
  static __device__ __forceinline__ bool full(const Prob& p, int m0) { return false; }
  static constexpr int STEP = 1;
  static __device__ __forceinline__ int first(int wv, int nch) { return wv * ((nch + 3) / 4); }
  static __device__ __forceinline__ int end(int wv, int nch) { return min(nch, first(wv, nch) + (nch + 3) / 4); }

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
          hs_f2u v = gldf2(ap + min(k, p.K - 1));
          if (p.conj) v.y = -v.y;
          if (p.trap) {
            v.x = multi_f32_trap(v.x, k, m, 1.0f);
            v.y = multi_f32_trap(v.y, k, m, 0.0f);
          }
          if (k >= p.K) { v.x = 0.0f; v.y = 0.0f; }
          a[ks * 2 + q] = f32_pack(v);
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
          hs_f2u v;
          if (fullk) {
            v = gldf2(ap + k);
          } else {
            v.x = gld(ap + min(k, p.K - 1));
            v.y = gld(ap + min(k + 1, p.K - 1));
          }
          if (p.trap) {
            v.x = multi_f32_trap(v.x, k, m, 1.0f);
            v.y = multi_f32_trap(v.y, k + 1, m, 1.0f);
          }
          if (k >= p.K) v.x = 0.0f;
          if (k + 1 >= p.K) v.y = 0.0f;
          a[i * 4 + q] = f32_pack(v);
        }
      }
    }
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

  template <int NT>
  static __device__ __forceinline__ void mfma(const hs_d2u (&af)[8], const typename MultiX<T>::type (&x)[NT][HSM_KS], v4d (&acc)[4][NT]) {
    hs_d2u a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = f32_widen(af[i]);
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

  static __device__ __forceinline__ int row(int m0, int q, int g, int l4) { return m0 + 16 * q + l4 + 4 * g; }
};

// the product of a sweep step for one front from its demoted descriptor: multi_resolve (kernels_solve_multi.hip), mode by mode
template <class T>
__device__ __forceinline__ bool multi_resolve_f32(const SolveNode<typename F32Of<T>::type>& nd, const MultiAux& ax, int mode, int blk, const MultiArgs& a, MultiProbF32<T>& p) {
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

// multi_t_resolve (kernels_solve_multi_t.hip), mode by mode
template <class T>
__device__ __forceinline__ bool multi_t_resolve_f32(const SolveNode<typename F32Of<T>::type>& nd, const MultiAux& ax, int mode, int blk, int conj, const MultiArgs& a,
                                                    MultiProbTF32<T>& p) {
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
    case HSMT_BELOW_U:
      if (c1 >= nd.ni) return false;
      p.A = nd.LF + (size_t)c0 + (size_t)c1 * nd.ldl;
      p.M = nd.ni - c1;
      p.K = 256;
      p.X = w2 + (long long)c0 * a.kcw;
      p.C = w1 + (long long)c1 * a.kcw;
      p.Cin = p.C;
      return true;
    case HSMT_LEFT_U:
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
    case HSMT_ABOVE_L:
      if (c0 <= 0 || c0 >= nd.ni) return false;
      p.A = nd.LF + (size_t)c0;
      p.M = c0;
      p.K = wl;
      p.X = w2 + (long long)c0 * a.kcw;
      p.C = w1;
      p.Cin = w1;
      return true;
    case HSMT_LEFT_L:
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
__global__ __launch_bounds__(256) void multi_level_f32_kernel(const SolveNode<typename F32Of<T>::type>* __restrict__ nodes, int mode, int blk, MultiArgs a) {
  __shared__ double red[2 * 16 * NT * 64];
  const SolveNode<typename F32Of<T>::type> nd = nodes[blockIdx.y];
  MultiProbF32<T> p;
  if (!multi_resolve_f32<T>(nd, a.aux[blockIdx.y], mode, blk, a, p)) return;
  if ((int)blockIdx.x * hs_multi_rows_per_wg_c(sizeof(T) == 16) >= p.M) return;
  multi_tile_body<MultiFwdF32<T>, T, NT>(p, a.kc, red);
}
template <class T, int NT>
__global__ __launch_bounds__(256) void multi_prob_f32_kernel(MultiProbF32<T> p, int kc) {
  __shared__ double red[2 * 16 * NT * 64];
  multi_tile_body<MultiFwdF32<T>, T, NT>(p, kc, red);
}
template <class T, int NT>
__global__ __launch_bounds__(256) void multi_t_level_f32_kernel(const SolveNode<typename F32Of<T>::type>* __restrict__ nodes, int mode, int blk, int conj, MultiArgs a) {
  __shared__ double red[2 * 16 * NT * 64];
  const SolveNode<typename F32Of<T>::type> nd = nodes[blockIdx.y];
  MultiProbTF32<T> p;
  if (!multi_t_resolve_f32<T>(nd, a.aux[blockIdx.y], mode, blk, conj, a, p)) return;
  if ((int)blockIdx.x * hs_multi_rows_per_wg_c(sizeof(T) == 16) >= p.M) return;
  multi_tile_body<MultiTrF32<T>, T, NT>(p, a.kc, red);
}
template <class T, int NT>
__global__ __launch_bounds__(256) void multi_t_prob_f32_kernel(MultiProbTF32<T> p, int kc) {
  __shared__ double red[2 * 16 * NT * 64];
  multi_tile_body<MultiTrF32<T>, T, NT>(p, kc, red);
}

template <class T>
void launch_multi_level_f32(const SolveNode<typename F32Of<T>::type>* sn, int nfronts, int mode, int blk, int maxM, const MultiArgs& a, hipStream_t s) {
  if (nfronts <= 0 || maxM <= 0 || a.kc <= 0) return;
  const int tr = hs_multi_rows_per_wg_c(sizeof(T) == 16);
  const dim3 grid((maxM + tr - 1) / tr, nfronts);
  hs_with_nt((a.kc + 15) / 16, [&](auto nt) {
    hipLaunchKernelGGL((multi_level_f32_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, sn, mode, blk, a);
  });
}
template <class T>
void launch_multi_prob_f32(const MultiProbF32<T>& p, int kc, hipStream_t s) {
  if (p.M <= 0 || kc <= 0) return;
  const int tr = hs_multi_rows_per_wg_c(sizeof(T) == 16);
  const dim3 grid((p.M + tr - 1) / tr);
  hs_with_nt((kc + 15) / 16, [&](auto nt) {
    hipLaunchKernelGGL((multi_prob_f32_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, p, kc);
  });
}
template <class T>
void launch_multi_level_t_f32(const SolveNode<typename F32Of<T>::type>* sn, int nfronts, int mode, int blk, int conj, int maxM, const MultiArgs& a, hipStream_t s) {
  if (nfronts <= 0 || maxM <= 0 || a.kc <= 0) return;
  const int tr = hs_multi_rows_per_wg_c(sizeof(T) == 16);
  const dim3 grid((maxM + tr - 1) / tr, nfronts);
  hs_with_nt((a.kc + 15) / 16, [&](auto nt) {
    hipLaunchKernelGGL((multi_t_level_f32_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, sn, mode, blk, conj, a);
  });
}
template <class T>
void launch_multi_prob_t_f32(const MultiProbTF32<T>& p, int kc, hipStream_t s) {
  if (p.M <= 0 || kc <= 0) return;
  const int tr = hs_multi_rows_per_wg_c(sizeof(T) == 16);
  const dim3 grid((p.M + tr - 1) / tr);
  hs_with_nt((kc + 15) / 16, [&](auto nt) {
    hipLaunchKernelGGL((multi_t_prob_f32_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, p, kc);
  });
}
template <class T>
void launch_multi_move_f32(const SolveNode<typename F32Of<T>::type>* sn, int nfronts, int what, int maxrows, const MultiArgs& a, hipStream_t s, int perm_what) {
  launch_multi_move<T>(reinterpret_cast<const SolveNode<T>*>(sn), nfronts, what, maxrows, a, s, perm_what);
}

#define INST(T)                                                                                                                                \
  template void launch_multi_level_f32<T>(const SolveNode<F32Of<T>::type>*, int, int, int, int, const MultiArgs&, hipStream_t);               \
  template void launch_multi_prob_f32<T>(const MultiProbF32<T>&, int, hipStream_t);                                                           \
  template void launch_multi_level_t_f32<T>(const SolveNode<F32Of<T>::type>*, int, int, int, int, int, const MultiArgs&, hipStream_t);        \
  template void launch_multi_prob_t_f32<T>(const MultiProbTF32<T>&, int, hipStream_t);                                                        \
  template void launch_multi_move_f32<T>(const SolveNode<F32Of<T>::type>*, int, int, int, const MultiArgs&, hipStream_t, int);
INST(double)
INST(cplx)
