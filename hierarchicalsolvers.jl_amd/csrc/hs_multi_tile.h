// hs_multi_tile.h -- what the panel-product kernels of the block solves share: the forward product (D = Cin - A X, hs_multi_fwd.h) and the
// transposed one (D = Cin - op(A)^T X, hs_multi_tr.h) hold the same 64- / 32-row tile of D in the same registers, so the workgroup's body --
// the accumulators, the two chunks in flight, the exchange of the partial sums through LDS, the way D is read and written -- is written
// once, here, over the operand loads and MFMA chains of the two sides, and the sides once over the scalar the factor panel is stored in
// (MultiElem).  Device-side __forceinline__ pieces only (and the host-side choice of NT): nothing in this header is a kernel;
// kernels_solve_multi.hip, kernels_solve_multi_t.hip and kernels_solve_multi_f32.hip stay separate translation units.
//
// The tile: acc[q][ct][g] is register g of the MFMA result of row tile q and column tile ct, i.e. column 16 ct + (lane & 15) and the row the
// kernel's row map gives for (q, g) (C/D of v_mfma_f64_16x16x4_f64: row (lane >> 4) + 4 g of the tile).  Float64 has four row tiles,
// ComplexF64 two: acc[q] re, acc[2 + q] im.
#pragma once
#include <type_traits>

#include "hs_solve_multi.h"

typedef double v4d __attribute__((ext_vector_type(4)));
// A chunk is 4 KS = 16 values of the reduction index (4 k-steps of the MFMA) and a wave keeps two of them in flight.  Measured in the forward
// kernel against 32-column chunks (two in flight: 256 VGPRs and the accumulators in AGPRs, one wave per SIMD) and 8-column ones on Poisson /
// Helmholtz 64^3, 32 right-hand sides: 9.1 / 15.2 ms with 16 columns, 10.3 / 28.7 ms with 32, 9.5 / 14.7 ms with 8 (DESIGN.md section
// 4a⁗′).  With 32 the ComplexF64 kernels for 48 and 64 right-hand sides did not fit 512 registers at all (scratch).
#define HSM_KS 4

// an element of X in registers: a double, or (re, im) as a 2-vector
template <class T>
struct MultiX {
  typedef double type;
  static __device__ __forceinline__ double load(const double* p) { return gld(p); }
};
template <>
struct MultiX<cplx> {
  typedef hs_d2u type;
  static __device__ __forceinline__ hs_d2u load(const cplx* p) { return gld2(p); }
};

// An element pair of the factor panel A, stored as S, on its way to the MFMA's A operand: the lane's row pair (forward) / k pair
// (transposed) of a Float64 / Float32 panel, or (re, im) of one ComplexF64 / ComplexF32 element.
//   pair, real   the loaded pair and its component type      ld2    the pair at p as one access
//   pack         the pair -> the body's hs_d2u operand register, as raw bytes      widen    those bytes -> two doubles, at the MFMA
// S = double, cplx: the pair is the hs_d2u itself, one 16-byte access, pack and widen are the identity.
template <class S>
struct MultiElem {
  typedef hs_d2u pair;
  typedef double real;
  static __device__ __forceinline__ pair ld2(const S* p) { return gld2(p); }
  static __device__ __forceinline__ hs_d2u pack(pair v) { return v; }
  static __device__ __forceinline__ hs_d2u widen(hs_d2u a) { return a; }
};
// S = float, cplxf: one 8-byte access.  The demoted copies have even leading dimensions (hs_f32_ld), but a panel may start at an odd row
// (the boundary rows of LF start at ni), so the pair type is 4-byte aligned.  The pair travels through the operand registers as its 8 raw
// bytes (in .x of the hs_d2u; .y is dead) and is widened (v_cvt_f64_f32, exact) where the MFMAs consume it.  Widening inside load would
// make every load's result due at once -- the convert depends on it -- and the loads of a chunk are issued before the MFMAs of the previous
// one precisely so that they are not: 4.53 against 3.08 ms at Poisson 40^3.
typedef float hs_f2u __attribute__((ext_vector_type(2), aligned(4)));
struct MultiElemF32 {
  typedef hs_f2u pair;
  typedef float real;
  static __device__ __forceinline__ pair ld2(const void* p) { return *(const hs_f2u HS_AS_GLOBAL*)p; }
  static __device__ __forceinline__ hs_d2u pack(pair f) { return hs_d2u{__builtin_bit_cast(double, f), 0.0}; }
  static __device__ __forceinline__ hs_d2u widen(hs_d2u a) {
    const hs_f2u f = __builtin_bit_cast(hs_f2u, (double)a.x);
    return hs_d2u{(double)f.x, (double)f.y};
  }
};
template <>
struct MultiElem<float> : MultiElemF32 {};
template <>
struct MultiElem<cplxf> : MultiElemF32 {};

// the complex product of a chunk, four real MFMAs per k-step: a[2 ks + q] = (re, im) of the A operand of k-step ks and row tile q
template <int NT>
__device__ __forceinline__ void multi_mfma_cplx(const hs_d2u (&a)[2 * HSM_KS], const hs_d2u (&x)[NT][HSM_KS], v4d (&acc)[4][NT]) {
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
#pragma unroll
      for (int ks = 0; ks < HSM_KS; ++ks) {
        acc[q][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[2 * ks + q].x, x[ct][ks].x, acc[q][ct], 0, 0, 0);
        acc[q][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[2 * ks + q].y, -x[ct][ks].y, acc[q][ct], 0, 0, 0);
      }
#pragma unroll
      for (int ks = 0; ks < HSM_KS; ++ks) {
        acc[2 + q][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[2 * ks + q].x, x[ct][ks].y, acc[2 + q][ct], 0, 0, 0);
        acc[2 + q][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[2 * ks + q].y, x[ct][ks].x, acc[2 + q][ct], 0, 0, 0);
      }
    }
}

// a wave's partial sums -> its LDS slot, and a slot added to a wave's partial sums (16 NT x 64 doubles, lane-contiguous)
template <int NT>
__device__ __forceinline__ void multi_red_put(double* slot, int lane, const v4d (&acc)[4][NT]) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int g = 0; g < 4; ++g) slot[((q * NT + ct) * 4 + g) * 64 + lane] = acc[q][ct][g];
}
template <int NT>
__device__ __forceinline__ void multi_red_add(const double* slot, int lane, v4d (&acc)[4][NT]) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[q][ct][g] += slot[((q * NT + ct) * 4 + g) * 64 + lane];
}

// The product of one workgroup.  K is the kernel's side of it (hs_multi_fwd.h: MultiFwd<T, S>, hs_multi_tr.h: MultiTr<T, S>):
//   K::Prob                               MultiProb<T, S> / MultiProbT<T, S>
//   K::STEP, K::first / K::end(wv, nch)   wave wv takes the 16-k chunks first, first + STEP, ... < end of the nch chunks of K
//   K::load<NT>(p, kb, r0, l15, l4, a, x) the chunk at kb -> the operand registers a (A) and x (X, negated when the product is subtracted)
//   K::mfma<NT>(a, x, acc)                acc += that chunk's product
//   K::row(r0, q, g, l4)                  the row of D in register g of row tile q
//   K::cin(p)                             D starts from stored values (Cin, or a second block that is added into)
//   K::MUL, K::lo / K::hi(p, r0, nch)     a side of hs_mul_*'s products (hs_solve_multi.h): the chunks [lo, hi) of a triangular operand that meet the
//                                         workgroup's rows are split over the waves, the others are not read; K::SPLITC: D has a second block (C2)
// Two chunks are in flight in two register arrays (the loads of a chunk are all issued before the MFMAs of the previous one); the partial
// sums of the four waves meet in LDS (red: 2 x 16 NT x 64 doubles) in the fixed order (w0 + w2) + (w1 + w3); wave 0 reads Cin into its
// accumulators before the first MFMA and stores D through cmap after the last sum: D is read once and written once, no atomics.
// The BODY is the shared piece and its callees live with the sides, not the other way round: the compiler optimizes an always-inline callee
// on its own before it inlines it, so an accumulator-initialise or a reduce-and-store function called from two written-out bodies changes
// the generated code of both (tried in four forms), while one body over the sides' own callees compiles to the parent's instructions,
// kernel by kernel (profiles/r18_solve_multi_refactor.txt; the argument order of K::row is part of that; the sides over S:
// profiles/r23_solve_multi_sides.txt).
template <class K, class T, int NT>
__device__ __forceinline__ void multi_tile_body(const typename K::Prob& p, int kc, double* red) {
  constexpr bool CX = sizeof(T) == 16;
  constexpr int RW = hs_multi_rows_per_wg_c(CX), NQ = CX ? 2 : 4;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int r0 = blockIdx.x * RW;
  constexpr int KCH = 4 * HSM_KS, ST = K::STEP;
  const bool full = K::full(p, r0);
  const int nch = (p.K + KCH - 1) / KCH;
  int cb, ce;
  if constexpr (K::MUL) {  // a triangular operand: the chunks [lo, hi) that meet the workgroup's rows, split over the waves like a whole K
    const int lo = K::lo(p, r0, nch), hi = K::hi(p, r0, nch), nc = max(hi - lo, 0);
    cb = lo + K::first(wv, nc);
    ce = lo + K::end(wv, nc);
  } else {
    cb = K::first(wv, nch);
    ce = K::end(wv, nch);
  }
  hs_d2u a0[2 * HSM_KS], a1[2 * HSM_KS];
  typename MultiX<T>::type x0[NT][HSM_KS], x1[NT][HSM_KS];
  if (cb < ce) K::template load<NT>(p, cb * KCH, r0, full, l15, l4, a0, x0);
  v4d acc[4][NT];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[q][ct] = v4d{0.0, 0.0, 0.0, 0.0};
  if (wv == 0 && K::cin(p)) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = K::row(r0, q, g, l4);
        if (row >= p.M) continue;
        const T* src;
        if constexpr (K::SPLITC) {
          if (p.C2 && row >= p.split)
            src = p.C2 + (long long)(row - p.split) * p.crs;
          else if (p.Cin)
            src = p.Cin + (long long)(p.cmap ? gld(p.cmap + row) : row) * p.crs;
          else
            continue;
        } else {
          src = p.Cin + (long long)(p.cmap ? gld(p.cmap + row) : row) * p.crs;
        }
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          const int col = ct * 16 + l15;
          if (col >= kc) continue;
          const T v = gld(src + col);
          if constexpr (CX) {
            acc[q][ct][g] = v.re;
            acc[2 + q][ct][g] = v.im;
          } else {
            acc[q][ct][g] = v;
          }
        }
      }
  }
  for (int ch = cb; ch < ce; ch += 2 * ST) {
    if (ch + ST < ce) K::template load<NT>(p, (ch + ST) * KCH, r0, full, l15, l4, a1, x1);
    K::template mfma<NT>(a0, x0, acc);
    if (ch + ST < ce) {
      if (ch + 2 * ST < ce) K::template load<NT>(p, (ch + 2 * ST) * KCH, r0, full, l15, l4, a0, x0);
      K::template mfma<NT>(a1, x1, acc);
    }
  }
  // (w0 + w2) + (w1 + w3)
  double* slot = red + (size_t)(wv & 1) * (16 * NT * 64);
  if (wv >= 2) multi_red_put<NT>(slot, lane, acc);
  __syncthreads();
  if (wv < 2) multi_red_add<NT>(slot, lane, acc);
  __syncthreads();
  if (wv == 1) multi_red_put<NT>(red, lane, acc);
  __syncthreads();
  if (wv != 0) return;
  multi_red_add<NT>(red, lane, acc);
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = K::row(r0, q, g, l4);
      if (row >= p.M) continue;
      T* dst;
      if constexpr (K::SPLITC)
        dst = (p.C2 && row >= p.split) ? p.C2 + (long long)(row - p.split) * p.crs : p.C + (long long)(p.cmap ? gld(p.cmap + row) : row) * p.crs;
      else
        dst = p.C + (long long)(p.cmap ? gld(p.cmap + row) : row) * p.crs;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const int col = ct * 16 + l15;
        if (col >= kc) continue;
        if constexpr (CX)
          gst(dst + col, cplx{acc[q][ct][g], acc[2 + q][ct][g]});
        else
          gst(dst + col, acc[q][ct][g]);
      }
    }
}

// host side: f(std::integral_constant<int, NT>) for NT = min(nt, 4) column tiles, the template argument of the kernels
template <class F>
inline void hs_with_nt(int nt, F f) {
  switch (nt) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
