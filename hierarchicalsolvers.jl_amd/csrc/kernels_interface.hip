// kernels_interface.hip -- the device code of the Schur-complement mode (hs_interface.hip):
//
//   S[rperm[i], j] = sum over k <= min(i, j) of L(i, k) U(k, j),       L\U the packed pivoted LU of the pseudo-root (nb x nb, ld ldl),
//
// i.e. S = P^T (L U) rebuilt from the factors the handle keeps, and the two copies that park the block solve's intermediates in the caller's
// block between condense and expand.
//
// The product is a triangular one: element (i, j) has min(i, j) + 1 terms, so the whole of it is 2/3 nb^3 flops, not 2 nb^3.  A workgroup
// owns one 64 x 64 tile of the output and walks K in stages of 16 columns only up to kend = min(row end, column end) of its tile: beyond it
// either L(i, k) (k > i) or U(k, j) (k > j) is a structural zero for every element of the tile.  With N tiles per side the launch executes
// (1/3 + 1/(2N)) of the full product (+ the padding of kend to the stage).  Tiles are handed out heaviest first (the grid is walked from
// the bottom right corner).
//  * L and U share one packed array, so a stage is masked as it is loaded: L(i, k) = stored / 1 / 0 for k < / = / > i, U(k, j) = stored / 0
//    for k <= / > j; rows and columns past nb are zeros.  A masked element is never read, so no access leaves the nb x nb block, and no
//    masked copy of L or U exists anywhere: the packed array is only read.
//  * A stage is 64 x 16 of L and 16 x 64 of U, four elements of each per thread, loaded into registers while the MFMAs of the previous stage
//    run, then stored k-major into LDS (pitch 80 doubles: the four k-rows a wave reads for one MFMA operand fall into two disjoint halves of
//    the banks).  ComplexF64 keeps re and im in two planes and runs four real MFMAs per k-step, as the other complex kernels do.
//  * Wave w of the four owns the 32 x 32 quarter (w >> 1, w & 1): 2 x 2 MFMA tiles, 4 (complex: 8) accumulators of 4 doubles.  Operand
//    A: row = lane & 15, k = lane >> 4;  B: k = lane >> 4, column = lane & 15;  C/D: column = lane & 15, row = (lane >> 4) + 4 reg.
//  * Every element is one chain of MFMAs over ascending k in one wave: no atomics, no split of K, the same bits on every call.
//  * The row permutation is applied on the store.
// Registers / LDS (hipcc --save-temps, gfx950): DESIGN.md section 4k.
#include <algorithm>

#include "hs_interface.h"

typedef double v4d __attribute__((ext_vector_type(4)));

namespace {
constexpr int LT = 64;  // output tile
constexpr int LK = 16;  // columns of K per stage
constexpr int LP = 80;  // LDS pitch of a k-row (doubles)

template <class T>
struct Plane;
template <>
struct Plane<double> {
  static constexpr int N = 1;
  static __device__ __forceinline__ double get(double v, int) { return v; }
};
template <>
struct Plane<cplx> {
  static constexpr int N = 2;
  static __device__ __forceinline__ double get(cplx v, int p) { return p ? v.im : v.re; }
};

// thread t's four elements of the L stage (row t & 63, columns (t >> 6) + 4 e) and of the U stage (row t & 15, columns (t >> 4) + 16 e)
template <class T>
__device__ __forceinline__ void lu_stage_load(const T* __restrict__ LF, long long ldl, int nb, int r0, int c0, int kb, int t, T (&la)[4], T (&ua)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = r0 + (t & 63), k = kb + (t >> 6) + 4 * e;
    T v = Scal<T>::zero();
    if (i < nb) {
      if (k < i)
        v = gld(LF + i + (long long)k * ldl);
      else if (k == i)
        v = Scal<T>::one();
    }
    la[e] = v;
    const int kk = kb + (t & 15), j = c0 + (t >> 4) + 16 * e;
    T u = Scal<T>::zero();
    if (j < nb && kk <= j) u = gld(LF + kk + (long long)j * ldl);
    ua[e] = u;
  }
}

template <class T>
__global__ __launch_bounds__(256) void lu_product_kernel(int nb, const T* __restrict__ LF, long long ldl, const int* __restrict__ rperm, T* __restrict__ S,
                                                         long long lds) {
  constexpr int NP = Plane<T>::N;
  __shared__ double As[NP][LK][LP], Bs[NP][LK][LP];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int r0 = (int)(gridDim.y - 1 - blockIdx.y) * LT, c0 = (int)(gridDim.x - 1 - blockIdx.x) * LT;  // heaviest tiles first
  const int kend = min(min(r0 + LT, nb), min(c0 + LT, nb));
  const int nstage = (kend + LK - 1) / LK;
  const int wr = (w >> 1) * 32, wc = (w & 1) * 32;
  v4d acc[NP][2][2];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[p][m][n] = v4d{0.0, 0.0, 0.0, 0.0};
  T la[4], ua[4];
  lu_stage_load<T>(LF, ldl, nb, r0, c0, 0, t, la, ua);
  for (int st = 0; st < nstage; ++st) {
    __syncthreads();  // the MFMAs of the previous stage have read their operands
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        As[p][(t >> 6) + 4 * e][t & 63] = Plane<T>::get(la[e], p);
        Bs[p][t & 15][(t >> 4) + 16 * e] = Plane<T>::get(ua[e], p);
      }
    __syncthreads();
    if (st + 1 < nstage) lu_stage_load<T>(LF, ldl, nb, r0, c0, (st + 1) * LK, t, la, ua);  // in flight under the MFMAs below
#pragma unroll
    for (int ks = 0; ks < LK / 4; ++ks) {
      const int kr = 4 * ks + l4;
      double a[NP][2], b[NP][2];
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          a[p][m] = As[p][kr][wr + 16 * m + l15];
          b[p][m] = Bs[p][kr][wc + 16 * m + l15];
        }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          if constexpr (NP == 1) {
            acc[0][m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][m], b[0][n], acc[0][m][n], 0, 0, 0);
          } else {
            acc[0][m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][m], b[0][n], acc[0][m][n], 0, 0, 0);
            acc[0][m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[NP - 1][m], b[NP - 1][n], acc[0][m][n], 0, 0, 0);
            acc[NP - 1][m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][m], b[NP - 1][n], acc[NP - 1][m][n], 0, 0, 0);
            acc[NP - 1][m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[NP - 1][m], b[0][n], acc[NP - 1][m][n], 0, 0, 0);
          }
        }
    }
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = r0 + wr + 16 * m + l4 + 4 * g;
      if (i >= nb) continue;
      const long long ri = gld(rperm + i);
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int j = c0 + wc + 16 * n + l15;
        if (j >= nb) continue;
        T v;
        if constexpr (NP == 1)
          v = acc[0][m][n][g];
        else
          v = T{acc[0][m][n][g], acc[NP - 1][m][n][g]};
        gst(S + ri + (long long)j * lds, v);
      }
    }
}

// the y of every front of a level between work block 2 and the caller's block, at the front's own int ids (no permutation): exact copies
template <class T>
__global__ __launch_bounds__(256) void interface_park_kernel(const SolveNode<T>* __restrict__ nodes, int what, MultiArgs a) {
  const SolveNode<T> nd = nodes[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (nd.ni <= 0 || i >= nd.ni) return;
  T* b = (T*)a.B + gld(nd.fidx + i);
  T* w = (T*)a.W2 + (nd.woff + i) * a.kcw;
  if (what == 0)
    for (int c = 0; c < a.kc; ++c) gst(b + (long long)c * a.ldb, gld(w + c));
  else
    for (int c = 0; c < a.kc; ++c) gst(w + c, gld(b + (long long)c * a.ldb));
}
}  // namespace

static double lu_product_flops(int nb, bool is_complex) {
  const int nt = (nb + LT - 1) / LT;
  double f = 0.0;
  for (int r = 0; r < nt; ++r)
    for (int c = 0; c < nt; ++c) {
      const int kend = std::min(std::min((r + 1) * LT, nb), std::min((c + 1) * LT, nb));
      f += 2.0 * LT * LT * ((kend + LK - 1) / LK * LK);
    }
  return is_complex ? 4.0 * f : f;
}

template <class T>
double launch_lu_product(int nb, const T* LF, long long ldl, const int* rperm, T* S, long long lds, hipStream_t s) {
  if (nb <= 0) return 0.0;
  const int nt = (nb + LT - 1) / LT;
  hipLaunchKernelGGL((lu_product_kernel<T>), dim3(nt, nt), dim3(256), 0, s, nb, LF, ldl, rperm, S, lds);
  return lu_product_flops(nb, sizeof(T) == 16);
}
template <class T>
void launch_interface_park(const SolveNode<T>* sn, int nfronts, int what, int maxrows, const MultiArgs& a, hipStream_t s) {
  if (nfronts <= 0 || maxrows <= 0 || a.kc <= 0) return;
  hipLaunchKernelGGL((interface_park_kernel<T>), dim3((maxrows + 255) / 256, nfronts), dim3(256), 0, s, sn, what, a);
}

#define INST(T)                                                                                               \
  template double launch_lu_product<T>(int, const T*, long long, const int*, T*, long long, hipStream_t);   \
  template void launch_interface_park<T>(const SolveNode<T>*, int, int, int, const MultiArgs&, hipStream_t);
INST(double)
INST(cplx)
