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
// This file holds the forward kernels with the factors stored as T, and nothing else is compiled into them.  What is the forward product's
// own -- MultiFwd (which k a lane loads, the real MFMA chain, the strided split of K, the row map of the row-pair tiles) and multi_resolve
// (the solve descriptors) -- is hs_multi_fwd.h; the workgroup's body, the complex MFMA chain, the LDS exchange and the choice of NT are
// shared with the transposed product through hs_multi_tile.h; the kernels and launches are hs_multi_kernels.h.  The copy kernel
// multi_move_kernel, here, serves both directions and both factor scalars.
#include "hs_multi_kernels.h"

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

template <class T, class S>
void launch_multi_move(const SolveNode<S>* sn_s, int nfronts, int what, int maxrows, const MultiArgs& a, hipStream_t s, int perm_what) {
  if (nfronts <= 0 || maxrows <= 0 || a.kc <= 0) return;
  // the one place a SolveNode<S> is read as a SolveNode<T>: the kernel touches ni, woff, rperm and fidx only (static_assert: hs_solve_multi.h)
  const SolveNode<T>* sn = reinterpret_cast<const SolveNode<T>*>(sn_s);
  const dim3 grid((maxrows + 255) / 256, nfronts);
  if (perm_what == 0)
    hipLaunchKernelGGL((multi_move_kernel<T, 0>), grid, dim3(256), 0, s, sn, what, a);
  else
    hipLaunchKernelGGL((multi_move_kernel<T, 2>), grid, dim3(256), 0, s, sn, what, a);
}

#define INST(T, S)                                                                                                \
  HS_MULTI_INST_FWD(T, T)                                                                                         \
  template void launch_multi_move<T, T>(const SolveNode<T>*, int, int, int, const MultiArgs&, hipStream_t, int); \
  template void launch_multi_move<T, S>(const SolveNode<S>*, int, int, int, const MultiArgs&, hipStream_t, int);
INST(double, float)
INST(cplx, cplxf)
