// hs_multi_kernels.h -- the kernels of the panel products of the block solves and their launches (declared in hs_solve_multi.h), written once
// over the work-block scalar T, the factor scalar S and the number of column tiles NT, and instantiated explicitly by the three files that
// include this header, each a translation unit of its own (the kernels sit at their register limit and keep their allocation only as long
// as nothing else is compiled into their functions, DESIGN.md section 4a⁗″):
//   kernels_solve_multi.hip      HS_MULTI_INST_FWD(T, T)              kernels_solve_multi_t.hip    HS_MULTI_INST_TR(T, T)
//   kernels_solve_multi_f32.hip  both, S = F32Of<T>::type            kernels_solve_multi_mul.hip  HS_MULTI_INST_MUL(T): the products of hs_mul_*
// level: one workgroup column per front of a tree level, the product resolved from the front's descriptor; prob: one given product (the
// low-rank transforms, the test hooks).
#pragma once
#include "hs_multi_fwd.h"
#include "hs_multi_tr.h"

template <class T, class S, int NT>
__global__ __launch_bounds__(256) void multi_level_kernel(const SolveNode<S>* __restrict__ nodes, int mode, int blk, MultiArgs a) {
  __shared__ double red[2 * 16 * NT * 64];
  const SolveNode<S> nd = nodes[blockIdx.y];
  MultiProb<T, S> p;
  if (!multi_resolve<T, S>(nd, a.aux[blockIdx.y], mode, blk, a, p)) return;
  if ((int)blockIdx.x * hs_multi_rows_per_wg_c(sizeof(T) == 16) >= p.M) return;
  multi_tile_body<MultiFwd<T, S>, T, NT>(p, a.kc, red);
}
template <class T, class S, int NT>
__global__ __launch_bounds__(256) void multi_prob_kernel(MultiProb<T, S> p, int kc) {
  __shared__ double red[2 * 16 * NT * 64];
  multi_tile_body<MultiFwd<T, S>, T, NT>(p, kc, red);
}
template <class T, class S, int NT>
__global__ __launch_bounds__(256) void multi_t_level_kernel(const SolveNode<S>* __restrict__ nodes, int mode, int blk, int conj, MultiArgs a) {
  __shared__ double red[2 * 16 * NT * 64];
  const SolveNode<S> nd = nodes[blockIdx.y];
  MultiProbT<T, S> p;
  if (!multi_t_resolve<T, S>(nd, a.aux[blockIdx.y], mode, blk, conj, a, p)) return;
  if ((int)blockIdx.x * hs_multi_rows_per_wg_c(sizeof(T) == 16) >= p.M) return;
  multi_tile_body<MultiTr<T, S>, T, NT>(p, a.kc, red);
}
template <class T, class S, int NT>
__global__ __launch_bounds__(256) void multi_t_prob_kernel(MultiProbT<T, S> p, int kc) {
  __shared__ double red[2 * 16 * NT * 64];
  multi_tile_body<MultiTr<T, S>, T, NT>(p, kc, red);
}

// launch(NT as an integral_constant, grid) for a product with M output rows in each of nfronts fronts; nothing when it is empty
template <class T, class Launch>
inline void multi_launch(int M, int nfronts, int kc, Launch launch) {
  if (nfronts <= 0 || M <= 0 || kc <= 0) return;
  constexpr int tr = hs_multi_rows_per_wg_c(sizeof(T) == 16);
  const dim3 grid((M + tr - 1) / tr, nfronts);
  hs_with_nt((kc + 15) / 16, [&](auto nt) { launch(nt, grid); });
}
template <class T, class S>
void launch_multi_level(const SolveNode<S>* sn, int nfronts, int mode, int blk, int maxM, const MultiArgs& a, hipStream_t s) {
  multi_launch<T>(maxM, nfronts, a.kc, [&](auto nt, dim3 grid) { hipLaunchKernelGGL((multi_level_kernel<T, S, decltype(nt)::value>), grid, dim3(256), 0, s, sn, mode, blk, a); });
}
template <class T, class S>
void launch_multi_prob(const MultiProb<T, S>& p, int kc, hipStream_t s) {
  multi_launch<T>(p.M, 1, kc, [&](auto nt, dim3 grid) { hipLaunchKernelGGL((multi_prob_kernel<T, S, decltype(nt)::value>), grid, dim3(256), 0, s, p, kc); });
}
template <class T, class S>
void launch_multi_level_t(const SolveNode<S>* sn, int nfronts, int mode, int blk, int conj, int maxM, const MultiArgs& a, hipStream_t s) {
  multi_launch<T>(maxM, nfronts, a.kc, [&](auto nt, dim3 grid) { hipLaunchKernelGGL((multi_t_level_kernel<T, S, decltype(nt)::value>), grid, dim3(256), 0, s, sn, mode, blk, conj, a); });
}
template <class T, class S>
void launch_multi_prob_t(const MultiProbT<T, S>& p, int kc, hipStream_t s) {
  multi_launch<T>(p.M, 1, kc, [&](auto nt, dim3 grid) { hipLaunchKernelGGL((multi_t_prob_kernel<T, S, decltype(nt)::value>), grid, dim3(256), 0, s, p, kc); });
}

// ---- the products of hs_mul_* (C = op(F) B): the same body over the MUL sides, S = T, a unit of their own (kernels_solve_multi_mul.hip) ----
template <class T, int NT>
__global__ __launch_bounds__(256) void mul_level_kernel(const SolveNode<T>* __restrict__ nodes, int mode, MultiArgs a) {
  __shared__ double red[2 * 16 * NT * 64];
  const SolveNode<T> nd = nodes[blockIdx.y];
  MultiProbMul<T, T> p;
  if (!mul_resolve<T>(nd, a.aux[blockIdx.y], mode, a, p)) return;
  if ((int)blockIdx.x * hs_multi_rows_per_wg_c(sizeof(T) == 16) >= p.M) return;
  multi_tile_body<MultiFwd<T, T, 1>, T, NT>(p, a.kc, red);
}
template <class T, int NT>
__global__ __launch_bounds__(256) void mul_prob_kernel(MultiProbMul<T, T> p, int kc) {
  __shared__ double red[2 * 16 * NT * 64];
  multi_tile_body<MultiFwd<T, T, 1>, T, NT>(p, kc, red);
}
template <class T, int NT>
__global__ __launch_bounds__(256) void mul_t_level_kernel(const SolveNode<T>* __restrict__ nodes, int mode, int conj, MultiArgs a) {
  __shared__ double red[2 * 16 * NT * 64];
  const SolveNode<T> nd = nodes[blockIdx.y];
  MultiProbMulT<T, T> p;
  if (!mul_t_resolve<T>(nd, a.aux[blockIdx.y], mode, conj, a, p)) return;
  if ((int)blockIdx.x * hs_multi_rows_per_wg_c(sizeof(T) == 16) >= p.M) return;
  multi_tile_body<MultiTr<T, T, 1>, T, NT>(p, a.kc, red);
}
template <class T, int NT>
__global__ __launch_bounds__(256) void mul_t_prob_kernel(MultiProbMulT<T, T> p, int kc) {
  __shared__ double red[2 * 16 * NT * 64];
  multi_tile_body<MultiTr<T, T, 1>, T, NT>(p, kc, red);
}
template <class T>
void launch_mul_level(const SolveNode<T>* sn, int nfronts, int mode, int maxM, const MultiArgs& a, hipStream_t s) {
  multi_launch<T>(maxM, nfronts, a.kc, [&](auto nt, dim3 grid) { hipLaunchKernelGGL((mul_level_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, sn, mode, a); });
}
template <class T>
void launch_mul_prob(const MultiProbMul<T, T>& p, int kc, hipStream_t s) {
  multi_launch<T>(p.M, 1, kc, [&](auto nt, dim3 grid) { hipLaunchKernelGGL((mul_prob_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, p, kc); });
}
template <class T>
void launch_mul_level_t(const SolveNode<T>* sn, int nfronts, int mode, int conj, int maxM, const MultiArgs& a, hipStream_t s) {
  multi_launch<T>(maxM, nfronts, a.kc, [&](auto nt, dim3 grid) { hipLaunchKernelGGL((mul_t_level_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, sn, mode, conj, a); });
}
template <class T>
void launch_mul_prob_t(const MultiProbMulT<T, T>& p, int kc, hipStream_t s) {
  multi_launch<T>(p.M, 1, kc, [&](auto nt, dim3 grid) { hipLaunchKernelGGL((mul_t_prob_kernel<T, decltype(nt)::value>), grid, dim3(256), 0, s, p, kc); });
}

#define HS_MULTI_INST_MUL(T)                                                                                      \
  template void launch_mul_level<T>(const SolveNode<T>*, int, int, int, const MultiArgs&, hipStream_t);         \
  template void launch_mul_prob<T>(const MultiProbMul<T, T>&, int, hipStream_t);                                 \
  template void launch_mul_level_t<T>(const SolveNode<T>*, int, int, int, int, const MultiArgs&, hipStream_t);  \
  template void launch_mul_prob_t<T>(const MultiProbMulT<T, T>&, int, hipStream_t);
#define HS_MULTI_INST_FWD(T, S)                                                                                    \
  template void launch_multi_level<T, S>(const SolveNode<S>*, int, int, int, int, const MultiArgs&, hipStream_t); \
  template void launch_multi_prob<T, S>(const MultiProb<T, S>&, int, hipStream_t);
#define HS_MULTI_INST_TR(T, S)                                                                                             \
  template void launch_multi_level_t<T, S>(const SolveNode<S>*, int, int, int, int, int, const MultiArgs&, hipStream_t);  \
  template void launch_multi_prob_t<T, S>(const MultiProbT<T, S>&, int, hipStream_t);
