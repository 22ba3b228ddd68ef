// kernels_solve_sparse.hip -- the data movement of hs_ldiv_sparse_* (hs_solve_sparse.hip): a chunk of sparse columns into a zero block, the
// wanted rows of the solved block out of it, the SolveNode entries of the active fronts into a compacted array, and zeros into the y
// segments of the fronts only the backward sweep visits.  The products of the sweeps are those of kernels_solve_multi(_t).hip, untouched.
// All four are plain memory kernels: every thread owns its destination (the rows of a CSC column are distinct, a compacted entry and a
// work-block row have one writer), so there are no atomics and nothing depends on the launch shape.
#include <algorithm>

#include "hs_solve_multi.h"

namespace {
constexpr int SPARSE_MAX_BLOCKS = 2048;  // grid-stride beyond: the lists are short next to the sweeps

// consecutive threads take consecutive stored entries (entries of one column are adjacent in the lists)
template <class T>
__global__ __launch_bounds__(256) void sparse_scatter_kernel(T* __restrict__ W, long long ldw, const T* __restrict__ val, const int* __restrict__ row,
                                                             const int* __restrict__ col, const long long* __restrict__ src, long long cnt) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < cnt; e += (long long)gridDim.x * 256)
    gst(W + gld(row + e) + (long long)gld(col + e) * ldw, gld(val + gld(src + e)));
}

// blockIdx.y = column of the chunk, consecutive threads take consecutive wanted rows: the stores of a wave are contiguous
template <class T>
__global__ __launch_bounds__(256) void sparse_gather_kernel(T* __restrict__ X, long long ldx, const long long* __restrict__ xcol, const T* __restrict__ W,
                                                            long long ldw, const int* __restrict__ rows, long long nrows) {
  const long long c = blockIdx.y;
  T* x = X + gld(xcol + c) * ldx;
  const T* w = W + c * ldw;
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < nrows; r += (long long)gridDim.x * 256)
    gst(x + r, gld(w + (rows ? (long long)gld(rows + r) : r)));
}

// one 8-byte word per thread: an entry is copied by consecutive lanes
template <int WORDS>
__global__ __launch_bounds__(256) void sparse_compact_kernel(unsigned long long* __restrict__ dst, const unsigned long long* __restrict__ src,
                                                             const long long* __restrict__ idx, long long cnt) {
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < cnt * WORDS; t += (long long)gridDim.x * 256) {
    const long long e = t / WORDS;
    const int w = (int)(t - e * WORDS);
    gst(dst + t, gld(src + gld(idx + e) * WORDS + w));
  }
}

// blockIdx.y = segment, one thread per row of it
template <class T>
__global__ __launch_bounds__(256) void sparse_zero_kernel(T* __restrict__ W2, int kcw, int kc, const HsZeroSeg* __restrict__ seg) {
  const long long woff = gld(&seg[blockIdx.y].woff);
  const int ni = gld(&seg[blockIdx.y].ni);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ni) return;
  T* w = W2 + (woff + i) * kcw;
  for (int c = 0; c < kc; ++c) gst(w + c, Scal<T>::zero());
}

int blocks_for(long long work) { return (int)std::min<long long>((work + 255) / 256, SPARSE_MAX_BLOCKS); }
}  // namespace

template <class T>
void launch_sparse_scatter(T* W, long long ldw, const T* val, const int* row, const int* col, const long long* src, long long cnt, hipStream_t s) {
  if (cnt <= 0) return;
  hipLaunchKernelGGL(sparse_scatter_kernel<T>, dim3(blocks_for(cnt)), dim3(256), 0, s, W, ldw, val, row, col, src, cnt);
}
template <class T>
void launch_sparse_gather(T* X, long long ldx, const long long* xcol, const T* W, long long ldw, const int* rows, long long nrows, int kc, hipStream_t s) {
  if (nrows <= 0 || kc <= 0) return;
  hipLaunchKernelGGL(sparse_gather_kernel<T>, dim3(blocks_for(nrows), kc), dim3(256), 0, s, X, ldx, xcol, W, ldw, rows, nrows);
}
template <class T>
void launch_sparse_compact(SolveNode<T>* dst, const SolveNode<T>* src, const long long* idx, long long cnt, hipStream_t s) {
  static_assert(sizeof(SolveNode<T>) % 8 == 0, "SolveNode is copied in 8-byte words");
  constexpr int WORDS = (int)(sizeof(SolveNode<T>) / 8);
  if (cnt <= 0) return;
  hipLaunchKernelGGL(sparse_compact_kernel<WORDS>, dim3(blocks_for(cnt * WORDS)), dim3(256), 0, s, (unsigned long long*)dst, (const unsigned long long*)src, idx, cnt);
}
template <class T>
void launch_sparse_zero(T* W2, int kcw, int kc, const HsZeroSeg* seg, int nseg, int maxni, hipStream_t s) {
  if (nseg <= 0 || maxni <= 0 || kc <= 0) return;
  hipLaunchKernelGGL(sparse_zero_kernel<T>, dim3((maxni + 255) / 256, nseg), dim3(256), 0, s, W2, kcw, kc, seg);
}

#define INST(T)                                                                                                                           \
  template void launch_sparse_scatter<T>(T*, long long, const T*, const int*, const int*, const long long*, long long, hipStream_t);     \
  template void launch_sparse_gather<T>(T*, long long, const long long*, const T*, long long, const int*, long long, int, hipStream_t); \
  template void launch_sparse_compact<T>(SolveNode<T>*, const SolveNode<T>*, const long long*, long long, hipStream_t);                 \
  template void launch_sparse_zero<T>(T*, int, int, const HsZeroSeg*, int, int, hipStream_t);
INST(double)
INST(cplx)
