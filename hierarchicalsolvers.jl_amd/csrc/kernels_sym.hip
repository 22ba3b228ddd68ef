// kernels_sym.hip -- device code of the symmetric mode (hs_options.symmetric, Sched::sym): the batched transposition that rebuilds upper
// blocks of a front from its lower ones, and the check of A == transpose(A) on the stored entries.
#include "hs_common.h"

// ------------------------------------------------------------------------------------------------
// sym_transpose: mat[c0:c1, r0:r1) <- transpose(mat[r0:r1, c0:c1)) inside the square part of LF (the interior) or SB, one workgroup per
// 32 x 32 tile of the source and front.  The tile goes through LDS with rows padded by one element (8- and 16-byte accesses: the lanes of
// a 32-lane group then read LDS addresses 33 elements apart, which fall on distinct banks), so the global read and the global write are
// both contiguous along a column of the column-major blocks.  lower: the range is a diagonal square; tiles above the diagonal do nothing,
// a diagonal tile is read whole before its strictly upper part is written (the barrier in between), so it cannot race with itself.
// ------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void sym_transpose_kernel(const NodeDesc<T>* __restrict__ nodes, int mat, int r0, int r1, int c0, int c1, int lower,
                                                            int tiles_r) {
  T* p;
  int ld, rows, cols;
  mat_of(nodes + blockIdx.y, mat, p, ld, rows, cols);
  const int lim = min(rows, cols);  // LF: ni (the interior square), SB: nb
  r1 = min(r1, lim);
  c1 = min(c1, lim);
  const int ti = blockIdx.x % tiles_r, tj = blockIdx.x / tiles_r;
  const int sr = r0 + 32 * ti, sc = c0 + 32 * tj;  // first row / column of the source tile
  if (sr >= r1 || sc >= c1 || (lower && ti < tj)) return;  // workgroup-uniform
  __shared__ T tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cl = ty + 8 * k;
    if (sr + tx < r1 && sc + cl < c1) tile[cl][tx] = gld(p + (size_t)(sc + cl) * ld + sr + tx);
  }
  __syncthreads();
  // destination (sc + tx, sr + rl) = source (sr + rl, sc + tx)
  const bool diag = lower && ti == tj;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rl = ty + 8 * k;
    if (sc + tx < c1 && sr + rl < r1 && (!diag || tx < rl)) gst(p + (size_t)(sr + rl) * ld + sc + tx, tile[tx][rl]);
  }
}

template <class T>
void launch_sym_transpose(const NodeDesc<T>* dnodes, int nbatch, int mat, int r0, int r1, int c0, int c1, int lower, int maxrows, int maxcols, hipStream_t s) {
  if (nbatch <= 0 || maxrows <= 0 || maxcols <= 0 || mat == HS_MAT_UR) return;
  const int tr = (maxrows + 31) / 32, tc = (maxcols + 31) / 32;
  dim3 grid((unsigned)((long long)tr * tc), nbatch);
  hipLaunchKernelGGL(sym_transpose_kernel<T>, grid, dim3(256), 0, s, dnodes, mat, r0, r1, c0, c1, lower, tr);
}

// ------------------------------------------------------------------------------------------------
// sym_check: one thread per column c; every entry (r, c) looks its partner (c, r) up in column r (any row order) and compares the bits.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }
__device__ __forceinline__ bool same_bits(cplx a, cplx b) { return same_bits(a.re, b.re) && same_bits(a.im, b.im); }

template <class T>
__global__ __launch_bounds__(256) void sym_check_kernel(int64_t n, const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                                        const T* __restrict__ nz, unsigned long long* __restrict__ first) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  for (int64_t e = colptr[c]; e < colptr[c + 1]; ++e) {
    const int64_t r = rowval[e];
    if (r == c) continue;
    bool ok = false;
    for (int64_t f = colptr[r]; f < colptr[r + 1]; ++f)
      if (rowval[f] == c) {
        ok = same_bits(gld(nz + e), gld(nz + f));
        break;
      }
    if (!ok) {
      atomicMin(first, (unsigned long long)e);
      return;  // (the entries of a column come in increasing e)
    }
  }
}

template <class T>
void launch_sym_check(int64_t n, const int64_t* colptr, const int32_t* rowval, const T* nz, unsigned long long* first, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(sym_check_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, colptr, rowval, nz, first);
}

#define HS_INST(T)                                                                                                              \
  template void launch_sym_transpose<T>(const NodeDesc<T>*, int, int, int, int, int, int, int, int, int, hipStream_t);          \
  template void launch_sym_check<T>(int64_t, const int64_t*, const int32_t*, const T*, unsigned long long*, hipStream_t);
HS_INST(double)
HS_INST(cplx)
#undef HS_INST
