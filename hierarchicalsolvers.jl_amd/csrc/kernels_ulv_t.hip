// kernels_ulv_t.hip -- the one operation of the transposed / adjoint ULV solve of the HSS module (hs_hss_ldiv_t, hs_hss.hip), grouped:
//
//   C[M x N] = Cin - op(A)^T X[K x N]      or      C = op(A)^T X,        A stored K x M column-major, op = identity or conj,
//
// one launch for all the jobs of a tree level and step (blockIdx.z = job, as the grouped GEMM and row kernels of the module).  A is a block
// of the stored ULV factors read along its COLUMNS: T^T and T of a node's interpolation, UR = L^-1 P X_RS, the rows X_SR U^-1 below the LU
// in LF, a row panel of U or a column panel of L inside LF, a 32 x 32 inverse diagonal block (invU / invL).  Nothing transposed or
// conjugated is ever stored: the transpose is the operand map, the conjugation a sign flip while loading.
//
// A translation unit of its own: the kernels of kernels_solve_multi*.hip and kernels_gemm.hip sit at their register limits and keep
// their allocation only as long as nothing else is compiled next to them.
//
// Operand maps (v_mfma_f64_16x16x4_f64: A operand lane l holds [i = l & 15][k = l >> 4], B operand [k = l >> 4][j = l & 15], D holds
// [i = (l >> 4) + 4 reg][j = l & 15]).  X, Cin and C are COLUMN-major here (the module's blocks of right-hand sides), so the MFMA computes
// the transposed tile  D[n][m] = sum_k X[k, n] * op(A)[k, m]:
//  * MFMA A operand  = X[k, n0 + 16 ct + (l & 15)],   MFMA B operand = op(A)[k, m0 + (l & 15)],   both with k contiguous in memory;
//  * D[reg] of lane l is C[m0 + (l & 15), n0 + 16 ct + (l >> 4) + 4 reg]: the 16 lanes of a group store 16 consecutive rows of a column.
//  * The sum over k does not care which k a (group, k-step) pair holds as long as both operands agree, so a lane owns PAIRS of
//    consecutive k (Float64: k = kb + 2 (l >> 4) + {0, 1}, one 16-byte load per operand and pair of k-steps; ComplexF64: k = kb + (l >> 4),
//    one 16-byte element, re and im being the operands of the four real MFMAs of a complex product).
//  * A wave owns 16 rows of C (columns of A) and up to 64 columns, and walks ALL of K itself: no LDS, no barrier, no atomics, and the
//    summation order of an output element depends on K alone -- not on M, N, the job's place in the launch or the other jobs.
//  * Rows past M, columns past N and k past K are clamped for the address and zeroed in the operand, so nothing outside the blocks is read.
// Plain launches only: workgroups never wait for each other.  hsk_ulv_t_group_* (hs_testhooks.hip) checks the maps with exact integer
// data (tests/test_ulv_t_gpu.py).
#include "hs_multi_tile.h"  // v4d, hs_with_nt
#include "hs_ulv_t.h"

__device__ __forceinline__ bool ulv_t_keep(int tri, int k, int m) { return tri == HS_ULVT_FULL || (tri == HS_ULVT_LOWER ? k >= m : k <= m); }

template <int NT>
__device__ __forceinline__ void ulv_t_body(const UlvTJob<double>& j, int m0, int n0, int lane) {
  const int l15 = lane & 15, g = lane >> 4;
  const int m = m0 + l15;
  const double* ap = j.A + (size_t)min(m, j.M - 1) * j.lda;
  const double* xp[NT];
  v4d acc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    xp[ct] = j.X + (size_t)min(n0 + 16 * ct + l15, j.N - 1) * j.ldx;
    acc[ct] = v4d{0.0, 0.0, 0.0, 0.0};
  }
  const bool minus = j.Cin != nullptr;
  if (minus && m < j.M) {
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 16 * ct + g + 4 * r;
        if (n < j.N) acc[ct][r] = gld(j.Cin + (size_t)m + (size_t)n * j.ldcin);
      }
  }
  for (int kb = 0; kb < j.K; kb += 8) {
    const int k0 = kb + 2 * g, k1 = k0 + 1;
    const bool full = k1 < j.K;
    hs_d2u a;
    if (full) {
      a = gld2(ap + k0);
    } else {
      a.x = k0 < j.K ? gld(ap + k0) : 0.0;
      a.y = 0.0;
    }
    if (!ulv_t_keep(j.tri, k0, m)) a.x = 0.0;
    if (!ulv_t_keep(j.tri, k1, m)) a.y = 0.0;
    if (m >= j.M) a = hs_d2u{0.0, 0.0};
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      hs_d2u x;
      if (full) {
        x = gld2(xp[ct] + k0);
      } else {
        x.x = k0 < j.K ? gld(xp[ct] + k0) : 0.0;
        x.y = 0.0;
      }
      if (minus) x = -x;
      acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x.x, a.x, acc[ct], 0, 0, 0);
      acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x.y, a.y, acc[ct], 0, 0, 0);
    }
  }
  if (m >= j.M) return;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 16 * ct + g + 4 * r;
      if (n < j.N) gst(j.C + (size_t)m + (size_t)n * j.ldc, acc[ct][r]);
    }
}

template <int NT>
__device__ __forceinline__ void ulv_t_body(const UlvTJob<cplx>& j, int m0, int n0, int lane) {
  const int l15 = lane & 15, g = lane >> 4;
  const int m = m0 + l15;
  const cplx* ap = j.A + (size_t)min(m, j.M - 1) * j.lda;
  const cplx* xp[NT];
  v4d re[NT], im[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    xp[ct] = j.X + (size_t)min(n0 + 16 * ct + l15, j.N - 1) * j.ldx;
    re[ct] = v4d{0.0, 0.0, 0.0, 0.0};
    im[ct] = v4d{0.0, 0.0, 0.0, 0.0};
  }
  const bool minus = j.Cin != nullptr;
  if (minus && m < j.M) {
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 16 * ct + g + 4 * r;
        if (n < j.N) {
          const cplx v = gld(j.Cin + (size_t)m + (size_t)n * j.ldcin);
          re[ct][r] = v.re;
          im[ct][r] = v.im;
        }
      }
  }
  for (int kb = 0; kb < j.K; kb += 4) {
    const int k = kb + g;
    const bool in = k < j.K;
    hs_d2u a = gld2(ap + min(k, j.K - 1));
    if (j.conj) a.y = -a.y;
    if (!in || m >= j.M || !ulv_t_keep(j.tri, k, m)) a = hs_d2u{0.0, 0.0};
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      hs_d2u x = gld2(xp[ct] + min(k, j.K - 1));
      if (!in) x = hs_d2u{0.0, 0.0};
      if (minus) x = -x;
      re[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x.x, a.x, re[ct], 0, 0, 0);
      re[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(-x.y, a.y, re[ct], 0, 0, 0);
      im[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x.x, a.y, im[ct], 0, 0, 0);
      im[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(x.y, a.x, im[ct], 0, 0, 0);
    }
  }
  if (m >= j.M) return;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 16 * ct + g + 4 * r;
      if (n < j.N) gst(j.C + (size_t)m + (size_t)n * j.ldc, cplx{re[ct][r], im[ct][r]});
    }
}

// grid: (ceil(maxM / 64), ceil(maxN / (16 NT)), jobs); the four waves of a workgroup own four consecutive 16-row tiles
template <class T, int NT>
__global__ __launch_bounds__(256) void ulv_t_kernel(const UlvTJob<T>* __restrict__ jobs) {
  const UlvTJob<T> j = jobs[blockIdx.z];
  if (j.M <= 0 || j.K <= 0 || j.N <= 0) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int m0 = ((int)blockIdx.x * 4 + wv) * 16, n0 = (int)blockIdx.y * 16 * NT;
  if (m0 >= j.M || n0 >= j.N) return;  // (uniform over the wave; there is no barrier below)
  ulv_t_body<NT>(j, m0, n0, lane);
}

template <class T>
void launch_ulv_t(const UlvTJob<T>* djobs, int njobs, int maxM, int maxN, hipStream_t s) {
  if (njobs <= 0 || maxM <= 0 || maxN <= 0) return;
  const int nt = std::min(4, (maxN + 15) / 16);
  const dim3 grid((maxM + 63) / 64, (maxN + 16 * nt - 1) / (16 * nt), njobs);
  hs_with_nt(nt, [&](auto c) {
    hipLaunchKernelGGL((ulv_t_kernel<T, decltype(c)::value>), grid, dim3(256), 0, s, djobs);
  });
}

template <class T>
__global__ __launch_bounds__(256) void ulv_rows_kernel(const int* __restrict__ idx, int rows, int cols, const T* src, long long lds, T* dst, long long ldd, int mode) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const long long k = gld(idx + i);
  const int c0 = blockIdx.y * 8, c1 = min(c0 + 8, cols);
  for (int c = c0; c < c1; ++c) {
    if (mode == 0)
      gst(dst + i + c * ldd, gld(src + k + c * lds));
    else
      gst(dst + k + c * ldd, gld(src + i + c * lds));
  }
}
template <class T>
void launch_ulv_rows(const int* idx, int rows, int cols, const T* src, long long lds, T* dst, long long ldd, int mode, hipStream_t s) {
  if (rows <= 0 || cols <= 0) return;
  hipLaunchKernelGGL(ulv_rows_kernel<T>, dim3((rows + 255) / 256, (cols + 7) / 8), dim3(256), 0, s, idx, rows, cols, src, lds, dst, ldd, mode);
}
template void launch_ulv_rows<double>(const int*, int, int, const double*, long long, double*, long long, int, hipStream_t);
template void launch_ulv_rows<cplx>(const int*, int, int, const cplx*, long long, cplx*, long long, int, hipStream_t);

template void launch_ulv_t<double>(const UlvTJob<double>*, int, int, int, hipStream_t);
template void launch_ulv_t<cplx>(const UlvTJob<cplx>*, int, int, int, hipStream_t);
