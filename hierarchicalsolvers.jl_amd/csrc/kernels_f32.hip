// kernels_f32.hip -- the demotion of stored factor blocks to Float32 (hs_f32_create, hsk_round_factors_f32, hsk_multi_prob*_f32_*): one
// grouped launch over a job list, a job being one column-major block of real scalars (F32Job, hs_f32.h).
//
// A thread owns one ROW PAIR of its block and walks 64 columns: the 64 lanes of a wave read 1 KB of consecutive doubles of a column and
// store 512 consecutive bytes as float2 (the copies have an even leading dimension and an 8-byte aligned base: hs_f32_ld); the last row of
// an odd block is stored alone.  blockIdx.y is the job, blockIdx.z the group of 64 columns.  The conversion is v_cvt_f32_f64: round to
// nearest, ties to even, overflow to +-Inf, Float32 subnormals kept.  In place, the source receives (double)(float)x instead.
//
// Two counters, ordinary device atomics, one add per thread that has something to report:
//   [0] elements that are finite in Float64 and +-Inf in Float32      [1] nonzero elements that became zero or subnormal
// tests/f32_mirror.py states the rule in NumPy.
#include <cfloat>

#include "hs_f32.h"

typedef float hs_f2a __attribute__((ext_vector_type(2)));  // an aligned row pair of a demoted block

#define F32_COLS 64  // columns a thread walks

__device__ __forceinline__ float f32_demote(double x, unsigned& over, unsigned& flush) {
  const float f = (float)x;
  if (isfinite(x) && isinf(f)) ++over;
  if (x != 0.0 && fabsf(f) < FLT_MIN) ++flush;
  return f;
}

template <bool INPLACE>
__global__ __launch_bounds__(256) void f32_demote_kernel(const F32Job* __restrict__ jobs, unsigned long long* counts) {
  const F32Job jb = jobs[blockIdx.y];
  const int r = 2 * (blockIdx.x * 256 + threadIdx.x);
  const int c0 = blockIdx.z * F32_COLS;
  if (r >= jb.rows || c0 >= jb.cols) return;
  const int c1 = min(jb.cols, c0 + F32_COLS);
  const bool pair = r + 1 < jb.rows;
  unsigned over = 0, flush = 0;
  for (int c = c0; c < c1; ++c) {
    const double* sp = jb.src + (long long)c * jb.lds + r;
    const double x0 = gld(sp);
    const double x1 = pair ? gld(sp + 1) : 0.0;
    const float f0 = f32_demote(x0, over, flush);
    const float f1 = f32_demote(x1, over, flush);
    if constexpr (INPLACE) {
      double* dp = (double*)jb.dst + (long long)c * jb.lds + r;
      gst(dp, (double)f0);
      if (pair) gst(dp + 1, (double)f1);
    } else {
      float* dp = (float*)jb.dst + (long long)c * jb.ldd + r;
      if (pair)
        *(hs_f2a HS_AS_GLOBAL*)dp = hs_f2a{f0, f1};
      else
        gst(dp, f0);
    }
  }
  if (over) atomicAdd(counts, (unsigned long long)over);
  if (flush) atomicAdd(counts + 1, (unsigned long long)flush);
}

__global__ __launch_bounds__(256) void f32_copy_int_kernel(const F32IntJob* __restrict__ jobs) {
  const F32IntJob jb = jobs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < jb.count) gst(jb.dst + i, gld(jb.src + i));
}

void launch_f32_demote(const F32Job* jobs, int njobs, int maxrows, int maxcols, bool inplace, unsigned long long* counts, hipStream_t s) {
  if (njobs <= 0 || maxrows <= 0 || maxcols <= 0) return;
  const unsigned gx = (unsigned)(((maxrows + 1) / 2 + 255) / 256), gz = (unsigned)((maxcols + F32_COLS - 1) / F32_COLS);
  for (int j0 = 0; j0 < njobs; j0 += 32768) {
    const dim3 grid(gx, (unsigned)std::min(32768, njobs - j0), gz);
    if (inplace)
      hipLaunchKernelGGL(f32_demote_kernel<true>, grid, dim3(256), 0, s, jobs + j0, counts);
    else
      hipLaunchKernelGGL(f32_demote_kernel<false>, grid, dim3(256), 0, s, jobs + j0, counts);
  }
}
void launch_f32_copy_int(const F32IntJob* jobs, int njobs, int maxcount, hipStream_t s) {
  if (njobs <= 0 || maxcount <= 0) return;
  for (int j0 = 0; j0 < njobs; j0 += 32768) {
    const dim3 grid((unsigned)((maxcount + 255) / 256), (unsigned)std::min(32768, njobs - j0));
    hipLaunchKernelGGL(f32_copy_int_kernel, grid, dim3(256), 0, s, jobs + j0);
  }
}
