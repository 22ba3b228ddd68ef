// hs_f32.h -- a factorization demoted to Float32 storage (hs_f32_*, hs_f32.hip; include/hs_solver.h): the launch API of kernels_f32.hip
// (the demotion), and what hs_solve_multi.hip, hs_gmres_block.hip and the test hooks see of the object.  The element types (cplxf,
// F32Of<T>) and the panel products over a Float32 / ComplexF32 panel are those of hs_solve_multi.h with S = F32Of<T>::type: the demoted
// object keeps arrays of SolveNode<S> and LowRank<S>, filled with its own copies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hs_common.h"
#include "hs_lowrank.h"
#include "hs_solve_multi.h"

// ---- kernels_f32.hip: the demotion ------------------------------------------------------------------------------------------------------
// One block of REAL scalars (a ComplexF64 block is one of twice as many rows): rows x cols, column-major.  dst is Float32 with ld ldd (even,
// dst 8-byte aligned: rows are stored in pairs), or -- inplace -- the source itself, which then receives (double)(float)x.
struct F32Job {
  const double* src;
  void* dst;
  long long lds, ldd;
  int rows, cols;
};
// x -> (float)x, round to nearest even, for every element of every job (jobs: device array); one grouped launch per 32768 jobs.
// counts (device, two entries, added to): [0] elements finite in Float64 that overflow Float32, [1] nonzero elements that become zero or
// subnormal.  maxrows / maxcols: the largest of the jobs.
void launch_f32_demote(const F32Job* jobs, int njobs, int maxrows, int maxcols, bool inplace, unsigned long long* counts, hipStream_t s);
struct F32IntJob {
  const int* src;
  int* dst;
  int count, pad;
};
void launch_f32_copy_int(const F32IntJob* jobs, int njobs, int maxcount, hipStream_t s);

// ---- hs_solve_multi.hip --------------------------------------------------------------------------------------------------------------------
// hs_solve_multi_run on a view whose descriptors (HsMultiLevel::sn, HsMultiLR::lrL / lrR) are SolveNode<S> / LowRank<S>: the same schedule,
// chunks, work blocks and summation orders; no active set and no phases
template <class T>
void hs_solve_multi_run_f32(const HsMultiView& v, int trans, T* dC, int64_t ldc, int64_t nrhs, hipStream_t s);

// ---- hs_f32.hip, as hs_gmres_block.hip and hs_testhooks.hip see it -------------------------------------------------------------------------
struct hs_f32;
struct hs_handle;
// hs_f32_ldiv_dev_d or _z by the element type of the object (device blocks, queued on s); returns its status
int hs_f32_apply_prec(hs_f32* G, int trans, void* dC, int64_t ldc, const void* dB, int64_t ldb, int64_t n, int64_t nrhs, hipStream_t s);
int64_t hs_f32_size(const hs_f32* G);
int hs_f32_is_complex(const hs_f32* G);
// rounds every element hs_f32_create would demote through Float32, in place in the handle (hsk_round_factors_f32); throws (hs_host.h)
void hs_f32_round_in_place(hs_handle* F, int64_t* counts2);
// the leading dimension of a demoted copy of a block with `rows` rows: even, so that a row pair is one aligned 8-byte word
inline long long hs_f32_ld(long long rows) { return (std::max<long long>(rows, 1) + 1) / 2 * 2; }
