// hs_f32.h -- a factorization demoted to Float32 storage (hs_f32_*, hs_f32.hip; include/hs_solver.h): the element types, the launch API of
// kernels_f32.hip (the demotion) and of kernels_solve_multi_f32.hip (the panel products of the block solve with the factor panel read as
// Float32 / ComplexF32 and everything else -- X, Cin, D, the accumulators -- as Float64 / ComplexF64), and what hs_solve_multi.hip,
// hs_gmres_block.hip and the test hooks see of the object.
//
// T is the element type of the work blocks (double, cplx), S = F32Of<T>::type that of the stored factors (float, cplxf).  A SolveNode<S> and
// a LowRank<S> have the layout of their <T> forms (pointers and integers only): the demoted object keeps arrays of them, filled with its
// own copies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hs_common.h"
#include "hs_lowrank.h"
#include "hs_solve_multi.h"

struct cplxf {
  float re, im;
};
template <class T>
struct F32Of;
template <>
struct F32Of<double> {
  typedef float type;
};
template <>
struct F32Of<cplx> {
  typedef cplxf type;
};
static_assert(sizeof(SolveNode<float>) == sizeof(SolveNode<double>) && sizeof(SolveNode<cplxf>) == sizeof(SolveNode<cplx>), "SolveNode<S> has the layout of SolveNode<T>");

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

// ---- kernels_solve_multi_f32.hip ---------------------------------------------------------------------------------------------------------
// MultiProb<T> / MultiProbT<T> (hs_solve_multi.h) with A stored as S
template <class T>
struct MultiProbF32 {
  const typename F32Of<T>::type* A;
  int lda, M, K;
  int trap;
  const T* X;
  long long xrs;
  const T* Cin;
  T* C;
  long long crs;
  const int* cmap;
};
template <class T>
struct MultiProbTF32 {
  const typename F32Of<T>::type* A;
  int lda, M, K;
  int trap;
  int conj;
  const T* X;
  long long xrs;
  const int* xmap;
  const T* Cin;
  T* C;
  long long crs;
  const int* cmap;
};
// the launches of hs_solve_multi.h over SolveNode<S>: the same modes (HSM_*, HSMT_*), grids and arguments
template <class T>
void launch_multi_level_f32(const SolveNode<typename F32Of<T>::type>* sn, int nfronts, int mode, int blk, int maxM, const MultiArgs& a, hipStream_t s);
template <class T>
void launch_multi_prob_f32(const MultiProbF32<T>& p, int kc, hipStream_t s);
template <class T>
void launch_multi_level_t_f32(const SolveNode<typename F32Of<T>::type>* sn, int nfronts, int mode, int blk, int conj, int maxM, const MultiArgs& a, hipStream_t s);
template <class T>
void launch_multi_prob_t_f32(const MultiProbTF32<T>& p, int kc, hipStream_t s);
// launch_multi_move<T> (kernels_solve_multi.hip, unchanged) on the descriptors of a demoted object: it reads ni, woff, rperm and fidx only
template <class T>
void launch_multi_move_f32(const SolveNode<typename F32Of<T>::type>* sn, int nfronts, int what, int maxrows, const MultiArgs& a, hipStream_t s, int perm_what);

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
