// hs_sweep.h -- the sweeps of ldiv!, one tree level at a time: which launches a level's forward and backward sweep are made of, and in which
// order, for ldiv!(F, B), ldiv!(transpose(F), B) and ldiv!(adjoint(F), B) on each of the three paths.  The level loops of hs_api.hip
// (solve_fwd / solve_bwd) and the test hook hsk_sweep_level_* (hs_testhooks.hip) both call sweep_level_fwd / sweep_level_bwd, so what the
// hook's tests see is the production sequence.  The kernels: kernels_solve.hip, kernels_solve_wide.hip, kernels_solve_t.hip.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "hs_common.h"

// what the sweeps of one level work on
template <class T>
struct SweepLevel {
  const SolveNode<T>* dn;  // the level's solve descriptors
  int nfronts, maxni, maxnb, maxm;
  T *w1, *w2, *part;  // the work vectors (SolveNode::woff) and the partial sums of the interior update (SolveNode::poff)
  T* b;               // the global vector
  T *E1, *E2;         // exchange vectors of the dataflow sweeps, armed with the sentinel by the caller
  int* err;           // raised by a dataflow workgroup whose wait ran out
};

// The path of the sweeps, read once per process from HS_SOLVE_FLOW and HS_SOLVE_WIDE (nothing else reads them).  0: dataflow, one launch per
// level and sweep (the default).  1 (HS_SOLVE_FLOW=0): 256 columns per launch.  2 (HS_SOLVE_FLOW=0 HS_SOLVE_WIDE=0): 32 columns per launch;
// the transposed and adjoint sweeps have no 32-column kernels and take their 256-column steps on path 2 as well.
inline int hs_sweep_path() {
  static const int path = [] {
    const auto off = [](const char* name) { return getenv(name) && getenv(name)[0] == '0'; };
    return !off("HS_SOLVE_FLOW") ? 0 : !off("HS_SOLVE_WIDE") ? 1 : 2;
  }();
  return path;
}

// f(std::bool_constant<CONJ>): trans == 2 on ComplexF64 is the adjoint; Float64 has no adjoint instantiation (its adjoint is its transpose)
template <class T, class F>
static inline void sweep_with_conj(int trans, F&& f) {
  if constexpr (sizeof(T) == 16) {
    if (trans == 2) return f(std::true_type());
  }
  f(std::false_type());
}

// Forward sweep of a level: gather, then the triangular sweep with the update of rhs[bnd] (y, or z for trans != 0, is left in w2).
// counter: the workgroup-id counter of a dataflow launch, zero (path 0 only); force_tall: launch_fwd_flow
template <class T>
static void sweep_level_fwd(const SweepLevel<T>& L, int path, int trans, int* counter, hipStream_t s, int force_tall = -1) {
  launch_sweep_gather<T>(L.dn, L.nfronts, L.maxni, L.b, L.w1, trans == 0, s);
  if (trans != 0) {
    sweep_with_conj<T>(trans, [&](auto conj) {
      constexpr bool CONJ = decltype(conj)::value;
      if (path == 0) {
        launch_t_fwd_flow<T, CONJ>(L.dn, L.nfronts, L.maxni, L.maxnb, L.w1, L.w2, L.b, L.E1, L.E2, counter, L.err, s);
      } else {
        const int nblk = (L.maxni + hs_solve_t_cols() - 1) / hs_solve_t_cols();
        for (int blk = 0; blk < nblk; ++blk) launch_t_fwd_step<T, CONJ>(L.dn, L.nfronts, blk, L.maxm, L.w1, L.w2, L.b, s);
      }
    });
  } else if (path == 0) {  // the whole level in one launch
    launch_fwd_flow<T>(L.dn, L.nfronts, L.maxni, L.maxnb, L.w1, L.w2, L.b, L.E1, L.E2, counter, L.err, s, force_tall);
  } else if (path == 1) {
    const int nblk = (L.maxni + hs_solve_wide_cols() - 1) / hs_solve_wide_cols();
    for (int blk = 0; blk < nblk; ++blk) launch_fwd_wide<T>(L.dn, L.nfronts, blk, L.maxm, L.w1, L.w2, L.b, s);
  } else {
    const int nblk = (L.maxni + HS_PB - 1) / HS_PB;
    for (int blk = 0; blk < nblk; ++blk) launch_fwd_step<T>(L.dn, L.nfronts, blk, L.maxm, L.w1, L.w2, L.b, s);
  }
}

// Backward sweep of a level: the interior update w1 = y - Uib rhs[bnd] (trans != 0: v = z - Lbi^T rhs[bnd]), between() -- what else the
// caller subtracts from w1 (the low-rank Gauss transforms) --, the triangular sweep (x is left in w2), scatter.
template <class T, class Between>
static void sweep_level_bwd(const SweepLevel<T>& L, int path, int trans, int* counter, hipStream_t s, Between&& between) {
  if (trans != 0) {
    sweep_with_conj<T>(trans, [&](auto conj) {
      constexpr bool CONJ = decltype(conj)::value;
      launch_t_int_update<T, CONJ>(L.dn, L.nfronts, L.maxni, L.b, L.w2, L.w1, s);
      between();
      if (path == 0) {
        launch_t_bwd_flow<T, CONJ>(L.dn, L.nfronts, L.maxni, L.w1, L.w2, L.E1, L.E2, counter, L.err, s);
      } else {
        const int nblk = (L.maxni + hs_solve_t_cols() - 1) / hs_solve_t_cols();
        for (int blk = nblk - 1; blk >= 0; --blk) launch_t_bwd_step<T, CONJ>(L.dn, L.nfronts, blk, L.w1, L.w2, s);
      }
    });
  } else {
    launch_int_update<T>(L.dn, L.nfronts, L.maxni, L.maxnb, L.b, L.part, L.w2, L.w1, s);
    between();
    if (path == 0) {
      launch_bwd_flow<T>(L.dn, L.nfronts, L.maxni, L.w1, L.w2, L.E1, L.E2, counter, L.err, s);
    } else if (path == 1) {
      const int nblk = (L.maxni + hs_solve_wide_cols() - 1) / hs_solve_wide_cols();
      for (int blk = nblk - 1; blk >= 0; --blk) launch_bwd_wide<T>(L.dn, L.nfronts, blk, L.w1, L.w2, s, blk == nblk - 1);
    } else {
      const int nblk = (L.maxni + HS_PB - 1) / HS_PB;
      for (int blk = nblk - 1; blk >= 0; --blk) launch_bwd_step<T>(L.dn, L.nfronts, blk, L.w1, L.w2, s);
    }
  }
  launch_sweep_scatter<T>(L.dn, L.nfronts, L.maxni, L.b, L.w2, trans != 0, s);
}
template <class T>
static void sweep_level_bwd(const SweepLevel<T>& L, int path, int trans, int* counter, hipStream_t s) {
  sweep_level_bwd<T>(L, path, trans, counter, s, [] {});
}
