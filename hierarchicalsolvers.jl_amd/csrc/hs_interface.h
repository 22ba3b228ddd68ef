// hs_interface.h -- Schur-complement mode (hs_interface_*): what hs_interface.hip reads from a factorization handle and the launch API of
// kernels_interface.hip.  hs_api.hip owns the handle; hs_interface_view, hs_multi_view (hs_solve_multi.h) and the two scratch calls of
// hs_selinv.h are the whole interface between the files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_common.h"
#include "hs_solve_multi.h"

struct hs_handle;

enum {
  HS_IF_SLICED = 1,  // the pseudo-root is one slice of a front eliminated in slices (hs_options.split)
  HS_IF_NOLU = 2,    // it does not keep one dense pivoted LU of its interior block
};

struct HsInterfaceView {
  int64_t n = 0;
  int is_complex = 0, factored = 0, device = 0, nranks = 1;
  int hss_node = -1;          // the first front that keeps its interior block D as an HSS matrix, -1: none
  int64_t nb = 0;             // |root.bnd|: the interior of the pseudo-root (0: the root keeps no boundary)
  const int* idx = nullptr;   // its nb global ids (0-based, host), in the order of S's rows and columns
  int flags = 0;              // HS_IF_*
  const void* LU = nullptr;   // the pseudo-root's packed L\U (nb x nb, ld ldlu, device)
  int ldlu = 0;
  const int* rperm = nullptr; // (P x)[i] = x[rperm[i]] (device)
  hipStream_t stream = nullptr;
  void** ix = nullptr;        // cache slot of hs_interface.hip (events, the last calls' figures), freed by hs_free through *ix_free
  void (**ix_free)(void*) = nullptr;
};
void hs_interface_view(hs_handle* h, HsInterfaceView* v);
int hs_handle_flow_check(hs_handle* h);  // HS_OK, or the error a sweep workgroup of an earlier solve raised (hs_api.hip)

// ---- kernels_interface.hip ------------------------------------------------------------------------------------------------------------
// S[rperm[i], j] = sum over k <= min(i, j) of L(i, k) U(k, j) from the packed L\U (nb x nb, ld ldl, unit lower L): v_mfma_f64_16x16x4_f64 over
// 64 x 64 output tiles, each walking K up to its own min(row end, column end), the triangles masked as the tiles are staged; one ascending-k
// chain per element.  Returns the real flops the launch executes (K padded to the 16-column stage).
template <class T>
double launch_lu_product(int nb, const T* LF, long long ldl, const int* rperm, T* S, long long lds, hipStream_t s);
// the intermediates of the block solve between the phases, for every front of a level (the grid of launch_multi_move), unpermuted:
//   what = 0: B[int, :] = W2     1: W2 = B[int, :]
template <class T>
void launch_interface_park(const SolveNode<T>* sn, int nfronts, int what, int maxrows, const MultiArgs& a, hipStream_t s);
