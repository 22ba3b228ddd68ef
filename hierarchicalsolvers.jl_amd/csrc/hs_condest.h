// hs_condest.h -- what the accuracy tools of hs_condest.hip (norm and condition estimates, refined solves) read from a factorization handle.
// hs_api.hip owns the handle; these two calls are the whole interface between the two files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct hs_handle;

struct HsHandleView {
  int64_t n = 0, nnz = 0;
  int is_complex = 0;
  int factored = 0;        // a numeric factorization is complete
  int device = 0;          // 0: a host-side plan only (hs_plan)
  int nranks = 1;
  int t_refused_node = -1; // first owned node whose transposed solve is refused (D kept as an HSS matrix: hss_d, mf = 2, 3); -1: none
  int64_t seed = 0;        // hs_options.seed
  const int64_t* colptr = nullptr;  // A in CSC on the device, 0-based; hs_numeric_begin keeps the values current
  const int32_t* rowval = nullptr;
  const void* nz = nullptr;
  const int64_t* rowptr = nullptr;  // hs_options.mf: the CSR pattern the matrix-free fronts already keep (CSR entry -> CSC entry in tperm); else null
  const int32_t* colind = nullptr;
  const int64_t* tperm = nullptr;
  hipStream_t stream = nullptr;     // the handle's own stream
  void** cx = nullptr;              // cache slot of hs_condest.hip (the CSR map of A), freed by hs_free through *cx_free
  void (**cx_free)(void*) = nullptr;
};

void hs_handle_view(hs_handle* h, HsHandleView* v);
// HS_OK, or HS_ERR_DEVICE with hs_last_error set when a dataflow sweep since the last check timed out (call after every synchronisation)
int hs_handle_flow_check(hs_handle* h);
