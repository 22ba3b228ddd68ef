// hs_gmres_op.h -- the handle's own A as the GMRES driver reads it (hs_gmres_t_*, hs_gmres_block_t_* with colptr = rowval = nzval = NULL).
// Plain declarations: hs_gmres_block.hip does not include hs_condest.h, whose kernel section switches floating-point
// contraction off for the rest of the including file; hs_gmres_op.hip is the one translation unit that reaches hs_ce::csr_of for it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct hs_handle;

// rows of op(A) as entry ranges ptr[i] .. ptr[i + 1] of (idx, val), 0-based, on the device, owned by the handle
struct HsGmresRows {
  const int64_t* ptr = nullptr;
  const int32_t* idx = nullptr;
  const void* val = nullptr;
};

// Host-only checks of an own-A call, before any device work: HS_OK, or the status with hs_last_error set -- HS_ERR_UNSUPPORTED for a handle
// over more than one rank, then (ranks_only == 0) HS_ERR_ARGUMENT for a handle without a completed numeric factorization.  The drivers ask for
// the ranks first, then let the solve name what it refuses, then ask for the rest.
int hs_gmres_own_check(hs_handle* F, const char* fn, int ranks_only);
// trans = 0: the CSR map of A kept in the handle (hs_ce::csr_of: built on first use, rows in column order), its values gathered on `s` from
// the CSC values of the last hs_numeric_begin.  trans = 1, 2: the handle's CSC arrays themselves.
int hs_gmres_own_rows(hs_handle* F, int trans, hipStream_t s, HsGmresRows* out);
