// hs_gmres_op.hip -- the handle's own A for hs_gmres_t_* / hs_gmres_block_t_* (hs_gmres_op.h).  Host code only: the CSR map and the gather of
// its values are hs_condest.hip's (hs_ce::csr_of), the CSC arrays are the handle's.
#include <new>

#include "../../include/hs_solver.h"
#include "hs_common.h"
#define HS_CONDEST_KERNELS
#include "hs_condest.h"
#include "hs_gmres_op.h"

int hs_gmres_own_check(hs_handle* F, const char* fn, int ranks_only) {
  if (!F) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: null factorization handle", fn);
    return HS_ERR_ARGUMENT;
  }
  HsHandleView v;
  hs_handle_view(F, &v);
  if (v.nranks > 1) {
    hs_set_error(HS_ERR_UNSUPPORTED, 0, "%s: the handle's own A is not available on a factorization over %d ranks (single-rank factorizations only; pass A)", fn,
                 v.nranks);
    return HS_ERR_UNSUPPORTED;
  }
  if (ranks_only) return HS_OK;
  if (!v.factored) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: factorization is not complete (the handle's own A has the values of the last hs_numeric_begin)", fn);
    return HS_ERR_ARGUMENT;
  }
  if (!v.device || !v.colptr || !v.rowval || !v.nz) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: handle holds a host-side plan only (hs_plan); use hs_analyze", fn);
    return HS_ERR_ARGUMENT;
  }
  return HS_OK;
}

int hs_gmres_own_rows(hs_handle* F, int trans, hipStream_t s, HsGmresRows* out) {
  HS_GUARD(HsHandleView v; hs_handle_view(F, &v); if (trans == 0) {
    hs_ce::CsrMap* m = v.is_complex ? hs_ce::csr_of<cplx>(v, s) : hs_ce::csr_of<double>(v, s);
    out->ptr = m->rowptr;
    out->idx = m->colind;
    out->val = m->valr;
  } else {
    out->ptr = v.colptr;
    out->idx = v.rowval;
    out->val = v.nz;
  });
}
