// hs_block_apply.h -- the one place where a driver applies op(F)^-1 to a block of columns on the device, and where it asks beforehand
// what that application refuses.  Host code only; include it after hs_solver.h, hs_common.h and hs_host.h.
//
// The switch is per handle (hs_ulv_mode, include/hs_solver.h).  With mode 0, or on a handle without fronts that keep their interior block D
// as an HSS matrix, the router calls exactly the entry point the call site names with `via` -- what each driver called before there was a
// router, so its bits and its refusals are unchanged.  With mode 1 on a handle WITH such fronts every `via` becomes hs_ldiv_ulv_dev_*, the
// block solve that serves them for N, T and H (DESIGN.md 4d').  A handle without such fronts never changes its path, whatever its mode:
// that is what makes "mode 1 returns the bits of mode 0" hold there for the column-by-column drivers too.
#pragma once
#include <string>

enum HsApplyVia {
  HS_VIA_BLOCK = 0,  // hs_ldiv_block_dev_* (trans = 0 only): the lockstep drivers' forward block solve
  HS_VIA_BLOCK_T,    // hs_ldiv_block_dev_t_*
  HS_VIA_COLS,       // hs_ldiv_dev_*   (trans = 0 only): one single-vector solve per column
  HS_VIA_COLS_T,     // hs_ldiv_dev_t_*
};

// true: the handle's hs_ulv_mode is 1 and it has fronts with an HSS interior block (the only handles the switch reroutes)
inline bool hs_ulv_routed(hs_handle* F) { return hs_handle_ulv_routed(F) != 0; }

// C (n x nc, ldc) = op(F)^-1 B (n x nc, ldb) on `stream`; C == B solves in place.  Returns the status of the entry point it called.
template <class T>
int hs_block_apply_dev(hs_handle* F, HsApplyVia via, int trans, T* C, int64_t ldc, const T* B, int64_t ldb, int64_t n, int64_t nc, hipStream_t stream) {
  constexpr bool Z = sizeof(T) == 16;
  double* c = (double*)C;
  const double* b = (const double*)B;
  void* s = (void*)stream;
  if (hs_ulv_routed(F)) return Z ? hs_ldiv_ulv_dev_z(F, trans, c, ldc, b, ldb, n, nc, s) : hs_ldiv_ulv_dev_d(F, trans, c, ldc, b, ldb, n, nc, s);
  switch (via) {
    case HS_VIA_BLOCK: return Z ? hs_ldiv_block_dev_z(F, 0, c, ldc, b, ldb, n, nc, s) : hs_ldiv_block_dev_d(F, 0, c, ldc, b, ldb, n, nc, s);
    case HS_VIA_BLOCK_T: return Z ? hs_ldiv_block_dev_t_z(F, trans, c, ldc, b, ldb, n, nc, s) : hs_ldiv_block_dev_t_d(F, trans, c, ldc, b, ldb, n, nc, s);
    case HS_VIA_COLS: return Z ? hs_ldiv_dev_z(F, c, ldc, b, ldb, n, nc, s) : hs_ldiv_dev_d(F, c, ldc, b, ldb, n, nc, s);
    default: return Z ? hs_ldiv_dev_t_z(F, trans, c, ldc, b, ldb, n, nc, s) : hs_ldiv_dev_t_d(F, trans, c, ldc, b, ldb, n, nc, s);
  }
}

// The zero-column probe: the checks of the application above and nothing else -- what it refuses is refused here, with its words, before
// any device work.  Returns the status; hs_last_error holds the entry point's own message.
template <class T>
int hs_block_probe(hs_handle* F, HsApplyVia via, int trans) {
  const int64_t n = hs_size(F);
  return hs_block_apply_dev<T>(F, via, trans, (T*)nullptr, n, (const T*)nullptr, n, n, 0, nullptr);
}
// ... and reworded for the caller of `fn`: "<fn>: the block solve does not serve this <what> (<why>)<hint>", the status unchanged
template <class T>
void hs_block_probe_or_fail(hs_handle* F, HsApplyVia via, int trans, const char* fn, const char* what, const char* hint, bool unsupported_only) {
  const int st = hs_block_probe<T>(F, via, trans);
  if (st == HS_OK) return;
  if (unsupported_only && st != HS_ERR_UNSUPPORTED) throw st;
  const std::string why = hs_last_error();
  hs_set_error(st, hs_last_error_info(), "%s: the block solve does not serve this %s (%s)%s", fn, what, why.c_str(), hint);
  throw st;
}
