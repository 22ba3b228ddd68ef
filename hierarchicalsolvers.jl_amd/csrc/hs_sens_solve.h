// hs_sens_solve.h -- what the two column-group drivers over the stored factorization share (hs_sens.hip: hs_sens_*, hs_misfit_*; hs_gn.hip:
// hs_tangent_*, hs_gn_hessvec_*, hs_gn_diag_*): the block argument, the choice among the library's own solves for one group of columns with
// its staging, the group width, the receiver rows as a sparse cotangent, and the refusals both word alike.  Host code only, internal
// linkage; include it after hs_solver.h, hs_common.h, hs_host.h, hs_block_apply.h, hs_solve_multi.h and hs_sens.h.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>

namespace {

template <class T>
struct Blk {  // an n x nrhs block: the values on the device, the index arrays on the host
  const T* dense = nullptr;
  int64_t ld = 0;
  const int64_t* colptr = nullptr;
  const int64_t* rowval = nullptr;
  const T* nzval = nullptr;
  bool sparse() const { return !dense; }
  int64_t nnz(int64_t c0, int64_t c1) const { return colptr[c1] - colptr[c0]; }
};

// the block application of op(F)^-1 (hs_block_apply.h).  ulv: the driver serves handles whose hs_ulv_mode reroutes it (hs_sens.hip); a
// driver that does not (hs_gn.hip) keeps hs_ldiv_block_dev_t_* and its refusals in either mode
template <class T>
int block_solve(hs_handle* F, bool ulv, int t, T* C, int64_t ldc, const T* B, int64_t ldb, int64_t n, int64_t nc, hipStream_t s) {
  if (ulv) return hs_block_apply_dev<T>(F, HS_VIA_BLOCK_T, t, C, ldc, B, ldb, n, nc, s);
  if (sizeof(T) == 16) return hs_ldiv_block_dev_t_z(F, t, (double*)C, ldc, (const double*)B, ldb, n, nc, (void*)s);
  return hs_ldiv_block_dev_t_d(F, t, (double*)C, ldc, (const double*)B, ldb, n, nc, (void*)s);
}
template <class T>
int sparse_solve(hs_handle* F, int t, int64_t n, int64_t nc, const int64_t* cp, const int64_t* rv, const T* dv, T* X, int64_t ldx, hipStream_t s) {
  if (sizeof(T) == 16) return hs_ldiv_sparse_dev_z(F, t, n, nc, cp, rv, (const double*)dv, nullptr, 0, (double*)X, ldx, (void*)s);
  return hs_ldiv_sparse_dev_d(F, t, n, nc, cp, rv, (const double*)dv, nullptr, 0, (double*)X, ldx, (void*)s);
}
template <class T>
int refine_solve(hs_handle* F, int t, T* X, int64_t ldx, const T* B, int64_t ldb, int64_t n, int64_t nc, int64_t itmax, double* berr, int64_t* steps, hipStream_t s) {
  if (sizeof(T) == 16) return hs_ldiv_refine_block_dev_z(F, t, (double*)X, ldx, (const double*)B, ldb, n, nc, itmax, berr, nullptr, steps, (void*)s);
  return hs_ldiv_refine_block_dev_d(F, t, (double*)X, ldx, (const double*)B, ldb, n, nc, itmax, berr, nullptr, steps, (void*)s);
}

// Gc: the widest group (a multiple of the block solve's chunk width) whose blocks fit half of the free memory; `env` overrides
inline int64_t group_width(size_t per_col, int64_t nrhs, const char* env, const char* fn) {
  const int64_t KC = hs_ldiv_block_cols();
  const int64_t all = std::min<int64_t>((nrhs + KC - 1) / KC * KC, 4096);
  if (const char* e = getenv(env)) {
    const long long w = atoll(e);
    if (w > 0) return std::min<int64_t>(all, (w + KC - 1) / KC * KC);
  }
  size_t fr = 0, tot = 0;
  HS_HIP(hipMemGetInfo(&fr, &tot));
  const int64_t fit = (int64_t)(fr / 2 / per_col);
  if (fit >= all) return all;
  const int64_t least = std::min<int64_t>(KC, nrhs);
  if (fit < least)
    HS_FAIL(HS_ERR_NOMEM, 0, "OutOfMemoryError: %s needs %zu bytes for one group of %lld columns, half of the free device memory is %zu bytes", fn,
            per_col * (size_t)least, (long long)least, fr / 2);
  return std::max<int64_t>(fit / KC * KC, least);
}

// One group of columns through one of the library's own entry points: hs_ldiv_block_dev_t_* (dense blocks), hs_ldiv_sparse_dev_* with all
// rows (sparse blocks: the pruned forward sweep), hs_ldiv_refine_block_dev_* (itmax > 0; a sparse block is expanded on the device first).
// The driver sets F, n, itmax, s and the work blocks its calls can reach.
template <class T>
struct HsGroupSolve {
  hs_handle* F = nullptr;
  int64_t n = 0, itmax = 0;
  hipStream_t s = nullptr;
  bool ulv = false;         // the handle's hs_ulv_mode reroutes this driver (HsHandleView::ulv): block_solve above, sparse blocks expanded
  T* stage = nullptr;       // n x Gc: the dense right-hand side of a refined solve that is not the caller's block as it stands
  T* vstage = nullptr;      // conjugated values of a sparse block (itmax = 0)
  int32_t* d_er = nullptr;  // entries of a sparse group for the expansion (itmax > 0)
  int32_t* d_ec = nullptr;
  int64_t solves = 0;       // calls issued
  std::vector<int64_t> cp;  // rebased column pointers of a sparse group
  std::vector<int32_t> er, ec;
  std::vector<double> berr;
  std::vector<int64_t> steps;

  // out (n x gc, ld n) = op_t(F)^-1 S, S = columns [g0, g0 + gc) of b, conjugated when cjin
  void solve(int t, const Blk<T>& b, int64_t g0, int gc, bool cjin, T* out) {
    ++solves;
    const int64_t off = b.sparse() ? b.colptr[g0] - 1 : 0, cnt = b.sparse() ? b.nnz(g0, g0 + gc) : 0;
    if (b.sparse()) {
      cp.resize((size_t)gc + 1);
      for (int j = 0; j <= gc; ++j) cp[(size_t)j] = b.colptr[g0 + j] - off;
    }
    if (itmax == 0 && !(ulv && b.sparse())) {
      if (!b.sparse()) {
        const T* src = b.dense + (size_t)g0 * b.ld;
        if (cjin) {
          launch_sens_copy<T>(out, n, src, b.ld, n, gc, 1, s);
          HS_CHECK(block_solve<T>(F, ulv, t, out, n, out, n, n, gc, s));
        } else {
          HS_CHECK(block_solve<T>(F, ulv, t, out, n, src, b.ld, n, gc, s));
        }
        return;
      }
      const T* val = b.nzval + off;
      if (cjin && cnt > 0) {
        launch_sens_copy<T>(vstage, cnt, val, cnt, cnt, 1, 1, s);
        val = vstage;
      }
      HS_CHECK(sparse_solve<T>(F, t, n, gc, cp.data(), b.rowval + off, val, out, n, s));
      return;
    }
    const T* src;
    int64_t lds;
    if (!b.sparse() && !cjin) {
      src = b.dense + (size_t)g0 * b.ld;
      lds = b.ld;
    } else {
      src = stage;
      lds = n;
      if (!b.sparse()) {
        launch_sens_copy<T>(stage, n, b.dense + (size_t)g0 * b.ld, b.ld, n, gc, 1, s);
      } else {
        HS_HIP(hipMemsetAsync(stage, 0, (size_t)n * gc * sizeof(T), s));
        if (cnt > 0) {
          er.resize((size_t)cnt);
          ec.resize((size_t)cnt);
          for (int j = 0; j < gc; ++j)
            for (int64_t e = cp[(size_t)j] - 1; e < cp[(size_t)j + 1] - 1; ++e) {
              er[(size_t)e] = (int32_t)(b.rowval[off + e] - 1);
              ec[(size_t)e] = j;
            }
          HS_HIP(hipStreamSynchronize(s));  // the lists of the previous expansion are no longer read
          HS_HIP(hipMemcpy(d_er, er.data(), (size_t)cnt * sizeof(int32_t), hipMemcpyHostToDevice));
          HS_HIP(hipMemcpy(d_ec, ec.data(), (size_t)cnt * sizeof(int32_t), hipMemcpyHostToDevice));
          launch_sens_expand<T>(stage, n, d_er, d_ec, b.nzval + off, cnt, cjin ? 1 : 0, s);
        }
      }
    }
    if (itmax == 0) {  // (ulv: a sparse block of the driver's own, expanded above -- the pruned sweeps run no HSS hook)
      HS_CHECK(block_solve<T>(F, ulv, t, out, n, src, lds, n, gc, s));
      return;
    }
    berr.resize((size_t)gc);
    steps.resize((size_t)gc);
    HS_CHECK(refine_solve<T>(F, t, out, n, src, lds, n, gc, itmax, berr.data(), steps.data(), s));
  }
};

// Distinct receiver rows as the pattern of a sparse cotangent of Gc columns: the wanted rows in the caller's order (0-based), their slot in
// ascending order, the values (nrows per column, rows ascending) and the host index arrays
template <class T>
struct HsReceiverRows {
  int32_t* d_rows = nullptr;
  int32_t* d_slot = nullptr;
  T* Wv = nullptr;
  std::vector<int64_t> wcp, wrv;
  Blk<T> W;

  // returns the bytes of the two index lists
  size_t setup(const int64_t* rows, int64_t nr, int64_t Gc, HsDevBuf& buf) {
    std::vector<int32_t> r0((size_t)nr), slot((size_t)nr), ord((size_t)nr);
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return rows[a] < rows[b]; });
    for (int64_t q = 0; q < nr; ++q) {
      r0[(size_t)q] = (int32_t)(rows[q] - 1);
      slot[(size_t)ord[(size_t)q]] = (int32_t)q;
    }
    wcp.resize((size_t)Gc + 1);
    wrv.resize((size_t)(Gc * nr));
    for (int64_t j = 0; j <= Gc; ++j) wcp[(size_t)j] = 1 + j * nr;
    for (int64_t j = 0; j < Gc; ++j)
      for (int64_t q = 0; q < nr; ++q) wrv[(size_t)(j * nr + q)] = rows[ord[(size_t)q]];
    d_rows = buf.get<int32_t>((size_t)nr);
    d_slot = buf.get<int32_t>((size_t)nr);
    Wv = buf.get<T>((size_t)(nr * Gc));
    if (nr > 0) {
      HS_HIP(hipMemcpy(d_rows, r0.data(), (size_t)nr * sizeof(int32_t), hipMemcpyHostToDevice));
      HS_HIP(hipMemcpy(d_slot, slot.data(), (size_t)nr * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    W.colptr = wcp.data();
    W.rowval = wrv.data();
    W.nzval = Wv;
    return (size_t)nr * 2 * sizeof(int32_t);
  }
};

// ---- refusals: before any device work, every output untouched ------------------------------------------------------------------------
template <class T>
void check_block(hs_handle* F, int trans, const char* fn, const char* name, const hs_block_arg* b, int64_t n, int64_t nrhs) {
  if (!b) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: %s == NULL", fn, name);
  if (nrhs == 0) return;
  if (b->dense) {
    if (b->ld < n) HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: the leading dimension of %s is %lld, it has %lld rows", fn, name, (long long)b->ld, (long long)n);
    return;
  }
  if (!b->colptr) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: %s has neither dense values nor a colptr", fn, name);
  // the rules of hs_ldiv_sparse_* through its own host-only check
  const int st = hs_ldiv_sparse_plan(F, trans, n, nrhs, b->colptr, b->rowval, nullptr, 0, nullptr, nullptr, nullptr);
  if (st != HS_OK) {
    const std::string why = hs_last_error();
    hs_set_error(st, hs_last_error_info(), "%s: %s is not a valid sparse block (%s)", fn, name, why.c_str());
    throw st;
  }
  if (b->colptr[nrhs] > 1 && !b->nzval) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: %s has stored entries and nzval == NULL", fn, name);
}

template <class T>
void check_common(hs_handle* F, const char* fn, int trans, int64_t n, int64_t nrhs, int64_t itmax, int pattern, HsHandleView* v, bool ulv = false) {
  *v = hs_view_of(F, fn);
  if ((v->is_complex != 0) != (sizeof(T) == 16)) HS_FAIL(HS_ERR_ARGUMENT, 0, "MethodError: %s: eltype of F and of the blocks differ", fn);
  hs_check_trans(fn, trans);
  if (pattern < 0 || pattern > 1) HS_FAIL(HS_ERR_ARGUMENT, pattern, "ArgumentError: %s: pattern = %d (0: the stored entries of A, 1: the diagonal)", fn, pattern);
  if (itmax < 0) HS_FAIL(HS_ERR_ARGUMENT, itmax, "ArgumentError: %s: itmax = %lld < 0", fn, (long long)itmax);
  if (!v->device) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: handle holds a host-side plan only (hs_plan)", fn);
  if (!v->factored) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: factorization is not complete", fn);
  {  // what hs_ldiv_block_t_* refuses is refused here, by its own check: a block solve of no columns
    const int st = block_solve<T>(F, ulv, trans, nullptr, v->n, nullptr, v->n, v->n, 0, nullptr);
    if (st != HS_OK) {
      const std::string why = hs_last_error();
      hs_set_error(st, hs_last_error_info(), "%s: the block solve does not serve this handle (%s)", fn, why.c_str());
      throw st;
    }
  }
  if (n != v->n || nrhs < 0)
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: the blocks have %lld rows and %lld columns, F is %lld x %lld", fn, (long long)n, (long long)nrhs, (long long)v->n,
            (long long)v->n);
}

// distinct rows inside 1..n
inline void check_rows(const char* fn, const int64_t* rows, int64_t nrows, int64_t n) {
  std::vector<unsigned char> seen((size_t)n, 0);
  for (int64_t q = 0; q < nrows; ++q) {
    if (rows[q] < 1 || rows[q] > n) HS_FAIL(HS_ERR_DIMENSION, q, "BoundsError: %s: rows[%lld] = %lld outside 1:%lld", fn, (long long)q + 1, (long long)rows[q], (long long)n);
    if (seen[(size_t)(rows[q] - 1)]) HS_FAIL(HS_ERR_ARGUMENT, q, "ArgumentError: %s: row %lld is listed twice (the receiver rows must be distinct)", fn, (long long)rows[q]);
    seen[(size_t)(rows[q] - 1)] = 1;
  }
}

template <class T>
void to_blk(const hs_block_arg* a, Blk<T>* b) {
  b->dense = (const T*)a->dense;
  b->ld = a->ld;
  b->colptr = a->colptr;
  b->rowval = a->rowval;
  b->nzval = (const T*)a->nzval;
}
// a host block on the device: dense with ld = n, or the stored values
template <class T>
void upload(const hs_block_arg* a, int64_t n, int64_t nrhs, Blk<T>* b, HsDevBuf& buf, hipStream_t s, double* moved) {
  to_blk<T>(a, b);
  if (nrhs == 0) return;
  if (a->dense) {
    T* d = buf.get<T>((size_t)n * nrhs);
    HS_HIP(hipMemcpy2DAsync(d, n * sizeof(T), a->dense, a->ld * sizeof(T), n * sizeof(T), nrhs, hipMemcpyHostToDevice, s));
    b->dense = d;
    b->ld = n;
    *moved += (double)n * nrhs;
  } else {
    const int64_t cnt = a->colptr[nrhs] - 1;
    T* d = buf.get<T>((size_t)cnt);
    if (cnt > 0) HS_HIP(hipMemcpyAsync(d, a->nzval, (size_t)cnt * sizeof(T), hipMemcpyHostToDevice, s));
    b->nzval = d;
    *moved += (double)cnt;
  }
}

}  // namespace
