// hs_gn.h -- the kernels of the tangent-linear solves and Gauss-Newton products (kernels_gn.hip) as hs_gn.hip and the test hooks see them.
//
// All are plain launches: one lane owns one output row (or one stored entry) and runs its sums serially in a register, every step the same
// unfused products and sums, no atomics and no waiting between workgroups.  The order of a sum depends on the pattern (kernel 1) or on the
// order of the columns (kernel 3) alone, so neither result depends on how the columns were grouped.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_common.h"

// The rows of op(E) as entry ranges ptr[i] .. ptr[i + 1] of idx (0-based): the CSR map of A for trans = 0 (perm = its CSR entry -> CSC entry
// map, the value of entry e is E[perm[e]]), the CSC arrays of A for trans = 1, 2 (perm = null: the value is E[e], conjugated when conj).
struct HsGnRows {
  const int64_t* ptr;
  const int32_t* idx;
  const int64_t* perm;
  int conj;
};
// P[i, c] = 0 - sum over the entries e of row i, in order, of val(e) * X[idx[e], c]   (n x kc, column-major), every step acc - v * x
template <class T>
void launch_gn_rhs(HsGnRows r, const T* E, int64_t n, const T* X, int64_t ldx, int kc, T* P, int64_t ldp, hipStream_t s);
// E on the diagonal (n values; colptr, rowval: the CSC pattern of A): P[i, c] = 0 - e_i X[i, c] (e_i conjugated when conj) where (i, i) is
// stored, 0 elsewhere
template <class T>
void launch_gn_rhs_diag(const int64_t* colptr, const int32_t* rowval, const T* Ed, int conj, int64_t n, const T* X, int64_t ldx, int kc, T* P, int64_t ldp, hipStream_t s);
// the receiver rows of a block: JE[q, c] = D[rows[q], c] (JE may be null) and Wv[c * nrows + slot[q]] = D[rows[q], c] or its conjugate (Wv
// may be null): the values of the sparse cotangent, rows ascending
template <class T>
void launch_gn_rows(const T* D, int64_t ldd, const int32_t* rows, const int32_t* slot, int64_t nrows, int kc, T* JE, int64_t ldj, T* Wv, int conj, hipStream_t s);
// acc[i] <- acc[i] + |X[i, c]|^2 for c = 0 .. kc-1 in order (|x|^2 = re^2 + im^2, or x * x)
template <class T>
void launch_gn_rowsq(const T* X, int64_t ldx, int64_t n, int kc, double* acc, hipStream_t s);
// Hd[p] = z2[a_p] * x2[b_p] for the stored entry p = (i, j): (a, b) = (i, j) or, with swap, (j, i)
void launch_gn_diag(const int32_t* rowval, const int32_t* ecol, int64_t nnz, const double* z2, const double* x2, int swap, double* Hd, hipStream_t s);
// Hd[j] = z2[j] * x2[j] where (j, j) is stored, 0 elsewhere
void launch_gn_diag_diag(const int64_t* colptr, const int32_t* rowval, int64_t n, const double* z2, const double* x2, double* Hd, hipStream_t s);

// hs_api.hip: the eight figures of the handle's last hs_tangent_* / hs_gn_* call (hs_gn_info)
struct hs_handle;
double* hs_handle_gn_info(hs_handle* h);
