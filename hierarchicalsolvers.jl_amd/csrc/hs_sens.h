// hs_sens.h -- the kernels of the adjoint-state sensitivities (kernels_sens.hip) as hs_sens.hip and the test hooks see them.
//
// The reduction is a sampled dense-dense product over the CSC pattern of A as the handle keeps it on the device (0-based int64 column
// pointers, 0-based int32 row indices; the hooks rebase Julia's 1-based arrays as every upload of the library does).  For the stored entry
// p = (i, j):
//
//   G[p] <- G[p] - sum over c = 0 .. kc-1 of f(L[a_p, c]) * g(R[b_p, c]),     (a_p, b_p) = (i, j) or, with `swap`, (j, i)
//
// f, g: identity or conjugate.  ONE chain per entry: it starts from the value G[p] holds, takes the columns in order, and every step is the
// same unfused expression (HsSensStep), so columns fed in several calls give the bits of one call, and both forms below give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_common.h"

struct HsSddmmFlags {
  int swap;   // 0: (a, b) = (i, j); 1: (j, i)
  int conjl;  // f = conj
  int conjr;  // g = conj
};

// ecol[p] = the column of stored entry p (the largest j with colptr[j] <= p): built once per call, read by both forms
void launch_sens_entry_cols(const int64_t* colptr, int64_t n, int64_t nnz, int32_t* ecol, hipStream_t s);
// the direct form: one lane per stored entry, L and R read where they are (column-major, leading dimensions ldl, ldr)
template <class T>
void launch_sddmm(const int32_t* rowval, const int32_t* ecol, int64_t nnz, const T* L, int64_t ldl, const T* R, int64_t ldr, int kc, HsSddmmFlags f, T* G, hipStream_t s);
// the row-staged form: Lt, Rt are the blocks transposed into row-major work blocks (row r at Lt + r * stride, hs_sens_row_stride(kc) elements)
int64_t hs_sens_row_stride(int kc, int is_complex);
template <class T>
void launch_sens_rowstage(const T* in, int64_t ld, int64_t n, int kc, T* out, int64_t stride, hipStream_t s);
template <class T>
void launch_sddmm_rows(const int32_t* rowval, const int32_t* ecol, int64_t nnz, const T* Lt, const T* Rt, int64_t stride, int kc, HsSddmmFlags f, T* G, hipStream_t s);
// the diagonal only: Gd[j] continues its chain where (j, j) is stored (the first such entry of the column) and is set to 0 where it is not
template <class T>
void launch_sddmm_diag(const int64_t* colptr, const int32_t* rowval, int64_t n, const T* L, int64_t ldl, const T* R, int64_t ldr, int kc, HsSddmmFlags f, T* Gd,
                       hipStream_t s);

// out[:, c] = in[:, c] or its conjugate (n x kc, column-major)
template <class T>
void launch_sens_copy(T* out, int64_t ldo, const T* in, int64_t ldi, int64_t n, int kc, int conj, hipStream_t s);
// out[erow[e], ecol[e]] = val[e] or its conjugate; out is zero-filled by the caller
template <class T>
void launch_sens_expand(T* out, int64_t ldo, const int32_t* erow, const int32_t* ecol, const T* val, int64_t cnt, int conj, hipStream_t s);
// the misfit form, one workgroup per column c: r = X[rows[q], c] - D[q, c] for q = 0 .. nrows-1; R[q, c] = r (R may be null);
// Wv[c * nrows + slot[q]] = r or conj(r) (the values of the sparse cotangent, rows ascending); J[c] = 0.5 * sum |r|^2, summed per thread over
// q = t, t + 256, ... and then over the threads by a binary tree: an order that depends on nrows alone
template <class T>
void launch_sens_misfit(const T* X, int64_t ldx, const int32_t* rows, const int32_t* slot, const T* D, int64_t ldd, int64_t nrows, int kc, T* R, int64_t ldr, T* Wv,
                        int conj, double* J, hipStream_t s);

// hs_api.hip: the eight figures of the handle's last hs_sens_* / hs_misfit_* call (hs_sens_info)
struct hs_handle;
double* hs_handle_sens_info(hs_handle* h);
