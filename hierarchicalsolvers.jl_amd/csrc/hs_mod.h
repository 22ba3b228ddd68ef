// hs_mod.h -- the launch API of kernels_mod.hip: the device pieces of a solve with A1 = A + U V^H through the Sherman-Morrison-Woodbury
// identity on a stored factorization (hs_mod_*, hs_mod.hip; include/hs_solver.h).  hs_mod.hip and the test hooks (hsk_mod_*) are the callers.
//
// Every block is column-major.  No kernel uses atomics or waits on another workgroup; every output element has one summation order that
// depends on the sizes alone (not on the grid, and not on the other columns of the block or on their number).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_common.h"

#ifndef HS_MOD_MAXRANK
#define HS_MOD_MAXRANK 256  // k <= 256: LU(C) is factored and applied by one workgroup per column (include/hs_solver.h)
#endif
#define HS_MOD_SLAB 2048    // rows of P and Y one workgroup of mod_inner reduces
#define HS_MOD_MAXCOLS 64   // m <= 64: the widest chunk of the block solve (HS_LDIV_BLOCK_COLS)

inline int64_t hs_mod_slabs(int64_t n) { return (n + HS_MOD_SLAB - 1) / HS_MOD_SLAB; }

// T (k x m, ld ldt) = op(P)^H Y with P n x k (ldp), Y n x m (ldy), op = identity (conj = 0: T = P^H Y) or conj (conj = 1: T = P^T Y; Float64
// ignores it).  v_mfma_f64_16x16x4_f64 with K = rows: workgroup (s, q) reduces rows [s SLAB, (s + 1) SLAB) for 64 columns of P and writes the
// partial part[s] (k x m, ld k); a second launch adds the partials in slab order.  part: hs_mod_slabs(n) * k * m elements.
// Order of one element: per slab, from zero, a chain of fused multiply-adds over its rows in steps of 8 rows, inside a step rows
// 0 2 4 6 1 3 5 7 (ComplexF64: steps of 4 rows in order; the real part takes re*re of the 4 rows, then -(+-im)*im; the imaginary part re*im,
// then (+-im)*re); rows past n enter as exact zeros.  tests/mod_mirror.py states it in NumPy.
template <class T>
void launch_mod_inner(const T* P, int64_t ldp, const T* Y, int64_t ldy, int64_t n, int k, int m, int conj, T* part, T* Tout, int64_t ldt, hipStream_t s);
// Y (n x m, ldy) -= op(Z) T with Z n x k (ldz) read once per 16 columns of Y, T k x m (ldt) negated into LDS; MFMA with K = k padded to 4 with
// zeros; op = conj with conj = 1 (ComplexF64).  One chain per element from Y's value over j = 0 .. k-1.
template <class T>
void launch_mod_apply(T* Y, int64_t ldy, const T* Z, int64_t ldz, const T* Tm, int64_t ldt, int64_t n, int k, int m, int conj, hipStream_t s);
// T[j, c] = Y[J[j], c] (J 0-based, on the device): the inner product with V = I[:, J]
template <class T>
void launch_mod_gather(T* Tout, int64_t ldt, const T* Y, int64_t ldy, const int64_t* J, int k, int m, hipStream_t s);
// partial-pivoting LU of C (k x k, ldc, k <= HS_MOD_MAXRANK) in place, one workgroup: piv[j] = the row exchanged with row j (0-based);
// *info = 0, or 1 + the first column whose pivot is exactly zero (the factorization stops there)
template <class T>
void launch_mod_cap_lu(T* C, int ldc, int k, int* piv, int* info, hipStream_t s);
// T (k x m, ldt; any m) = op(C)^-1 T from LU(C): op = 0: C, 1: C^T, 2: C^H.  One workgroup per column
template <class T>
void launch_mod_cap_solve(const T* LU, int ldc, int k, const int* piv, int op, T* Tm, int64_t ldt, int m, hipStream_t s);
// C[j, j] += 1 for j < k
template <class T>
void launch_mod_add_eye(T* C, int ldc, int k, hipStream_t s);
// out[row[e] + col[e] * ld] = val[e] for e < cnt (out cleared by the caller; the entries are distinct)
template <class T>
void launch_mod_scatter(T* out, int64_t ld, const int32_t* row, const int32_t* col, const T* val, int64_t cnt, hipStream_t s);

// ---- hs_mod.hip, as hs_gmres_block.hip sees it (hs_gmres_block_mod_*) -------------------------------------------------------------------------
struct hs_mod;
struct hs_handle;
// hs_mod_ldiv_dev_d or _z by the element type of the object (device blocks, queued on s); returns its status
int hs_mod_apply_prec(hs_mod* M, int trans, void* dC, int64_t ldc, const void* dB, int64_t ldb, int64_t n, int64_t nrhs, hipStream_t s);
// the factorization handle the modification was built on (null for a null object)
hs_handle* hs_mod_handle(hs_mod* M);
