// hs_eigs.h -- the launch API of kernels_eigs.hip: the device pieces of hs_eigs_* (hs_eigs.hip; include/hs_solver.h), shift-invert block Arnoldi
// on a stored factorization.  hs_eigs.hip and the test hooks (hsk_eigs_*) are the callers; the tall-skinny inner products and corrections
// of the Gram-Schmidt passes are launch_mod_inner / launch_mod_apply (hs_mod.h).
//
// As there: every block is column-major, no kernel uses atomics or waits on another workgroup, and every output element has one summation
// order that depends on the sizes alone (not on the grid, and not on the number of rows).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_common.h"
#include "hs_mod.h"

#define HS_EIGS_MAXBASIS HS_MOD_MAXRANK  // ncv + block <= 256: the k of launch_mod_inner / launch_mod_apply and the K of launch_eigs_rotate
#define HS_EIGS_MAXBLOCK HS_MOD_MAXCOLS  // block <= 64: the m of those two and the p of launch_eigs_chol_inv
#define HS_EIGS_SLAB 2048                // rows one workgroup of eigs_colsq reduces

inline int64_t hs_eigs_slabs(int64_t n) { return (n + HS_EIGS_SLAB - 1) / HS_EIGS_SLAB; }

// Out[:, :N] (n rows, ldo) = V[:, :K] (ldv) Q with Q K x N (ldq) on the device, K <= 256, N <= K.  Out may be V (the same pointer and ld):
// a workgroup owns 32 rows (ComplexF64: 16), copies all K entries of them into LDS and only then writes.  v_mfma_f64_16x16x4_f64 on the
// transposed tile (Out^T = Q^T V^T, as mod_apply); per element one chain from zero over j = 0 .. K-1, K padded to 4 with zeros; ComplexF64:
// the real part takes re*re then -im*im per step of 4, the imaginary part re*im then im*re.
template <class T>
void launch_eigs_rotate(T* Out, int64_t ldo, const T* V, int64_t ldv, const T* Q, int64_t ldq, int64_t n, int K, int N, hipStream_t s);
// G (p x p Gram matrix, ldg, Hermitian, upper triangle read; p <= 64) = R^H R:  R and Rinv = R^-1 (both p x p, ld p, upper, zeros below),
// *info = -1, or the first column c whose pivot G[c, c] - sum_i |R[i, c]|^2 is not above (64 eps)^2 times the largest diagonal entry of G
// (R and Rinv are then not to be used).  One workgroup.
template <class T>
void launch_eigs_chol_inv(const T* G, int ldg, int p, T* R, T* Rinv, int* info, hipStream_t s);
// Column figures of a block, slab partials added in slab order.  With X == nullptr: nrm[c] = ||Y[:, c]||_2.  With X: Y[:, c] -= the column
// c of X diag(mu) first (Y = op(A) X on entry, the residual on exit): mu[c] = (re, im); pair[c] = 0: a column of its own (Float64: mu real),
// +1 / -1: the real / imaginary part of a Float64 conjugate pair in columns (c, c + 1) / (c - 1, c), which take the 2 x 2 block
// [re -im; im re] of the first.  A pair shares one figure: the norm of the complex vector.  part: hs_eigs_slabs(n) * nc doubles.
template <class T>
void launch_eigs_resid(T* Y, int64_t ldy, const T* X, int64_t ldx, const double* mu, const int* pair, int64_t n, int nc, double* part, double* nrm, hipStream_t s);
// d[c] = Re sum_i conj(X[i, c]) Y[i, c], the slab scheme of launch_eigs_resid: HS_EIGS_SLAB rows per workgroup, a thread adds its rows in
// order, the partials fold by halves, the slabs are added in slab order.  pair as above (may be nullptr): a Float64 pair shares one figure,
// the sum over both columns.  With Y = op(M) X this is x^H op(M) x of the generalized problem (hs_eigs_gen_*); any nc, unlike
// launch_mod_inner.  part: hs_eigs_slabs(n) * nc doubles.
template <class T>
void launch_eigs_coldot(const T* X, int64_t ldx, const T* Y, int64_t ldy, const int* pair, int64_t n, int nc, double* part, double* d, hipStream_t s);
// d[c] = sqrt(d[c]) where d[c] > 0, else 0 (launch_eigs_scale then leaves the column)
void launch_eigs_sqrt(double* d, int nc, hipStream_t s);
// X[:, c] /= nrm[c] (a zero norm leaves the column)
template <class T>
void launch_eigs_scale(T* X, int64_t ldx, const double* nrm, int64_t n, int nc, hipStream_t s);
// X[i, c] = the entry i of the seeded column `col0 + c` of draw `salt`: uniform in (-1, 1) from a splitmix64 counter (ComplexF64: both parts)
template <class T>
void launch_eigs_init(T* X, int64_t ldx, int64_t n, int nc, int64_t seed, int col0, int salt, hipStream_t s);
