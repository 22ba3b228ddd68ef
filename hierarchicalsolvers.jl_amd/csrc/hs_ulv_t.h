// hs_ulv_t.h -- the grouped product of the transposed / adjoint ULV solve of the HSS module (kernels_ulv_t.hip, hs_hss_ldiv_t).
#pragma once
#include "hs_common.h"

// One job of a grouped launch:   C[M x N] = Cin - op(A)^T X   or, with Cin null,   C = op(A)^T X.
//   A    K x M column-major (lda): a stored block of the ULV factors read along its columns, so the reduction index k is the contiguous one
//   X    K x N column-major (ldx), Cin and C  M x N column-major (ldcin, ldc)
//   conj op = conj (ComplexF64 only), applied while A is loaded
//   tri  0: every stored entry counts;  1: only k >= m (A lower triangular: a 32 x 32 inverse of a unit-lower diagonal block);
//        2: only k <= m (upper triangular: the inverse of an upper diagonal block)
// C may be Cin (every entry is read and written by the same lane); C must not overlap X or A.  A job with M, K or N <= 0 does nothing.
template <class T>
struct UlvTJob {
  const T* A;
  const T* X;
  const T* Cin;
  T* C;
  int M, K, N;
  int lda, ldx, ldcin, ldc;
  int conj, tri;
};
enum { HS_ULVT_FULL = 0, HS_ULVT_LOWER = 1, HS_ULVT_UPPER = 2 };

// one plain launch over djobs[0 .. njobs) (device array, njobs <= 65535), job = blockIdx.z; maxM / maxN: the largest M / N among them
template <class T>
void launch_ulv_t(const UlvTJob<T>* djobs, int njobs, int maxM, int maxN, hipStream_t s);

// rows of a column-major block through an index list (the front-level steps of hs_ldiv_ulv_* work on the caller's block directly):
//   mode 0: dst[i, c] = src[idx[i], c]        mode 1: dst[idx[i], c] = src[i, c]        for i < rows, c < cols
template <class T>
void launch_ulv_rows(const int* idx, int rows, int cols, const T* src, long long lds, T* dst, long long ldd, int mode, hipStream_t s);
