// kernels_solve_multi_t.hip -- the one operation of the transposed / adjoint block solve (hs_ldiv_block_t_*, hs_solve_multi.hip):
//
//   D[M x kc] = op(A)^T X[K x kc]      or      D = Cin - op(A)^T X,        A stored K x M column-major, op = identity or conj,
//
// A a stored factor panel read along its columns (a row panel of U11 / L11, Uib, Lbi, a 256 x 256 inverse diagonal block, a factor of a
// low-rank Gauss transform), X, Cin and D rows of the row-major work blocks of the driver, kc <= 64 right-hand sides.
//
// A translation unit of its own, with its own kernels: multi_level_kernel / multi_prob_kernel (kernels_solve_multi.hip) sit at their
// register limit and keep their allocation only as long as nothing else is compiled into their functions (DESIGN.md section 4a⁗″).  What
// the two products have in common -- the workgroup's body (accumulators, chunks in flight, LDS exchange, the read and the store of D), the
// complex MFMA chain, MultiX, the choice of NT -- is source shared through hs_multi_tile.h and instantiated here, for factors stored as T,
// over MultiTr (hs_multi_tr.h): the transposed product's own operand loads, real MFMA chain, contiguous split of K and row map.  The
// kernels and launches are hs_multi_kernels.h; the column-major <-> row-major copies of both directions are launch_multi_move of
// kernels_solve_multi.hip.
//
// The forward kernel reads A[M x K] with the OUTPUT rows contiguous; here the REDUCTION index k is the contiguous one.  The A operand of
// v_mfma_f64_16x16x4_f64 wants lane (m = lane & 15, group = lane >> 4) to hold op(A)^T[m, k] = A[k, m] for one k of the group's four per
// k-step; the natural k = kb + 4 ks + group makes every lane fetch isolated 8-byte words.  The sum over k does not care which k a (group,
// k-step) pair holds as long as the X operand uses the same assignment, so a lane owns PAIRS of consecutive k of its column:
//  * Float64:  k(ks) = kb + 8 (ks >> 1) + 2 group + (ks & 1): one 16-byte load per lane and pair of k-steps.  A load instruction covers 64
//    consecutive bytes (4 groups x 16 B) of each of 16 columns, the two loads of a 16-row chunk 128 bytes of each column.
//  * ComplexF64:  k(ks) = kb + 4 ks + group, one 16-byte element per lane: the same 64 bytes per column and instruction, 256 per chunk.
//    re and im are the two operands of the four real MFMAs of a complex product (conj: im is negated as it is loaded).
//  * A workgroup owns 64 (ComplexF64: 32) output rows = columns of A, as four (two) MFMA row tiles of 16 columns each; the four waves SPLIT
//    K into four CONTIGUOUS quarters (a wave streams 512 consecutive bytes of each of its columns when K = 256), 16 k at a time, two
//    chunks in flight in two register arrays, and the partial sums meet in LDS in the fixed order (w0 + w2) + (w1 + w3).
//  * A goes from global memory straight to the operand registers, is used for ceil(kc / 16) MFMAs and never touches LDS; X is the B
//    operand (16 adjacent doubles of a row-major work-block row per lane group), optionally gathered through a row map (the trapezoid
//    form of a low-rank C: C^T x = trap(Lp)^T (P x)).
//  * No atomics, one summation order per output element that depends on K alone, and a column of D depends on its own column of X and Cin
//    only, wherever it sits in the chunk.
// C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg; hsk_multi_prob_t_* (hs_testhooks.hip) checks the maps, xmap included,
// with exact integer data (tests/test_ldiv_block_t_gpu.py).
#include "hs_multi_kernels.h"

HS_MULTI_INST_TR(double, double)
HS_MULTI_INST_TR(cplx, cplx)
