// kernels_solve_multi_mul.hip -- the panel products of hs_mul_* (C = op(F) B, hs_mul_run in hs_solve_multi.hip): the workgroup body of the block
// solves (hs_multi_tile.h) over the MUL sides of hs_multi_fwd.h / hs_multi_tr.h, factors stored as T.
//
// What a product with the factors needs and a solve does not:
//  * triangular operands in place in LF: the unit lower trapezoid (trap = 1, [L11; Lbi] as ONE panel) and the upper triangle with its
//    diagonal (trap = 2, U11).  A workgroup reads only the 16-column chunks that meet its rows -- about half of the ni x ni block over all
//    workgroups -- and splits THOSE over its four waves as a solve's product splits all of K; the partial sums meet in the same order
//    (w0 + w2) + (w1 + w3).  What lies in the other triangle of a chunk that is read is replaced by a select, never multiplied.
//  * D = Cin + A X (minus = 0 with Cin set) beside Cin - A X and A X.
//  * two work blocks on one side of one product: rows >= ni of the trapezoid's result are added into the boundary block (C2), and its
//    transpose reads its X from the interior rows and then from the boundary block (X2).
// A unit of its own like the other three: the kernels of the solves keep their allocation as long as nothing else is compiled beside them
// (DESIGN.md section 4a).
#include "hs_multi_kernels.h"

HS_MULTI_INST_MUL(double)
HS_MULTI_INST_MUL(cplx)
