// kernels_solve_multi_f32.hip -- the two panel products of the block solves with the factor panel stored in Float32 / ComplexF32
// (hs_f32_*, hs_f32.hip): the kernels of hs_multi_kernels.h over MultiFwd<T, S> and MultiTr<T, S> with S = F32Of<T>::type.  A is read as
// S, carried through the hs_d2u operand registers of the shared workgroup body and widened in front of the MFMAs that consume it
// (MultiElem<S>, hs_multi_tile.h); everything else is the code of the FP64 kernels, so a lane holds the element the FP64 side holds for
// it and every output element has their summation order: on values that Float32 represents exactly the two give the same bits
// (tests/test_f32_gpu.py compares them so).
//
// Loads.  Float64 handles: the lane's row pair (forward) / k pair (transposed) is 8 bytes, one load; a wave load covers 128 contiguous
// bytes of each of its 4 columns (forward) or 32 bytes of each of 16 columns (transposed); the pair type is 4-byte aligned, since a panel
// may start at an odd row.  ComplexF64 handles: one cplxf (8 bytes) per lane and row tile.  (A lane taking FOUR rows, 16 bytes, with the
// row map changed to match, is the wider alternative; not built: DESIGN.md 4m.)
//
// A translation unit of its own, for the reason kernels_solve_multi_t.hip is one.
#include "hs_multi_kernels.h"

HS_MULTI_INST_FWD(double, float)
HS_MULTI_INST_FWD(cplx, cplxf)
HS_MULTI_INST_TR(double, float)
HS_MULTI_INST_TR(cplx, cplxf)
