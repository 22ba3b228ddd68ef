// hs_envelope.h -- block envelope of a front's sparsity pattern (host side, analysis time): leaf fronts (hs_leaf_envelope) and branch fronts
// (hs_branch_envelope: two dense Schur complements on disjoint DOF sets plus A's entries across the cut -- not a dense matrix).
//
// A leaf front F = [Aii Aib; Abi Abb] (front order [int; bnd]) is assembled from A alone, and LU that pivots only inside the 32-row diagonal
// blocks (optimistic pivoting) keeps the envelope of F taken per 32-row / 32-column block:
//   L[r, k] = 0 (and L21 = Abi * U^-1 likewise) for k < firstL[block of r],   U[k, c] = 0 (and U12 = L^-1 * P * Aib) for k < firstU[block of c],
// because every entry outside it is a sum of products with an exact zero factor, and a swap inside a diagonal block moves a row inside its
// own block.  The GEMM tiles of such a front start their K loop at max(firstL of their rows, firstU of their columns) (kernels_gemm.hip).
//
//   firstL[b]: first column < ni, rounded down to a multiple of 32, at which any row of block b has a structural entry; HS_ENV_NONE if none
//   firstU[b]: first row    < ni, rounded down likewise,            at which any column of block b has one;          HS_ENV_NONE if none
// Blocks: hs_env_block (hs_common.h) -- interior blocks from 0, boundary blocks from the start of the boundary part (ni is no multiple of 32).
// The diagonal counts as present; explicitly stored zeros of A are structural entries.
#pragma once
#include <stdint.h>
#include "hs_common.h"

inline int hs_env_nblocks(int ni, int nb) { return (ni + 31) / 32 + (nb + 31) / 32; }

// colptr / rowval: the CSC pattern of A, 1-based (as the C ABI takes it); fidx: ni + nb global ids (0-based), front order;
// where: n entries, all -1 on entry and on return (scratch); firstL, firstU: hs_env_nblocks(ni, nb) entries each
inline void hs_leaf_envelope(const int64_t* colptr, const int64_t* rowval, const int* fidx, int ni, int nb, int* where, int* firstL, int* firstU) {
  const int m = ni + nb, nblk = hs_env_nblocks(ni, nb);
  for (int b = 0; b < nblk; ++b) firstL[b] = firstU[b] = HS_ENV_NONE;
  for (int p = 0; p < m; ++p) where[fidx[p]] = p;
  for (int p = 0; p < ni; ++p) {  // the diagonal of the interior block
    const int b = p >> 5, v = p & ~31;
    firstL[b] = std::min(firstL[b], v);
    firstU[b] = std::min(firstU[b], v);
  }
  for (int c = 0; c < m; ++c) {
    const int64_t g = fidx[c];
    const int bc = hs_env_block(c, ni);
    for (int64_t e = colptr[g] - 1; e < colptr[g + 1] - 1; ++e) {
      const int r = where[rowval[e] - 1];
      if (r < 0) continue;
      if (c < ni) { int& f = firstL[hs_env_block(r, ni)]; f = std::min(f, c & ~31); }
      if (r < ni) firstU[bc] = std::min(firstU[bc], r & ~31);
    }
  }
  for (int p = 0; p < m; ++p) where[fidx[p]] = -1;
}

// A branch front is assembled from the Schur complements of its two children and from the entries of A across the cut.  The children own
// disjoint DOFs: positions p < ni1 and ni <= p < ni + nb1 belong to child 1, the others to child 2 (front order [int1; int2 | bnd1; bnd2]).
// Its structural pattern is every pair of positions of the same child (a Schur complement is dense), every stored entry of A between the
// front's DOFs and the interior diagonal; the tables are those of hs_leaf_envelope for that pattern.  For a 7-point stencil rows bnd2 then
// have nothing in columns int1 (L[bnd2, int1] = 0, U[int1, bnd2] = 0) and rows int2 start at their partner column of int1.
// A missing child is ni1 = nb1 = 0 or ni1 = ni, nb1 = nb: one dense block.  Arguments as for hs_leaf_envelope.
inline void hs_branch_envelope(const int64_t* colptr, const int64_t* rowval, const int* fidx, int ni, int nb, int ni1, int nb1, int* where, int* firstL,
                               int* firstU) {
  hs_leaf_envelope(colptr, rowval, fidx, ni, nb, where, firstL, firstU);  // the entries of A and the diagonal
  const int m = ni + nb;
  // a position of child s meets every interior position of child s: the first of them is 0 (child 1) or ni1 (child 2)
  const int first[2] = {ni1 > 0 ? 0 : HS_ENV_NONE, ni1 < ni ? (ni1 & ~31) : HS_ENV_NONE};
  for (int p = 0; p < m; ++p) {
    const int side = p < ni ? (p < ni1 ? 0 : 1) : (p - ni < nb1 ? 0 : 1);
    const int b = hs_env_block(p, ni);
    firstL[b] = std::min(firstL[b], first[side]);
    firstU[b] = std::min(firstU[b], first[side]);
  }
}
