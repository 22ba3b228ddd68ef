"""NumPy statement of the schedule of hs_mul_* (csrc/hs_solve_multi.hip, hs_mul_run): C = op(F) X with the stored factorization as an
operator, over the Front objects of tests/ldiv_block_mirror.py (per front  P D = L11 U11,  Lbi = Abi U11^-1,  Uib = L11^-1 P Aib;
(P x)[i] = x[rperm[i]]).  With Y_f an intermediate per front, an n x k block takes two passes per chunk of `kc` columns and no triangular
solve:

  trans = 0     U pass, every front on its own:   Y_f = triu(U11) X[int] + Uib X[bnd]                  (low-rank:  + G (Z_R X[bnd]))
                L pass, root level first:         B[int[rperm]] = unit-tril(L11) Y_f;   B[bnd] += Lbi Y_f       (+= C_L (Z_L Y_f))
  trans = 1, 2  first pass, every front:          Z_f = op(L11)^T X[int[rperm]] + op(Lbi)^T X[bnd]     (+ op(Z_L)^T (op(C_L)^T X[bnd]))
                second pass, root level first:    B[int] = op(U11)^T Z_f;   B[bnd] += op(Uib)^T Z_f             (+= op(Z_R)^T (op(G)^T Z_f))

op = identity (trans = 1) or conj (trans = 2).  The first pass reads X only, so the product may be formed in place; the second sets the
interior rows of a front and adds into its boundary rows, which are interior rows of its ancestors: root first.  `lowrank=True` fronts
(ldiv_block_mirror.fronts_by_level) apply Lbi and Uib through C Z / G Z."""
import numpy as np

TRANS = {0: 0, 1: 1, 2: 2, "N": 0, "T": 1, "C": 2, "H": 2}


def _chunk(levels, X, trans):
    op = np.conj if trans == 2 else (lambda a: a)
    B = np.empty_like(X)
    mid = {}
    for fronts in levels:  # any order: every front reads X only
        for f in fronts:
            has_b = len(f.bnd) and len(f.int)
            if trans == 0:
                Y = f.U11 @ X[f.int]
                if has_b:
                    if f.lowrank:
                        _, _, G, ZR = f.lowrank
                        Y += G @ (ZR @ X[f.bnd])
                    else:
                        Y += f.Uib @ X[f.bnd]
            else:
                Y = op(f.L11).T @ X[f.int[f.rperm]]
                if has_b:
                    if f.lowrank:
                        CL, ZL, _, _ = f.lowrank
                        Y += op(ZL).T @ (op(CL).T @ X[f.bnd])
                    else:
                        Y += op(f.Lbi).T @ X[f.bnd]
            mid[id(f)] = Y
    for fronts in levels:  # root -> leaves
        for f in fronts:
            has_b = len(f.bnd) and len(f.int)
            Y = mid[id(f)]
            if trans == 0:
                B[f.int[f.rperm]] = f.L11 @ Y
                if has_b:
                    if f.lowrank:
                        CL, ZL, _, _ = f.lowrank
                        B[f.bnd] += CL @ (ZL @ Y)
                    else:
                        B[f.bnd] += f.Lbi @ Y
            else:
                B[f.int] = op(f.U11).T @ Y
                if has_b:
                    if f.lowrank:
                        _, _, G, ZR = f.lowrank
                        B[f.bnd] += op(ZR).T @ (op(G).T @ Y)
                    else:
                        B[f.bnd] += op(f.Uib).T @ Y
    return B


def mul(levels, X, trans=0, kc=32):
    """op(F) X for a vector or an n x k block, `kc` columns at a time; trans = 0 / 1 / 2 (or "N" / "T" / "C")."""
    t = TRANS[trans]
    X = np.array(X, dtype=np.result_type(np.asarray(X).dtype, levels[0][0].L11.dtype), copy=True)
    vec = X.ndim == 1
    Xm = X.reshape(X.shape[0], -1)
    out = np.empty_like(Xm)
    for c0 in range(0, Xm.shape[1], kc):
        out[:, c0 : c0 + kc] = _chunk(levels, Xm[:, c0 : c0 + kc], t)
    return out[:, 0] if vec else out


def op_of(A, trans):
    """op(A) of a SciPy sparse matrix for trans = 0 / 1 / 2."""
    t = TRANS[trans]
    return A if t == 0 else (A.T if t == 1 else A.conj().T)
