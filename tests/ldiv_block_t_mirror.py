"""NumPy statement of the schedule of the transposed / adjoint block solve (csrc/hs_solve_multi.hip: hs_solve_multi_run with trans = 1, 2) over the fronts
of tests/ldiv_block_mirror.py (P D = L11 U11, Lbi = Abi U11^-1, Uib = L11^-1 P Aib, the inverses of the 256 x 256 diagonal blocks).

With op(x) = x for transpose(F) and conj(x) for adjoint(F), per chunk of `kc` columns

  forward, deepest level first, per front:   W = B[int, :] (no permutation);  for each 256-block j:  Z_j = op(inv(U11_jj))^T W_j,
                                             W[below j] -= op(U11[j, below j])^T Z_j;   B[bnd, :] -= op(Uib)^T Z
                                             (low-rank:  -= op(Z_R)^T (op(G)^T Z))
  backward, root first, per front:           W = Z - op(Lbi)^T B[bnd, :]   (low-rank:  - op(Z_L)^T (op(C_L)^T B[bnd, :]));  for each block j,
                                             last first:  X_j = op(inv(L11_jj))^T W_j,  W[above j] -= op(L11[j, above j])^T X_j;
                                             B[int[rperm[i]], :] = X[i, :]

`left=True` is the left-looking order of the triangular sweeps (W_j takes all its updates just before block j is solved)."""
import numpy as np

from ldiv_block_mirror import BS, Front, fronts_by_level  # noqa: F401  (Front: the class the schedule runs over)


def _chunk_t(levels, B, conj, left):
    op = np.conj if conj else (lambda x: x)
    Z = {}
    for fronts in reversed(levels):  # leaves -> root
        for f in fronts:
            ni = len(f.int)
            W = B[f.int].copy()
            Zf = np.empty_like(W)
            for j, c0 in enumerate(range(0, ni, BS)):
                c1 = min(ni, c0 + BS)
                if left:
                    W[c0:c1] -= op(f.U11[:c0, c0:c1]).T @ Zf[:c0]
                Zf[c0:c1] = op(f.invU[j]).T @ W[c0:c1]
                if not left:
                    W[c1:] -= op(f.U11[c0:c1, c1:]).T @ Zf[c0:c1]
            if len(f.bnd) and ni:
                if f.lowrank:
                    _, _, G, ZR = f.lowrank
                    B[f.bnd] -= op(ZR).T @ (op(G).T @ Zf)
                else:
                    B[f.bnd] -= op(f.Uib).T @ Zf
            Z[id(f)] = Zf
    for fronts in levels:  # root -> leaves
        for f in fronts:
            ni = len(f.int)
            W = Z[id(f)].copy()
            if len(f.bnd) and ni:
                if f.lowrank:
                    CL, ZL, _, _ = f.lowrank
                    W -= op(ZL).T @ (op(CL).T @ B[f.bnd])
                else:
                    W -= op(f.Lbi).T @ B[f.bnd]
            X = np.empty_like(W)
            starts = list(range(0, ni, BS))
            for j in reversed(range(len(starts))):
                c0, c1 = starts[j], min(ni, starts[j] + BS)
                if left:
                    W[c0:c1] -= op(f.L11[c1:, c0:c1]).T @ X[c1:]
                X[c0:c1] = op(f.invL[j]).T @ W[c0:c1]
                if not left:
                    W[:c0] -= op(f.L11[c0:c1, :c0]).T @ X[c0:c1]
            B[f.int[f.rperm]] = X


def ldiv_block_t(levels, B, trans="T", kc=32, left=False):
    """F^-T B (trans = "T") or F^-H B (trans = "H") for an n x k block, `kc` columns at a time."""
    assert trans in ("T", "H")
    B = np.array(B, dtype=np.result_type(B.dtype, levels[0][0].L11.dtype), copy=True)
    vec = B.ndim == 1
    Bm = B.reshape(B.shape[0], -1)
    for c0 in range(0, Bm.shape[1], kc):
        blk = Bm[:, c0 : c0 + kc].copy()
        _chunk_t(levels, blk, trans == "H", left)
        Bm[:, c0 : c0 + kc] = blk
    return Bm[:, 0] if vec else Bm
