"""NumPy statement of the schedule of the block solve (csrc/hs_solve_multi.hip) over a tree of (D, L, R, int, bnd) blocks such as the
oracle's FactorNode (oracle/hs_oracle.py: D = Aii, L = Abi D^-1, R = D^-1 Aib, 1-based index vectors).

Per front the device keeps  P D = L11 U11  (partial pivoting; (P x)[i] = x[rperm[i]]),  Lbi = Abi U11^-1,  Uib = L11^-1 P Aib  and the
explicit inverses of the 256 x 256 diagonal blocks of L11 and U11.  An n x k block goes through the tree in chunks of `kc` columns; per
chunk

  forward, deepest level first, per front:   W = B[int[rperm], :];  for each 256-row block j:  Y_j = inv(L11_jj) W_j,
                                             W[below j] -= L11[below j, j] Y_j;   B[bnd, :] -= Lbi Y   (low-rank:  -= C_L (Z_L Y))
  backward, root first, per front:           W = Y - Uib B[bnd, :]   (low-rank:  - G (Z_R B[bnd, :]));  for each block j, last first:
                                             X_j = inv(U11_jj) W_j,  W[above j] -= U11[above j, j] X_j;   B[int, :] = X

with ragged last blocks and a ragged last chunk.  `lowrank=True` applies Lbi and Uib through C Z / G Z taken from a full-rank SVD, the
form the compressed fronts use."""
import numpy as np
import scipy.linalg as sla

from selinv_mirror import dense_d, _dense

BS = 256


class Front:
    def __init__(self, x, level, lowrank):
        self.level = level
        self.int = np.asarray(x.int, dtype=np.int64) - 1
        self.bnd = np.asarray(x.bnd, dtype=np.int64) - 1
        ni = len(self.int)
        D = dense_d(x.D) if ni else np.zeros((0, 0))
        lu, piv = sla.lu_factor(D) if ni else (D, np.zeros(0, dtype=np.int64))
        rperm = np.arange(ni)
        for i, p in enumerate(piv):  # LAPACK swap targets -> accumulated permutation
            rperm[i], rperm[p] = rperm[p], rperm[i]
        self.rperm = rperm
        self.L11 = np.tril(lu, -1) + np.eye(ni)
        self.U11 = np.triu(lu)
        self.invL, self.invU = [], []
        for c0 in range(0, ni, BS):
            c1 = min(ni, c0 + BS)
            self.invL.append(np.linalg.inv(self.L11[c0:c1, c0:c1]))
            self.invU.append(np.linalg.inv(self.U11[c0:c1, c0:c1]))
        self.lowrank = None
        if len(self.bnd) and ni:
            Abi = _dense(x.L) @ D
            Aib = D @ _dense(x.R)
            self.Lbi = sla.solve_triangular(self.U11, Abi.T, trans="T", lower=False).T
            self.Uib = sla.solve_triangular(self.L11, Aib[rperm], lower=True, unit_diagonal=True)
            if lowrank:
                U, s, Vh = np.linalg.svd(self.Lbi, full_matrices=False)
                U2, s2, Vh2 = np.linalg.svd(self.Uib, full_matrices=False)
                self.lowrank = (U * s, Vh, U2 * s2, Vh2)  # C_L, Z_L, G, Z_R
        else:
            self.Lbi = np.zeros((len(self.bnd), ni), dtype=D.dtype)
            self.Uib = np.zeros((ni, len(self.bnd)), dtype=D.dtype)


def fronts_by_level(F, lowrank=False):
    levels, stack = {}, [(F, 1)]
    while stack:
        x, lv = stack.pop()
        levels.setdefault(lv, []).append(Front(x, lv, lowrank))
        stack += [(c, lv + 1) for c in (x.left, x.right) if c is not None]
    return [levels[lv] for lv in sorted(levels)]


def _chunk(levels, B):
    Y = {}
    for fronts in reversed(levels):  # leaves -> root
        for f in fronts:
            ni = len(f.int)
            W = B[f.int[f.rperm]].copy()
            Yf = np.empty_like(W)
            for j, c0 in enumerate(range(0, ni, BS)):
                c1 = min(ni, c0 + BS)
                Yf[c0:c1] = f.invL[j] @ W[c0:c1]
                W[c1:] -= f.L11[c1:, c0:c1] @ Yf[c0:c1]
            if len(f.bnd) and ni:
                if f.lowrank:
                    CL, ZL, _, _ = f.lowrank
                    B[f.bnd] -= CL @ (ZL @ Yf)
                else:
                    B[f.bnd] -= f.Lbi @ Yf
            Y[id(f)] = Yf
    for fronts in levels:  # root -> leaves
        for f in fronts:
            ni = len(f.int)
            W = Y[id(f)].copy()
            if len(f.bnd) and ni:
                if f.lowrank:
                    _, _, G, ZR = f.lowrank
                    W -= G @ (ZR @ B[f.bnd])
                else:
                    W -= f.Uib @ B[f.bnd]
            X = np.empty_like(W)
            starts = list(range(0, ni, BS))
            for j in reversed(range(len(starts))):
                c0, c1 = starts[j], min(ni, starts[j] + BS)
                X[c0:c1] = f.invU[j] @ W[c0:c1]
                W[:c0] -= f.U11[:c0, c0:c1] @ X[c0:c1]
            B[f.int] = X


def ldiv_block(levels, B, kc=32):
    """F^-1 B for an n x k block, `kc` columns at a time."""
    B = np.array(B, dtype=np.result_type(B.dtype, levels[0][0].L11.dtype), copy=True)
    vec = B.ndim == 1
    Bm = B.reshape(B.shape[0], -1)
    for c0 in range(0, Bm.shape[1], kc):
        blk = Bm[:, c0 : c0 + kc].copy()
        _chunk(levels, blk)
        Bm[:, c0 : c0 + kc] = blk
    return Bm[:, 0] if vec else Bm
