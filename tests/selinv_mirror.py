"""NumPy statement of what csrc/hs_selinv.hip computes, over a tree of (D, L, R, int, bnd) blocks such as the oracle's FactorNode
(oracle/hs_oracle.py: D = Aii, L = Abi D^-1, R = D^-1 Aib, 1-based index vectors):

  * logabsdet: det(A) = prod over fronts of det(D) (times det(S) of a root that keeps a boundary) -- the Gauss transforms between
    fronts are unit block-triangular;
  * selected inversion, root to leaves: with Z = A^-1 and Zbb = Z[bnd, bnd] of a front known,
        Z[int, bnd] = -R Zbb,   Z[bnd, int] = -Zbb L,   Z[int, int] = D^-1 + R Zbb L,
    and a child's Zbb is read out of its parent's finished block (its boundary is a subset of the parent's [int; bnd]);
  * entry ownership: the stored entry (r, c) of A belongs to the front that eliminates whichever of r, c goes first; it must lie inside
    that front's [int; bnd] x [int; bnd] block, or the selected inverse would have a hole there.

The device runs the same recurrence on the pivoted LU factors (R = U^-1 Uib, L = Lbi L^-1 P); the mirror uses dense solves."""
import numpy as np


def dense_d(D):
    """The interior block as a dense matrix (the oracle keeps a branch's D as the 2 x 2 block factorization of blockmatrix.jl:115-120)."""
    B = getattr(D, "B", None)
    if B is None:
        return np.asarray(D)
    A22 = B.A22 + B.A21 @ np.linalg.solve(B.A11, B.A12) if B.A11.shape[0] else B.A22
    return np.block([[B.A11, B.A12], [B.A21, A22]])


def _dense(M):
    return M.dense() if hasattr(M, "dense") else np.asarray(M)


def nodes_of(F):
    """Fronts of the tree, parents before children."""
    out, stack = [], [F]
    while stack:
        x = stack.pop()
        out.append(x)
        stack += [c for c in (x.left, x.right) if c is not None]
    return out


def root_schur(F):
    """S of the root in the order of F.bnd (the oracle stores S[perm, perm], perm = [int_loc; bnd_loc])."""
    perm = np.concatenate([F.int_loc, F.bnd_loc]).astype(np.int64) - 1
    S = _dense(F.S)
    out = np.empty_like(S)
    out[np.ix_(perm, perm)] = S
    return out


def logabsdet(F):
    """(log|det|, sign) of the factored matrix; sign is +-1.0 or a unit complex number (numpy.linalg.slogdet's convention)."""
    la, sign = 0.0, 1.0
    blocks = [dense_d(x.D) for x in nodes_of(F) if len(x.int)]
    if len(F.bnd):
        blocks.append(root_schur(F))
    for D in blocks:
        s, l = np.linalg.slogdet(D)
        la += l
        sign = sign * s
        if np.iscomplexobj(sign) and sign != 0:
            sign = sign / abs(sign)  # renormalised product: never drifts off the unit circle
    return la, sign


def selinv(F, n):
    """Dense n x n array holding (A^-1)[i, j] wherever the recurrence produces it and NaN elsewhere."""
    cplx = any(np.iscomplexobj(dense_d(x.D)) for x in nodes_of(F))
    Z = np.full((n, n), np.nan, dtype=np.complex128 if cplx else np.float64)
    if len(F.bnd):
        b = F.bnd - 1
        Z[np.ix_(b, b)] = np.linalg.inv(root_schur(F))
    for x in nodes_of(F):  # parents first: Z[bnd, bnd] of x is complete when x is reached
        i, b = x.int - 1, x.bnd - 1
        Dinv = np.linalg.inv(dense_d(x.D)) if len(i) else np.zeros((0, 0))
        if len(b) == 0:
            Z[np.ix_(i, i)] = Dinv
            continue
        Zbb = Z[np.ix_(b, b)]
        assert not np.isnan(Zbb).any(), "a front's boundary block must come complete from its ancestors"
        R, L = _dense(x.R), _dense(x.L)
        Z[np.ix_(i, b)] = -R @ Zbb
        Z[np.ix_(b, i)] = -Zbb @ L
        Z[np.ix_(i, i)] = Dinv + R @ Zbb @ L
    return Z


def entry_owners(A, fronts):
    """Owner of every stored entry of the CSC matrix A.  `fronts`: list of (int, bnd, level) with 0-based index arrays, level growing
    towards the leaves.  Returns (owner, inside): owner[e] = index of the front that eliminates the earlier of the entry's row and column
    (-1: the two are eliminated by different fronts of one level, i.e. in unrelated subtrees), inside[e] = the entry's row and column are
    both in the owner's [int; bnd]."""
    A = A.tocsc()
    n = A.shape[0]
    elim = np.full(n, -1)
    level = np.array([lv for _, _, lv in fronts])
    for f, (i, _, _) in enumerate(fronts):
        assert (elim[i] == -1).all(), "a DOF is interior to two fronts"
        elim[i] = f
    assert (elim >= 0).all(), "a DOF is interior to no front"
    cols = np.repeat(np.arange(n), np.diff(A.indptr))
    rows = A.indices
    fr, fc = elim[rows], elim[cols]
    owner = np.where(level[fr] >= level[fc], fr, fc)
    owner[(fr != fc) & (level[fr] == level[fc])] = -1
    inside = np.zeros(len(rows), dtype=bool)
    member = np.zeros(n, dtype=bool)
    for f, (i, b, _) in enumerate(fronts):
        e = np.flatnonzero(owner == f)
        member[i] = True
        member[b] = True
        inside[e] = member[rows[e]] & member[cols[e]]
        member[i] = False
        member[b] = False
    return owner, inside


def fronts_of(F):
    """(int, bnd, level) of every front of an oracle FactorNode / NDNode tree, 0-based."""
    out, stack = [], [(F, 1)]
    while stack:
        x, lv = stack.pop()
        out.append((np.asarray(x.int, dtype=np.int64) - 1, np.asarray(x.bnd, dtype=np.int64) - 1, lv))
        stack += [(c, lv + 1) for c in (x.left, x.right) if c is not None]
    return out
