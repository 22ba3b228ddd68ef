"""NumPy statement of the pruned schedule of the sparse-right-hand-side solve (csrc/hs_solve_sparse.hip) over the fronts of
tests/ldiv_block_mirror.py: X = (op(F)^-1 B)[rows, :] for a sparse B.

Columns are processed in a stable sort by the post-order id of the front that owns their first stored row (empty columns last), `kc` at a
time.  Per chunk

  forward set  = the fronts that own a stored row of the chunk's columns, and their ancestors
  backward set = the fronts that own a wanted row, and their ancestors

the forward sweep of ldiv_block_mirror / ldiv_block_t_mirror runs over the forward set only, the backward sweep over the backward set
only, and a front of the backward set the forward sweep did not visit starts from y = 0.  A chunk of empty columns is not swept at all.
What is skipped is exactly zero in the full schedule, so the wanted rows carry its bits."""
import numpy as np

from ldiv_block_mirror import BS, Front


def fronts_with_parents(F, lowrank=False):
    """The levels of ldiv_block_mirror.fronts_by_level, every Front with `.parent` (a Front or None) and `.post` (post-order id)."""
    levels, post = {}, [0]

    def walk(x, lv, parent):
        f = Front(x, lv, lowrank)
        f.parent = parent
        for c in (x.left, x.right):
            if c is not None:
                walk(c, lv + 1, f)
        f.post = post[0]
        post[0] += 1
        levels.setdefault(lv, []).append(f)

    walk(F, 1, None)
    return [levels[lv] for lv in sorted(levels)]


def owners(levels, n):
    own = np.full(n, None, dtype=object)
    for fr in levels:
        for f in fr:
            own[f.int] = f
    return own


def closure(own, idx):
    out = set()
    for i in idx:
        f = own[i]
        while f is not None and id(f) not in out:
            out.add(id(f))
            f = f.parent
    return out


def column_order(own, B):
    """Stable sort of the columns of the CSC matrix B by the post-order id of the owner of their first stored row, empty columns last."""
    big = 1 << 60
    key = [own[B.indices[B.indptr[j]]].post if B.indptr[j + 1] > B.indptr[j] else big for j in range(B.shape[1])]
    return np.array(sorted(range(B.shape[1]), key=lambda j: key[j]), dtype=np.int64)


def _chunk_pruned(levels, B, fwd, bwd, trans):
    op = np.conj if trans == "H" else (lambda x: x)
    Y = {}
    for fronts in reversed(levels):  # leaves -> root
        for f in fronts:
            if id(f) not in fwd:
                continue
            ni = len(f.int)
            W = B[f.int[f.rperm]].copy() if trans == "N" else B[f.int].copy()
            Yf = np.empty_like(W)
            for j, c0 in enumerate(range(0, ni, BS)):
                c1 = min(ni, c0 + BS)
                if trans == "N":
                    Yf[c0:c1] = f.invL[j] @ W[c0:c1]
                    W[c1:] -= f.L11[c1:, c0:c1] @ Yf[c0:c1]
                else:
                    Yf[c0:c1] = op(f.invU[j]).T @ W[c0:c1]
                    W[c1:] -= op(f.U11[c0:c1, c1:]).T @ Yf[c0:c1]
            if len(f.bnd) and ni:
                if trans == "N":
                    B[f.bnd] -= f.lowrank[0] @ (f.lowrank[1] @ Yf) if f.lowrank else f.Lbi @ Yf
                else:
                    B[f.bnd] -= op(f.lowrank[3]).T @ (op(f.lowrank[2]).T @ Yf) if f.lowrank else op(f.Uib).T @ Yf
            Y[id(f)] = Yf
    for fronts in levels:  # root -> leaves
        for f in fronts:
            if id(f) not in bwd:
                continue
            ni = len(f.int)
            W = Y[id(f)].copy() if id(f) in Y else np.zeros((ni, B.shape[1]), dtype=B.dtype)  # not visited on the way up: y = 0
            if len(f.bnd) and ni:
                if trans == "N":
                    W -= f.lowrank[2] @ (f.lowrank[3] @ B[f.bnd]) if f.lowrank else f.Uib @ B[f.bnd]
                else:
                    W -= op(f.lowrank[1]).T @ (op(f.lowrank[0]).T @ B[f.bnd]) if f.lowrank else op(f.Lbi).T @ B[f.bnd]
            X = np.empty_like(W)
            starts = list(range(0, ni, BS))
            for j in reversed(range(len(starts))):
                c0, c1 = starts[j], min(ni, starts[j] + BS)
                if trans == "N":
                    X[c0:c1] = f.invU[j] @ W[c0:c1]
                    W[:c0] -= f.U11[:c0, c0:c1] @ X[c0:c1]
                else:
                    X[c0:c1] = op(f.invL[j]).T @ W[c0:c1]
                    W[:c0] -= op(f.L11[c0:c1, :c0]).T @ X[c0:c1]
            if trans == "N":
                B[f.int] = X
            else:
                B[f.int[f.rperm]] = X


def ldiv_sparse(levels, B, rows=None, trans="N", kc=32):
    """(op(F)^-1 B)[rows, :] for a scipy.sparse B; returns (X, stats) with stats = {"order", "forward": fronts visited per chunk,
    "backward": the same for the backward sweep, "fronts": fronts of the tree}."""
    assert trans in ("N", "T", "H")
    B = B.tocsc()
    B.sort_indices()
    n, k = B.shape
    own = owners(levels, n)
    order = column_order(own, B)
    dtype = np.result_type(B.dtype, levels[0][0].L11.dtype)
    allf = {id(f) for fr in levels for f in fr}
    bwd = allf if rows is None else closure(own, rows)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    X = np.zeros((len(rows), k), dtype=dtype)
    stats = {"order": order, "forward": [], "backward": [], "fronts": len(allf)}
    for c0 in range(0, k, kc):
        cols = order[c0 : c0 + kc]
        stored = np.concatenate([B.indices[B.indptr[j] : B.indptr[j + 1]] for j in cols])
        if not len(stored):  # zero columns: zero solution, no sweep
            stats["forward"].append(0)
            stats["backward"].append(0)
            continue
        fwd = closure(own, stored)
        blk = np.asarray(B[:, cols].toarray(), dtype=dtype)
        _chunk_pruned(levels, blk, fwd, bwd, trans)
        X[:, cols] = blk[rows]
        stats["forward"].append(len(fwd))
        stats["backward"].append(len(bwd))
    return X, stats
