"""NumPy statement of the adjoint-state sensitivities of hs_sens_* / hs_misfit_* (include/hs_solver.h, csrc/hs_sens.hip).

op(A) = A, A^T, A^H for trans = 0, 1, 2; X = op(A)^-1 B; W is the cotangent of a real objective (dJ = Re<W, dX>); Lam = op(A)^-H W and, for
every stored entry p = (i, j) of A,

    trans 0:  Lam = A^-H W               G_p = -sum_c Lam[i, c] conj(X[j, c])
    trans 1:  Lam = conj(A^-1 conj(W))   G_p = -sum_c Lam[j, c] conj(X[i, c])
    trans 2:  Lam = A^-1 W               G_p = -sum_c conj(Lam[j, c]) X[i, c]

so that d/ds Re<W, op(A + sE)^-1 B> at s = 0 equals Re sum_p E_p conj(G_p) for any E on the pattern of A.  `solve(M, t)` is any solver of
op_t(A) Y = M with t in "N", "T", "H" (SuperLU in the tests)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def canonical(A):
    """A as CSC with sorted indices: the order of the values the factorization was given."""
    A = sp.csc_matrix(A, copy=True)
    A.sort_indices()
    return A


def entry_index(A):
    """(i, j) of every stored entry of a canonical CSC matrix."""
    return A.indices.astype(np.int64), np.repeat(np.arange(A.shape[1], dtype=np.int64), np.diff(A.indptr))


def superlu_solver(A):
    lu = spla.splu(sp.csc_matrix(A))
    return lambda M, t: lu.solve(np.ascontiguousarray(M), trans=t)


def forward(solve, B, trans):
    return solve(B, "NTH"[trans])


def adjoint_state(solve, W, trans):
    if trans == 0:
        return solve(W, "H")
    if trans == 1:
        return np.conj(solve(np.conj(W), "N"))
    return solve(W, "N")


def pairs(A, Lam, X, trans):
    """The two factors of every entry's sum, (nnz x k) each: G = -(l * r).sum(axis=1)."""
    i, j = entry_index(A)
    if trans == 0:
        return Lam[i], np.conj(X[j])
    if trans == 1:
        return Lam[j], np.conj(X[i])
    return np.conj(Lam[j]), X[i]


def reduce(A, Lam, X, trans):
    """G on the pattern of A from the two blocks."""
    l, r = pairs(A, Lam, X, trans)
    return -(l * r).sum(axis=1)


def bound(A, Lam, X, trans):
    """S_p = sum_c |Lam| |X| over the index pairs of entry p."""
    l, r = pairs(A, Lam, X, trans)
    return (np.abs(l) * np.abs(r)).sum(axis=1)


def diag_positions(A):
    """Position of the stored (j, j) in the values of A, -1 where A stores no diagonal entry."""
    i, j = entry_index(A)
    pos = np.full(A.shape[0], -1, dtype=np.int64)
    d = np.flatnonzero(i == j)
    pos[j[d]] = d
    return pos


def diagonal(A, G):
    """The diagonal mode: G_jj for the stored (j, j), 0 elsewhere."""
    pos = diag_positions(A)
    out = np.zeros(A.shape[0], dtype=G.dtype)
    out[pos >= 0] = G[pos[pos >= 0]]
    return out


def sensitivity(A, solve, B, W, trans):
    """(G, X, Lam) with dense B, W."""
    X = forward(solve, B, trans)
    Lam = adjoint_state(solve, W, trans)
    return reduce(A, Lam, X, trans), X, Lam


def scatter(rows, R, n):
    W = np.zeros((n, R.shape[1]), dtype=R.dtype)
    W[np.asarray(rows)] = R
    return W


def misfit(A, solve, B, rows, D, trans):
    """(J, G, R): R = X[rows] - D, J_c = 0.5 ||R[:, c]||^2, G the sensitivity for W = scatter(R)."""
    X = forward(solve, B, trans)
    R = X[np.asarray(rows)] - D
    J = 0.5 * (np.abs(R) ** 2).sum(axis=0)
    Lam = adjoint_state(solve, scatter(rows, R, A.shape[0]), trans)
    return J, reduce(A, Lam, X, trans), R
