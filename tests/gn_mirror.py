"""NumPy statement of the tangent-linear solves and Gauss-Newton products of hs_tangent_* / hs_gn_hessvec_* / hs_gn_diag_*
(include/hs_solver.h, csrc/hs_gn.hip), on top of tests/sens_mirror.py.

op(A) = A, A^T, A^H for trans = 0, 1, 2; X = op(A)^-1 B.  E is a perturbation on the stored pattern of A (nnz values in the order of A's
data, or n diagonal values: pattern "diag"), op(E) accordingly.

    tangent       dX(E) = d/ds op(A + sE)^-1 B at s = 0 = -op(A)^-1 op(E) X
    Gauss-Newton  J E = dX(E)[rows];  H E = J* J E = the G of sens_mirror for W = scatter(rows, J E)
    diagonal      Z = op(A)^-H S (S: the unit columns of rows), z2 = sum |Z|^2 over the columns, x2 = sum |X|^2 over the columns,
                  H_pp = z2[i] x2[j] (trans 0) or z2[j] x2[i] (trans 1, 2) for the stored p = (i, j)

`solve(M, t)` is any solver of op_t(A) Y = M with t in "N", "T", "H" (SuperLU in the tests)."""
import numpy as np
import scipy.sparse as sp

import sens_mirror as SM


def embed(A, E, pattern):
    """E as nnz values on the pattern of the canonical A: itself, or the diagonal values at the stored (j, j) (others count as 0)."""
    E = np.asarray(E)
    if pattern in ("A", 0):
        return E
    pos = SM.diag_positions(A)
    full = np.zeros(A.nnz, dtype=np.result_type(E.dtype, A.dtype))
    full[pos[pos >= 0]] = E[pos >= 0]
    return full


def restrict(A, G, pattern):
    """A result on the pattern of A as the pattern asks for it."""
    return G if pattern in ("A", 0) else SM.diagonal(A, G)


def op_matrix(A, E, trans, pattern="A"):
    M = sp.csc_matrix((embed(A, E, pattern), A.indices, A.indptr), shape=A.shape)
    return (M, M.T, M.conj().T)[trans].tocsr()


def tangent(A, solve, B, E, trans, pattern="A", X=None):
    """(dX, X)"""
    X = SM.forward(solve, B, trans) if X is None else X
    P = -(op_matrix(A, E, trans, pattern) @ X)
    return SM.forward(solve, P, trans), X


def gn_hessvec(A, solve, B, rows, E, trans, pattern="A", X=None):
    """(HE, JE, X)"""
    dX, X = tangent(A, solve, B, E, trans, pattern, X)
    JE = dX[np.asarray(rows)]
    Lam = SM.adjoint_state(solve, SM.scatter(rows, JE, A.shape[0]), trans)
    return restrict(A, SM.reduce(A, Lam, X, trans), pattern), JE, X


def rowsq(M, acc=None):
    """acc + sum over the columns, in order, of |M[:, c]|^2 as re * re + im * im: the chain of the device kernel."""
    acc = np.zeros(M.shape[0]) if acc is None else acc.copy()
    for c in range(M.shape[1]):
        col = M[:, c]
        acc = acc + ((col.real * col.real + col.imag * col.imag) if np.iscomplexobj(M) else col * col)
    return acc


def diag_from(A, z2, x2, trans, pattern="A"):
    i, j = SM.entry_index(A)
    a, b = (i, j) if trans == 0 else (j, i)
    return restrict(A, z2[a] * x2[b], pattern)


def gn_diag(A, solve, B, rows, trans, pattern="A", X=None):
    """(Hd, z2, x2)"""
    n = A.shape[0]
    X = SM.forward(solve, B, trans) if X is None else X
    S = SM.scatter(rows, np.eye(len(rows), dtype=X.dtype), n)
    Z = SM.adjoint_state(solve, S, trans)
    z2, x2 = rowsq(Z), rowsq(X)
    return diag_from(A, z2, x2, trans, pattern), z2, x2
