"""NumPy statement of hs_eigs_gen_* (csrc/hs_eigs.hip): the loop of tests/eigs_mirror.py, unchanged, on the operator C = op(F)^-1 op(M) of
the pencil (A, M), F a factorization of A_s = A - sigma M; theta the eigenvalues of C of largest modulus, lambda = sigma + 1 / theta.

inner = "euclid": the loop as it is; only `solve` changes (it multiplies by op(M) first).  inner = "M": the same loop with an orth_block that
takes every inner product against MW = op(M) W, recomputed after every change of W, so that the basis is op(M)-orthonormal; the vectors come
back with x^H op(M) x = 1.

Below: the test pencils with known spectra that tests/test_eigs_gen_host.py and tests/test_eigs_gen_gpu.py share."""
import types

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import eigs_mirror as EM
from eigs_mirror import convection, convection_spectrum, poisson, poisson_spectrum


def m_orth_block(opM):
    """orth_block of eigs_mirror.py in the op(M) inner product"""

    def orth_block(V, k, p, rng, log):
        n = V.shape[0]
        W = V[:, k:k + p]
        Racc = np.eye(p, dtype=V.dtype)
        Hacc = np.zeros((k, p), dtype=V.dtype)
        for attempt in range(p + 1):
            for _pass in range(2):
                if k:
                    h = V[:, :k].conj().T @ (opM @ W)
                    W -= V[:, :k] @ h
                    Hacc += h @ Racc
                    log["orth"] += 1
            bad = -1
            for _round in range(2):
                Gm = W.conj().T @ (opM @ W)
                if k == 0 and attempt == 0 and _round == 0 and not np.all(np.real(np.diag(Gm)) > 0):
                    raise ValueError("inner = 'M' needs a Hermitian positive definite M: v^H op(M) v <= 0 on the start block")
                R, Rinv, bad = EM.chol_inv(Gm)
                if bad >= 0:
                    break
                W[:] = W @ Rinv
                Racc = R @ Racc
            if bad < 0:
                return Hacc, Racc
            v = rng.standard_normal(n)
            W[:, bad] = v / np.linalg.norm(v)
            Racc[bad, :] = 0.0
            log["replaced"] += 1
        raise ArithmeticError("orth_block: more replacements than columns")

    return orth_block


def eigs_gen_mirror(solve, opM, n, dtype, inner="euclid", **kw):
    """(theta, X, log) of eigs_mirror for C = solve(opM @ .); `solve` stands for op(F)^-1, opM for op(M) (None: the identity).  log gains
    nmprod, the products with op(M) the expansions made."""
    if opM is None:
        return EM.eigs_mirror(solve, n, dtype, **kw)
    count = {"n": 0}

    def gsolve(B):
        count["n"] += 1
        return solve(opM @ B)

    loop = EM.eigs_mirror
    if inner == "M":  # the same code object, run with the M-inner orth_block for its global name
        loop = types.FunctionType(EM.eigs_mirror.__code__, {**vars(EM), "orth_block": m_orth_block(opM)}, "eigs_mirror", EM.eigs_mirror.__defaults__)
    elif inner != "euclid":
        raise ValueError(inner)
    theta, X, log = loop(gsolve, n, dtype, **kw)
    if inner == "M":
        X = X / np.sqrt(np.real(np.sum(X.conj() * (opM @ X), axis=0)))
    log["nmprod"] = count["n"]
    return theta, X, log


# ---- test pencils ---------------------------------------------------------------------------------------------------------------------------
def _eye(n):
    return sp.identity(n, format="csc")


def pencil_S(shape):
    """Hermitian definite, M on A's pattern: (P, I + P/4), spectrum a / (1 + a/4), lambda_min(M) >= 1"""
    P, a = poisson(shape), poisson_spectrum(shape)
    return P, (_eye(P.shape[0]) + P / 4).tocsc(), np.sort(a / (1 + a / 4))


def pencil_W(shape):
    """M wider than A's pattern: (P, (I + P/4)^2), spectrum a / (1 + a/4)^2"""
    P, a = poisson(shape), poisson_spectrum(shape)
    B = (_eye(P.shape[0]) + P / 4).tocsc()
    return P, (B @ B).tocsc(), a / (1 + a / 4) ** 2


def pencil_N(shape, pe=8.0):
    """real non-symmetric with complex pairs: (Pc, I + Pc/4), spectrum ac / (1 + ac/4); the eigenvectors are those of Pc"""
    Pc, ac = convection(shape, pe), convection_spectrum(shape, pe)
    return Pc, (_eye(Pc.shape[0]) + Pc / 4).tocsc(), ac / (1 + ac / 4)


def pencil_Z(shape, seed=11):
    """singular M: (P, diag(rho)), rho in [1, 2) with every 7th entry 0; the finite eigenvalues nearest 0 from scipy's eigsh"""
    P = poisson(shape)
    rho = 1.0 + np.random.default_rng(seed).random(P.shape[0])
    rho[::7] = 0.0
    M = sp.diags(rho, format="csc")
    ref = spla.eigsh(P, 6, M=M, sigma=0, tol=0, return_eigenvectors=False)
    return P, M, np.sort(ref)


def pencil_H(shape=(10, 9, 8), seed=12):
    """ComplexF64: (poisson - 1.5 I + i diag(d), diag(rho)), d in [0.1, 0.3], rho in [1, 2); the six eigenvalues nearest 0 from scipy's eigs
    and the condition number of the eigenvectors of M^-1 A from a dense eig"""
    rng = np.random.default_rng(seed)
    P = poisson(shape)
    n = P.shape[0]
    d, rho = 0.1 + 0.2 * rng.random(n), 1.0 + rng.random(n)
    A = (P - 1.5 * _eye(n) + 1j * sp.diags(d)).tocsc()
    M = sp.diags(rho, format="csc")
    ref = spla.eigs(A, 6, M=M.astype(complex), sigma=0, tol=0, return_eigenvectors=False)
    condX = np.linalg.cond(np.linalg.eig(A.toarray() / rho[:, None])[1])
    return A, M, ref, condX


def m_residual(op_As, op_M, X, mu):
    """||op(A_s) X - (op(M) X) diag(mu)||_2 by column"""
    return np.linalg.norm(op_As @ X - (op_M @ X) * mu, axis=0)
