"""NumPy statement of the loop of hs_eigs_* (csrc/hs_eigs.hip): block Arnoldi on op(F)^-1 with thick restart in Krylov-decomposition form.

State: an orthonormal basis V (n x (m + p)) and G ((m + p) x m) with  op(F)^-1 V[:, :m] = V G.  `solve(B)` stands for op(F)^-1 B (SuperLU in
the host tests).  The dense eigenproblem of H = G[:m] is numpy.linalg.eig here and csrc/hs_small_eig.h in the library; the start block and
the replacement columns come from numpy's generator here and from the library's counter-based one there, so the two agree in what they
converge to and in the order of the steps, not in bits.

Below the loop: the test matrices with known spectra that tests/test_eigs_host.py and tests/test_eigs_gpu.py share."""
import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -53
DEF_TOL = (64 * EPS) ** 2  # a Cholesky pivot at or below this times the largest diagonal entry of the Gram matrix: a dependent column


def chol_inv(Gm):
    """(R, R^-1, first deficient column or -1) of the Gram matrix Gm = R^H R, R upper (launch_eigs_chol_inv)."""
    p = Gm.shape[0]
    R = np.zeros_like(Gm)
    dmax = max(float(np.max(np.real(np.diag(Gm)))), 0.0)
    for c in range(p):
        for i in range(c):
            R[i, c] = (Gm[i, c] - np.vdot(R[:i, i], R[:i, c])) / R[i, i]
        piv = float(np.real(Gm[c, c] - np.vdot(R[:c, c], R[:c, c])))
        if not piv > DEF_TOL * dmax:
            return R, None, c
        R[c, c] = np.sqrt(piv)
    return R, np.linalg.inv(R), -1


def orth_block(V, k, p, rng, log):
    """Orthonormalise W = V[:, k:k+p] against V[:, :k] and in itself, in place; returns (h, R) with W_in = V[:, :k] h + W_out R."""
    n = V.shape[0]
    W = V[:, k:k + p]
    Racc = np.eye(p, dtype=V.dtype)
    Hacc = np.zeros((k, p), dtype=V.dtype)
    for _ in range(p + 1):
        for _pass in range(2):  # classical Gram-Schmidt, twice
            if k:
                h = V[:, :k].conj().T @ W
                W -= V[:, :k] @ h
                Hacc += h @ Racc
                log["orth"] += 1
        bad = -1
        for _round in range(2):  # CholQR2
            R, Rinv, bad = chol_inv(W.conj().T @ W)
            if bad >= 0:
                break
            W[:] = W @ Rinv
            Racc = R @ Racc
        if bad < 0:
            return Hacc, Racc
        v = rng.standard_normal(n)
        W[:, bad] = v / np.linalg.norm(v)
        Racc[bad, :] = 0.0  # the dependent remainder is dropped: no original column has a component along the new vector through it
        log["replaced"] += 1
    raise ArithmeticError("orth_block: more replacements than columns")


def split_pairs(theta, cplx_h):
    """pair[c]: 0 a real Ritz value (or a ComplexF64 handle), +1 the first of a conjugate pair, -1 the second; theta sorted, pairs adjacent."""
    m = len(theta)
    pair = np.zeros(m, dtype=int)
    if cplx_h:
        return pair
    scale = max(float(np.max(np.abs(theta))), 1e-300)
    c = 0
    while c < m:
        if abs(theta[c].imag) > 64 * EPS * scale and c + 1 < m:
            pair[c], pair[c + 1] = 1, -1
            c += 2
        else:
            c += 1
    return pair


def sort_ritz(theta, Y, cplx_h):
    """|theta| descending; for a real H the two members of a conjugate pair adjacent, the one with the negative imaginary part first."""
    order = list(np.argsort(-np.abs(theta), kind="stable"))
    if not cplx_h:
        scale = max(float(np.max(np.abs(theta))), 1e-300)
        out, used = [], set()
        for i in order:
            if i in used:
                continue
            used.add(i)
            if abs(theta[i].imag) > 64 * EPS * scale:
                rest = [j for j in order if j not in used]
                j = min(rest, key=lambda q: abs(theta[q] - np.conj(theta[i])))
                used.add(j)
                out += [i, j] if theta[i].imag < 0 else [j, i]  # lambda = sigma + 1 / theta: the positive imaginary part first
            else:
                out.append(i)
        order = out
    return theta[order], Y[:, order]


def real_phase(y):
    """the eigenvector of a real eigenvalue of a real matrix as a real vector: the phase that makes its largest entry real"""
    i = int(np.argmax(np.abs(y)))
    return np.real(y * (np.conj(y[i]) / abs(y[i])))


def eigs_mirror(solve, n, dtype, nev=6, ncv=48, block=8, tol=1e-10, maxrestart=100, v0=None, seed=0):
    """Returns (theta, X, log): the nout Ritz values of op(F)^-1 of largest modulus (lambda = sigma + 1 / theta), their unit vectors as
    complex columns, and the counters."""
    cplx_h = np.dtype(dtype).kind == "c"
    p = block
    rng = np.random.default_rng(seed)
    log = {"restarts": 0, "nsolves": 0, "orth": 0, "replaced": 0, "nconv": 0}
    V = np.zeros((n, ncv + p + 1), dtype=dtype)
    G = np.zeros((ncv + p + 1, ncv + 1), dtype=dtype)
    V[:, :p] = rng.standard_normal((n, p)) if v0 is None else v0
    orth_block(V, 0, p, rng, log)
    m, lim = 0, ncv
    while True:
        while m + p <= lim:  # expansion of block m
            V[:, m + p:m + 2 * p] = solve(V[:, m:m + p])
            log["nsolves"] += 1
            h, R = orth_block(V, m + p, p, rng, log)
            G[:m + p, m:m + p] = h
            G[m + p:m + 2 * p, m:m + p] = R
            m += p
        H, B = G[:m, :m], G[m:m + p, :m]
        theta, Y = np.linalg.eig(H)
        theta, Y = sort_ritz(theta, Y / np.linalg.norm(Y, axis=0), cplx_h)
        pair = split_pairs(theta, cplx_h)
        est = np.linalg.norm(B @ Y, axis=0) / np.abs(theta)
        nout = nev + 1 if pair[nev - 1] == 1 else nev
        log["nconv"] = int(np.sum(est[:nout] <= tol))
        if log["nconv"] == nout or log["restarts"] >= maxrestart:
            break
        t = max(1, (ncv - nev - p) // p)
        keep = max(m - t * p, 1)
        lim = ncv
        if pair[keep - 1] == 1:  # a conjugate pair stays whole: one more vector (and one more basis column), or one fewer where n forbids it
            more = ncv + 1 + p <= n and keep + 1 < m
            keep += 1 if more else -1
            lim = ncv + 1 if more else ncv
        if cplx_h:
            Z = Y[:, :keep]
        else:
            Z = np.zeros((m, keep))
            for c in range(keep):
                Z[:, c] = real_phase(Y[:, c]) if pair[c] == 0 else (Y[:, c].real if pair[c] == 1 else Y[:, c - 1].imag)
        Q = np.linalg.qr(Z)[0]
        Gn = np.vstack([Q.conj().T @ H @ Q, B @ Q])
        V[:, :keep] = V[:, :m] @ Q
        V[:, keep:keep + p] = V[:, m:m + p]
        G[:] = 0
        G[:keep + p, :keep] = Gn
        m = keep
        log["restarts"] += 1
    X = V[:, :m] @ Y[:, :nout]
    X = X / np.linalg.norm(X, axis=0)
    log["est"] = est[:nout]
    return theta[:nout], X, log


# ---- test matrices with known spectra ---------------------------------------------------------------------------------------------------
def tri(n, lo, d, up):
    return sp.diags([lo * np.ones(n - 1), d * np.ones(n), up * np.ones(n - 1)], [-1, 0, 1], format="csr")


def kron3(fz, fy, fx):  # x fastest, as hs.problems.grid_matrix
    return sp.kron(sp.kron(fz, fy), fx, format="csc")


def poisson(shape):
    nx, ny, nz = shape
    I = sp.identity
    return (kron3(I(nz), I(ny), tri(nx, -1, 2, -1)) + kron3(I(nz), tri(ny, -1, 2, -1), I(nx)) + kron3(tri(nz, -1, 2, -1), I(ny), I(nx))).tocsc()


def lap_eigs(n):
    return 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))


def poisson_spectrum(shape):
    nx, ny, nz = shape
    return np.sort(np.add.outer(np.add.outer(lap_eigs(nz), lap_eigs(ny)), lap_eigs(nx)).ravel())


def convection(shape, pe):
    """Poisson plus x-only central convection: the x-factor tridiag(-1 - pe/2, 2, -1 + pe/2) has the eigenvalues
    2 + 2 i sqrt(pe^2/4 - 1) cos(k pi / (nx + 1)) for pe > 2."""
    nx, ny, nz = shape
    return (poisson(shape) + kron3(sp.identity(nz), sp.identity(ny), tri(nx, -pe / 2, 0.0, pe / 2))).tocsc()


def convection_spectrum(shape, pe):
    nx, ny, nz = shape
    fx = 2.0 + 2.0j * np.sqrt(pe * pe / 4 - 1.0) * np.cos(np.arange(1, nx + 1) * np.pi / (nx + 1))
    return np.add.outer(np.add.outer(lap_eigs(nz), lap_eigs(ny)), fx).ravel()


def nearest(spec, sigma, k):
    return spec[np.argsort(np.abs(spec - sigma), kind="stable")[:k]]


def match(lam, ref):
    """the largest distance of a computed eigenvalue from the nearest reference value, and the reverse"""
    lam, ref = np.asarray(lam, dtype=complex), np.asarray(ref, dtype=complex)
    d = np.abs(lam[:, None] - ref[None, :])
    return max(d.min(axis=1).max(), d.min(axis=0).max())
