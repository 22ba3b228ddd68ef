"""NumPy restatement of the block 1-norm estimator of csrc/hs_condest.hip (Higham & Tisseur, SIAM J. Matrix Anal. Appl. 21(4), 2000,
Algorithm 2.4) and of the xGERFS error formulas, step for step: the same +-1 hash, the same tie-breaking, the same stopping tests.  B is
given by two callbacks, ``apply(X) = B X`` and ``apply_h(X) = B^H X``; with ``F.solve(., trans)`` callbacks it must reproduce what the
device returns for ``hs_normestinv`` (estimate and number of solves)."""
import numpy as np

M64 = (1 << 64) - 1


def _sm64(x):
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def col_key(seed, col, salt):
    return int(_sm64(np.uint64(int(_sm64(np.uint64(seed & M64)))) ^ np.uint64((salt << 8) & M64) ^ np.uint64(col)))


def pm1(n, col, salt, seed):
    """+-1 column `col` of draw `salt` (0: start block; k * 64 + attempt: re-drawn sign column of iteration k)."""
    bits = _sm64(np.uint64(col_key(seed, col, salt)) ^ np.arange(n, dtype=np.uint64)) & np.uint64(1)
    return np.where(bits == 1, -1.0, 1.0)


def _sign(Y):
    if np.iscomplexobj(Y):
        a = np.abs(Y)
        safe = np.where(a == 0, 1.0, a)
        return np.where(a == 0, 1.0 + 0j, Y.real / safe + 1j * (Y.imag / safe))
    return np.where(Y >= 0, 1.0, -1.0)


def normest1(apply, apply_h, n, t=2, itmax=5, seed=123, cplx=False):
    """Lower bound of ||B||_1; returns ``(est, nsolves)`` (nsolves = columns passed to the callbacks)."""
    dt = np.complex128 if cplx else np.float64
    X = np.empty((n, t), dtype=dt)
    X[:, 0] = 1.0
    for j in range(1, t):
        X[:, j] = pm1(n, j, 0, seed)
    X *= 1.0 / n
    est_old, ind_best, hist, ind = 0.0, -1, [], None
    S = S_old = None
    ns = 0
    k = 1
    while True:
        # 2. apply B
        Y = apply(X)
        ns += t
        norms = np.abs(Y).sum(axis=0)
        jmax = int(np.argmax(norms))  # the first maximum
        est = float(norms[jmax])
        if (est > est_old or k == 2) and k >= 2:
            ind_best = ind[jmax]
        if k >= 2 and est <= est_old:
            est = est_old
            break
        # 3. iteration limit
        est_old = est
        S_old = S
        if k > itmax:
            break
        # 4. signs
        S = _sign(Y)
        # 5. parallel columns (real only)
        if not cplx:
            if S_old is not None and all(np.any(np.abs(S[:, j] @ S_old) == n) for j in range(t)):
                break
            if t > 1:
                for j in range(t):
                    attempt = 1
                    while True:
                        par = any(abs(S[:, j] @ S[:, q]) == n for q in range(j))
                        if S_old is not None:
                            par = par or bool(np.any(np.abs(S[:, j] @ S_old) == n))
                        if not par or attempt > 32:
                            break
                        S[:, j] = pm1(n, j, k * 64 + attempt, seed)
                        attempt += 1
        # 6. apply B^H
        Z = apply_h(S)
        ns += t
        h = np.abs(Z).max(axis=1)
        if k >= 2 and h.max() == h[ind_best]:
            break
        # 7. next unit vectors: h descending, ties by ascending index, outside the history
        order = np.lexsort((np.arange(n), -h))
        hs = set(hist)
        if t > 1 and all(int(i) in hs for i in order[:t]):
            break
        ind = [int(i) for i in order if int(i) not in hs][:t]
        if len(ind) < t:
            break
        X = np.zeros((n, t), dtype=dt)
        X[ind, np.arange(t)] = 1.0
        hist += ind
        k += 1
    return est, ns


def normestinv(solve, n, trans=0, t=2, itmax=5, seed=123, cplx=False):
    """hs_normestinv: ``solve(X, tr)`` with tr in "N", "T", "C" applies F^-1, F^-T, F^-H to the columns of X."""
    def op(code, X):  # 0: F^-1, 1: F^-T, 2: F^-H, 3: conj(F)^-1
        if not cplx:
            code = {2: 1, 3: 0}.get(code, code)
        if code == 3:
            return np.conj(solve(np.conj(X), "N"))
        return solve(X, "NTC"[code])

    adj = {0: 2, 1: 3, 2: 0, 3: 1}[trans]
    return normest1(lambda X: op(trans, X), lambda X: op(adj, X), n, t, itmax, seed, cplx)


def cabs1(z):
    return np.abs(z.real) + np.abs(z.imag) if np.iscomplexobj(z) else np.abs(z)


EPS = 2.0 ** -53
SAFMIN = np.finfo(np.float64).tiny


def gerfs_berr(opA, x, b, nz):
    """xGERFS componentwise backward error of x for op(A) x = b (opA a dense or sparse matrix), with its residual and weights."""
    r = b - opA @ x
    absA = abs(opA.real) + abs(opA.imag) if np.iscomplexobj(opA) else abs(opA)
    w = cabs1(b) + absA @ cabs1(x)
    safe1 = nz * SAFMIN
    safe2 = safe1 / EPS
    ra = cabs1(r)
    ratio = np.where(w > safe2, ra / np.where(w > safe2, w, 1.0), (ra + safe1) / (w + safe1))
    return float(ratio.max()), r, w


def gerfs_ferr_exact(opA, x, r, w, nz):
    """The quantity xGERFS bounds, || |op(A)^-1| v ||_Inf / ||x||_Inf with v = |r| + nz eps w, computed exactly (dense)."""
    safe1 = nz * SAFMIN
    safe2 = safe1 / EPS
    v = np.where(w > safe2, cabs1(r) + nz * EPS * w, cabs1(r) + nz * EPS * w + safe1)
    Ainv = np.linalg.inv(np.asarray(opA.todense() if hasattr(opA, "todense") else opA))
    return float(np.max(np.abs(Ainv) @ v) / np.max(cabs1(x)))
