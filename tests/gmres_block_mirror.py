"""TEST INFRASTRUCTURE: a NumPy statement of the lockstep schedule of `hs_gmres_block_*` (csrc/hs_gmres_block.hip), and the plain single-vector
GMRES it must reproduce column by column.

`gmres_single` is the iteration of tests/gmres_mirror.py in NumPy: classical Gram-Schmidt with one re-orthogonalisation pass, Givens rotations,
right preconditioning x = x0 + Pr^-1 V y, tol = max(reltol ||r0||, abstol).

`gmres_block` runs nrhs such iterations together, the way the device does:

  * columns are processed in groups of `group` columns;
  * inside a group every n x nact object is a block whose column c is slot c; the basis vector j of slot c is V[c, j] (the device keeps
    V_j as an n x G block; here a slot's basis is contiguous so that its dot products are the very NumPy calls of `gmres_single`);
  * a step applies the preconditioner to the whole block of active slots ONCE (`prec` is a callable on n x nact blocks), multiplies by A once,
    orthogonalises every unfrozen slot against its own basis and updates its own H, cs, sn, g;
  * a slot whose estimate reaches its tolerance, that breaks down or that exhausts maxiter is FROZEN for the rest of the cycle: nothing of its
    state is written any more (its stale basis columns still travel through `prec` and A, and are ignored);
  * at the end of the cycle every slot solves its own triangular system with its own k_used, the updates go through ONE `prec` call, X receives
    them through the slot -> column map, and the true residuals are recomputed with one product;
  * the columns that go on are compacted into the leading slots.

`stats` (if given) receives prec_calls, column_applications, spmm, cycles, groups, max_active as hs_gmres_block_info reports them."""
import numpy as np
import scipy.sparse as sp


def _rotate(H, cs, sn, g, k):
    """apply the previous rotations to column k of H, then a new one annihilating H[k+1, k]; returns |g[k+1]|"""
    for i in range(k):
        t = cs[i] * H[i, k] + sn[i] * H[i + 1, k]
        H[i + 1, k] = -np.conj(sn[i]) * H[i, k] + cs[i] * H[i + 1, k]
        H[i, k] = t
    a, b = H[k, k], H[k + 1, k]
    den = np.sqrt(abs(a) ** 2 + abs(b) ** 2)
    if den == 0:
        cs[k], sn[k] = 1.0, 0.0
    else:
        cs[k], sn[k] = abs(a) / den, (a / abs(a) if abs(a) > 0 else 1.0) * np.conj(b) / den
    H[k, k] = cs[k] * a + sn[k] * b
    H[k + 1, k] = 0.0
    g[k + 1] = -np.conj(sn[k]) * g[k]
    g[k] = cs[k] * g[k]
    return abs(g[k + 1])


def _defaults(n, reltol, restart, maxiter):
    restart = min(20, n) if restart is None else int(restart)
    maxiter = n if maxiter is None else int(maxiter)
    reltol = float(np.sqrt(np.finfo(np.float64).eps)) if reltol is None else float(reltol)
    return reltol, restart, maxiter


def gmres_single(A, b, prec=None, reltol=None, abstol=0.0, restart=None, maxiter=None, x0=None):
    """Restarted GMRES on one vector; `prec(v)` applies the right preconditioner to a vector.  Returns (x, history dict)."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    dt = np.result_type(A.dtype, np.asarray(b).dtype, np.float64)
    if prec is not None:
        dt = np.result_type(dt, prec(np.zeros(n, dtype=dt)).dtype)
    reltol, restart, maxiter = _defaults(n, reltol, restart, maxiter)
    b = np.asarray(b, dtype=dt)
    x = np.zeros(n, dtype=dt) if x0 is None else np.array(x0, dtype=dt)
    r = b - A @ x if x0 is not None else b.copy()
    beta = float(np.linalg.norm(r))
    tol = max(reltol * beta, abstol)
    hist = [beta]
    it = 0
    converged = beta <= tol
    V = np.zeros((restart + 1, n), dtype=dt)
    while not converged and it < maxiter:
        V[0] = r / beta
        H = np.zeros((restart + 1, restart), dtype=dt)
        cs = np.zeros(restart, dtype=dt)
        sn = np.zeros(restart, dtype=dt)
        g = np.zeros(restart + 1, dtype=dt)
        g[0] = beta
        k_used = 0
        for k in range(restart):
            if it >= maxiter:
                break
            z = prec(V[k]) if prec is not None else V[k]
            w = A @ z
            h = V[: k + 1].conj() @ w
            w = w - V[: k + 1].T @ h
            h2 = V[: k + 1].conj() @ w
            w = w - V[: k + 1].T @ h2
            hn = float(np.linalg.norm(w))
            H[: k + 1, k] = h + h2
            H[k + 1, k] = hn
            if hn > 0:
                V[k + 1] = w / hn
            res = _rotate(H, cs, sn, g, k)
            it += 1
            k_used = k + 1
            hist.append(float(res))
            if res <= tol or hn == 0:
                converged = res <= tol
                break
        if k_used:
            y = np.linalg.solve(np.triu(H[:k_used, :k_used]), g[:k_used])
            upd = V[:k_used].T @ y
            x = x + (prec(upd) if prec is not None else upd)
        r = b - A @ x
        beta = float(np.linalg.norm(r))
        converged = converged or beta <= tol
        if k_used == 0:
            break
    return x, dict(resnorm=hist, isconverged=bool(converged), iters=it)


class _Col:
    def __init__(self, col):
        self.col = col
        self.it = 0
        self.conv = False
        self.frozen = False
        self.hist = []
        self.beta = self.tol = 0.0


def gmres_block(A, B, prec=None, reltol=None, abstol=0.0, restart=None, maxiter=None, X0=None, group=None, chunk=32, stats=None):
    """The lockstep schedule on the n x nrhs block B; `prec(Z)` applies the right preconditioner to an n x nact block.
    Returns (X, [history dict per column])."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    B = np.asarray(B)
    vec = B.ndim == 1
    B = B.reshape(n, -1)
    nrhs = B.shape[1]
    dt = np.result_type(A.dtype, B.dtype, np.float64)
    if prec is not None:
        dt = np.result_type(dt, prec(np.zeros((n, 1), dtype=dt)).dtype)
    reltol, m, maxiter = _defaults(n, reltol, restart, maxiter)
    B = B.astype(dt)
    X = np.zeros((n, nrhs), dtype=dt) if X0 is None else np.array(np.asarray(X0).reshape(n, -1), dtype=dt)
    allw = -(-nrhs // chunk) * chunk
    G = allw if group is None else min(allw, -(-int(group) // chunk) * chunk)
    G = max(min(G, nrhs), 1)
    st = dict(prec_calls=0, column_applications=0, spmm=0, cycles=0, groups=0, max_active=0)
    cols = []
    for g0 in range(0, nrhs, G):
        gc = min(G, nrhs - g0)
        st["groups"] += 1
        V = np.zeros((G, m + 1, n), dtype=dt)  # V[c, j]: basis vector j of slot c
        cur = [_Col(g0 + c) for c in range(gc)]
        cols += cur
        idx = [q.col for q in cur]
        if X0 is not None:
            R = B[:, idx] - A @ X[:, idx]
            st["spmm"] += 1
        else:
            R = B[:, idx].copy()
        for c, q in enumerate(cur):
            q.beta = float(np.linalg.norm(R[:, c]))
            q.tol = max(reltol * q.beta, abstol)
            q.hist.append(q.beta)
            q.conv = q.beta <= q.tol
        while True:
            keep = [c for c, q in enumerate(cur) if not q.conv and q.it < maxiter]
            if not keep:
                break
            R = R[:, keep]  # compaction: the columns that go on take the leading slots
            cur = [cur[c] for c in keep]
            nact = len(cur)
            idx = [q.col for q in cur]
            st["cycles"] += 1
            st["max_active"] = max(st["max_active"], nact)
            H = np.zeros((nact, m + 1, m), dtype=dt)
            cs = np.zeros((nact, m), dtype=dt)
            sn = np.zeros((nact, m), dtype=dt)
            g = np.zeros((nact, m + 1), dtype=dt)
            kused = [0] * nact
            for c, q in enumerate(cur):
                V[c, 0] = R[:, c] / q.beta
                g[c, 0] = q.beta
                q.frozen = False
            for k in range(m):
                if all(q.frozen for q in cur):
                    break
                Vk = V[:nact, k].T  # the block V_k of the active slots
                if prec is not None:
                    Z = prec(Vk)
                    st["prec_calls"] += 1
                    st["column_applications"] += nact
                else:
                    Z = Vk
                W = A @ Z
                st["spmm"] += 1
                for c, q in enumerate(cur):
                    if q.frozen:
                        continue
                    Vc = V[c, : k + 1]
                    w = np.ascontiguousarray(W[:, c])  # BLAS rounds a strided and a contiguous vector differently
                    h = Vc.conj() @ w
                    w = w - Vc.T @ h
                    h2 = Vc.conj() @ w
                    w = w - Vc.T @ h2
                    hn = float(np.linalg.norm(w))
                    H[c, : k + 1, k] = h + h2
                    H[c, k + 1, k] = hn
                    V[c, k + 1] = w / hn if hn > 0 else w
                    res = float(_rotate(H[c], cs[c], sn[c], g[c], k))
                    q.it += 1
                    kused[c] = k + 1
                    q.hist.append(res)
                    if res <= q.tol or hn == 0 or q.it >= maxiter:
                        q.conv = res <= q.tol
                        q.frozen = True
            U = np.zeros((n, nact), dtype=dt)
            for c in range(nact):
                ku = kused[c]
                y = np.linalg.solve(np.triu(H[c, :ku, :ku]), g[c, :ku])
                U[:, c] = V[c, :ku].T @ y
            if prec is not None:
                U = prec(U)
                st["prec_calls"] += 1
                st["column_applications"] += nact
            X[:, idx] += U
            R = B[:, idx] - A @ X[:, idx]
            st["spmm"] += 1
            for c, q in enumerate(cur):
                q.beta = float(np.linalg.norm(R[:, c]))
                q.conv = q.conv or q.beta <= q.tol
    if stats is not None:
        stats.update(st)
    chs = [dict(resnorm=q.hist, isconverged=bool(q.conv), iters=q.it) for q in cols]
    if vec:
        return X[:, 0], chs[0]
    return X, chs


def rhs_mix(n, k, cplx, seed=0):
    """The right-hand sides of the block tests: a constant vector, point sources, random vectors, one of them scaled by 1e6, and a zero
    column (index 3) -- columns that need different numbers of iterations."""
    rng = np.random.default_rng(seed)
    B = np.zeros((n, k), dtype=np.complex128 if cplx else np.float64)
    for c in range(k):
        if c == 0:
            B[:, c] = 1.0
        elif c == 3:
            pass
        elif c % 3 == 1:
            B[rng.integers(0, n), c] = 1.0 + (0.5j if cplx else 0.0)
        else:
            B[:, c] = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
    if k > 5:
        B[:, 5] *= 1e6
    return B
