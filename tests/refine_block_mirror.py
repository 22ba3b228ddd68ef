"""NumPy restatement of the lockstep schedule of csrc/hs_refine_block.hip (hs_ldiv_refine_block_*): column groups, freezing, compaction into
the leading slots, the xGERFS stopping rule, the per-column state machine of the Higham-Tisseur estimator and the order of the block
applications.  The single-column definitions (residual, weights, guarded ratio, the +-1 hash, signs, tie-breaking) are those of
tests/normest_mirror.py.

``solve(block, tr)`` with tr in "N", "T", "C" applies F^-1, F^-T, F^-H to the columns of ``block`` (one block application); ``opA`` is op(A)
as a scipy CSR (or dense) matrix; ``trans`` in 0, 1, 2 names op.  :func:`refine_single` is the column-by-column loop of hs_ldiv_refine_* on
the same callbacks: with a ``solve`` whose columns do not depend on each other the two agree exactly."""
import numpy as np

import normest_mirror as M

EST_T = 2       # estimator columns per right-hand side: t = min(2, n)
EST_ITMAX = 5   # estimator iterations


def _ops(solve, trans, cplx):
    """(apply op_fwd(F)^-1, apply op_adj(F)^-1) of the estimator of diag(v) op(F)^-H: fwd = adj(trans), adj = trans (codes of hs_condest.hip)."""
    def op(code, X):  # 0: F^-1, 1: F^-T, 2: F^-H, 3: conj(F)^-1
        if not cplx:
            code = {2: 1, 3: 0}.get(code, code)
        if code == 3:
            return np.conj(solve(np.conj(X), "N"))
        return solve(X, "NTC"[code])

    adj = {0: 2, 1: 3, 2: 0, 3: 1}[trans]
    return (lambda X: op(adj, X)), (lambda X: op(trans, X))


def _weights(r, w, nz):
    safe1 = nz * M.SAFMIN
    safe2 = safe1 / M.EPS
    return np.where(w > safe2, M.cabs1(r) + nz * M.EPS * w, M.cabs1(r) + nz * M.EPS * w + safe1)


def refine_single(solve, opA, B, nz, trans=0, itmax=5, ferr=True, seed=123):
    """hs_ldiv_refine_*: one column after the other, every solve a single-column call."""
    cplx = np.iscomplexobj(B)
    n, nrhs = B.shape
    fwd, adj = _ops(solve, trans, cplx)
    tr = "NTC"[trans]
    X = np.zeros_like(B)
    berr, fe, steps = np.zeros(nrhs), np.zeros(nrhs), np.zeros(nrhs, dtype=np.int64)
    for c in range(nrhs):
        b = B[:, c]
        x = solve(b[:, None].copy(), tr)[:, 0]
        lst, cnt = 3.0, 0
        while True:
            be, r, w = M.gerfs_berr(opA, x, b, nz)
            if not (be > M.EPS and 2.0 * be <= lst and cnt < itmax):
                break
            x = x + solve(r[:, None].copy(), tr)[:, 0]
            lst = be
            cnt += 1
        X[:, c], berr[c], steps[c] = x, be, cnt
        if ferr:
            v = _weights(r, w, nz)[:, None]
            est, _ = M.normest1(lambda Y: v * fwd(Y), lambda Y: adj(v * Y), n, min(EST_T, n), EST_ITMAX, seed, cplx)
            xn = M.cabs1(x).max()
            fe[c] = est / xn if xn != 0.0 else est
    return X, berr, (fe if ferr else None), steps


class _Est:
    """State of one column's estimator (normest1 of tests/normest_mirror.py, one object per right-hand side)."""

    def __init__(self, n, t, seed, dt):
        self.X = np.empty((n, t), dtype=dt)
        self.X[:, 0] = 1.0
        for j in range(1, t):
            self.X[:, j] = M.pm1(n, j, 0, seed)  # the keys do not depend on the right-hand side
        self.X *= 1.0 / n
        self.est = self.est_old = 0.0
        self.ind, self.ind_best, self.hist = None, -1, []
        self.S = self.S_old = None


def _estimate_lockstep(fwd, adj, V, seed, cplx, count):
    """Every column of V its own Algorithm 2.4 on diag(v) op_fwd(F)^-1 / op_adj(F)^-1 diag(v); the active estimators share ONE block
    application per half-step, compacted into the leading slots.  Returns the estimates."""
    n, gc = V.shape
    t = min(EST_T, n)
    dt = np.complex128 if cplx else np.float64
    E = [_Est(n, t, seed, dt) for _ in range(gc)]
    act = list(range(gc))
    k = 1
    while act:
        # 2. Y = B X for all active estimators: one application of op_fwd(F)^-1 on nact * t columns
        Yb = fwd(np.hstack([E[c].X for c in act]))
        count("est", len(act) * t)
        nxt = []
        for a, c in enumerate(act):
            q = E[c]
            q.Y = V[:, [c]] * Yb[:, a * t:(a + 1) * t]
            norms = np.abs(q.Y).sum(axis=0)
            jmax = int(np.argmax(norms))
            q.est = float(norms[jmax])
            if (q.est > q.est_old or k == 2) and k >= 2:
                q.ind_best = q.ind[jmax]
            if k >= 2 and q.est <= q.est_old:
                q.est = q.est_old
                continue
            # 3. iteration limit
            q.est_old = q.est
            q.S_old = q.S
            if k > EST_ITMAX:
                continue
            nxt.append(c)
        act = nxt
        # 4. signs, 5. parallel columns (real only; the device batches the +-1 dot products, a round of redraws per synchronisation)
        nxt = []
        for c in act:
            q = E[c]
            S = M._sign(q.Y)
            if not cplx:
                if q.S_old is not None and all(np.any(np.abs(S[:, j] @ q.S_old) == n) for j in range(t)):
                    continue
                if t > 1:
                    for j in range(t):
                        attempt = 1
                        while True:
                            par = any(abs(S[:, j] @ S[:, p]) == n for p in range(j))
                            if q.S_old is not None:
                                par = par or bool(np.any(np.abs(S[:, j] @ q.S_old) == n))
                            if not par or attempt > 32:
                                break
                            S[:, j] = M.pm1(n, j, k * 64 + attempt, seed)
                            attempt += 1
            q.S = S
            nxt.append(c)
        act = nxt
        if not act:
            break
        # 6. Z = B^H S for all active estimators: one application of op_adj(F)^-1
        Zb = adj(np.hstack([V[:, [c]] * E[c].S for c in act]))
        count("est", len(act) * t)
        nxt = []
        for a, c in enumerate(act):
            q = E[c]
            h = np.abs(Zb[:, a * t:(a + 1) * t]).max(axis=1)
            if k >= 2 and h.max() == h[q.ind_best]:
                continue
            # 7. next unit vectors: h descending, ties by ascending index, outside the column's own history
            order = np.lexsort((np.arange(n), -h))
            hs = set(q.hist)
            if t > 1 and all(int(i) in hs for i in order[:t]):
                continue
            ind = [int(i) for i in order if int(i) not in hs][:t]
            if len(ind) < t:
                continue
            q.ind = ind
            q.X = np.zeros((n, t), dtype=dt)
            q.X[ind, np.arange(t)] = 1.0
            q.hist += ind
            nxt.append(c)
        act = nxt
        k += 1
    return np.array([q.est for q in E])


def refine_block(solve, opA, B, nz, trans=0, itmax=5, ferr=True, group=None, chunk=32, seed=123, stats=None):
    """hs_ldiv_refine_block_*: returns ``(X, berr, ferr, steps)``.  ``group``: the group width G (default: all columns, rounded up to the chunk
    width like the device; any positive width is taken as given so that a test can use 1 or 2).  ``stats`` (a dict) receives "refine_solves"
    and "est_solves" (block applications), "col_apps" / "est_col_apps" (columns summed over them), "chunks" (sum of ceil(nact / chunk)),
    "residuals", "groups", "max_active"."""
    cplx = np.iscomplexobj(B)
    n, nrhs = B.shape
    fwd, adj = _ops(solve, trans, cplx)
    tr = "NTC"[trans]
    st = stats if stats is not None else {}
    for key in ("refine_solves", "est_solves", "col_apps", "est_col_apps", "chunks", "residuals", "groups", "max_active"):
        st[key] = 0

    def count(kind, cols):
        st["refine_solves" if kind == "ref" else "est_solves"] += 1
        st["col_apps"] += cols
        st["chunks"] += -(-cols // chunk)
        if kind == "est":
            st["est_col_apps"] += cols

    G = group if group else max(nrhs, 1)
    X = np.zeros_like(B)
    berr, fe, steps = np.zeros(nrhs), np.zeros(nrhs), np.zeros(nrhs, dtype=np.int64)
    for g0 in range(0, nrhs, G):
        gc = min(G, nrhs - g0)
        st["groups"] += 1
        cols = list(range(g0, g0 + gc))  # slot -> column
        X[:, cols] = solve(B[:, cols].copy(), tr)
        count("ref", gc)
        lst = {c: 3.0 for c in cols}
        cnt = {c: 0 for c in cols}
        V = np.zeros((n, gc))
        while cols:
            st["residuals"] += 1
            st["max_active"] = max(st["max_active"], len(cols))
            R = np.zeros((n, len(cols)), dtype=B.dtype)  # one fused pass: r, w, v and the ratio of every active column
            ratios = []
            for s, c in enumerate(cols):
                be, r, w = M.gerfs_berr(opA, X[:, c], B[:, c], nz)
                R[:, s] = r
                V[:, c - g0] = _weights(r, w, nz)
                ratios.append(be)
            nxt, src = [], []
            for s, c in enumerate(cols):  # the host reads nact ratios
                be = ratios[s]
                if be > M.EPS and 2.0 * be <= lst[c] and cnt[c] < itmax:
                    lst[c] = be
                    cnt[c] += 1
                    nxt.append(c)
                    src.append(s)
                else:  # frozen: x, berr and steps are final
                    berr[c], steps[c] = be, cnt[c]
            if not nxt:
                break
            D = solve(R[:, src].copy(), tr)  # the columns that go on, compacted into the leading slots
            count("ref", len(nxt))
            X[:, nxt] += D
            cols = nxt
        if ferr:
            est = _estimate_lockstep(fwd, adj, V, seed, cplx, count)
            for c in range(g0, g0 + gc):
                xn = M.cabs1(X[:, c]).max()
                fe[c] = est[c - g0] / xn if xn != 0.0 else est[c - g0]
    return X, berr, (fe if ferr else None), steps
