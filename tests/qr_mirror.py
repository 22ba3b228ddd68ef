"""NumPy restatement of the rank-revealing orthogonalisation of the HSS module (qr_refine, csrc/hs_hss.hip) in the order of decisions
of the device code, so a test can compare the device's ranks, row orders, accepted blocks, d_j and interpolation matrices with it.

  * `select`      : qr_select_kernel -- the window of a norm-ordered job: the largest res2 of the unaccepted rows, a histogram of
                    log2(max / res2) over 16 buckets (frexp), the smallest bucket `cut` <= 14 that fills the window, a stable partition
                    (every row of the buckets < cut and the first rows of bucket `cut` that still fit in front, the rest behind them, both
                    in their original order), and the largest res2 among the rows not selected.  Nothing is re-ordered when every remaining row fits the window.
  * `chol_window` : chol_block_kernel -- greedy diagonal pivoting of the window's Gram matrix (largest remaining diagonal entry, the
                    lowest index among equals), stopped by the first of
                        not dk > tau,   tau = max(atol * atol_scale, rtol * max(top, scale_floor), floor_abs, noise_rel * top)
                        not dk > cond * d0           (d0: the window's first pivot)
                        not dk > 0
                        dk^2 < theta^2 * next2       (k > 0 only; next2: the largest res2 outside the selection)
                    Rejected candidates stay next in line, in the order the accepted swaps left them.
  * `refine`      : qr_refine for one job -- window from p or from the selection, two Gram-Schmidt passes against the accepted rows,
                    Gram matrix, chol_window, Q_new = LinvP W, the rows of L, (norm order) the coefficients of every row, the downdate
                    res2 = max(res2 - |c|^2, 0) and the refresh from the explicit residual once the largest downdated norm^2 fell below
                    1e-10 of the value at the last exact norms; a job ends at rmax rows or at a window that accepts nothing; T by the block
                    back-substitution from the right, T = L_RS L_SS^-1.

Two precisions, chosen by `prec`: np.float64 and np.longdouble (complex inputs run in the matching complex type).  The constants (window
width, conditioning cut-off, theta, noise_rel) come from hsk_qr_params through `params(hs)`, never from here.

Every run reports its SMALLEST DECISION MARGIN (`Margin`): the smallest relative distance |a - b| / max(|a|, |b|) by which an accept /
stop comparison that was evaluated (in the kernel's short-circuit order), the pivot choice of an accepted pivot (best against second
best), a bucket assignment (the ratio against the powers of two 2^1 .. 2^15 next to it) or a refresh test was decided.  Comparisons
between two exact zeros (a zero matrix) are the same in every arithmetic and are not counted.  Device and mirror may be compared
decision by decision only where this margin is far above the rounding errors: tests/test_qr_refine_host.py checks >= 1e-6 for every
input of the GPU tests (`refine_cases`, `chol_cases`), together with the agreement of the two precisions on every decision.

The numeric bound of the GPU tests (issue section 5).  Scaled distances
    d:  |d_j - d_ref_j| / (|M[p_j, :]| + d0_window^2 / d_j)          (max over the accepted rows)
    T:  max|T - T_ref| / (cond_2(M[p_S, :]) * max(1, max|T_ref|))
measured between the float64 and the extended-precision mirror over all `refine_cases` in both orders, on the CPU:
    d 5.605e-16, T 1.076e-15      (MEASURED_D = 5.7e-16, MEASURED_T = 1.1e-15 below; test_qr_refine_host.py re-measures and compares)
The device sums in MFMA order, not NumPy's: the GPU tests allow 16 times these, BOUND_D = 9.12e-15 and BOUND_T = 1.76e-14.  Largest
distances of the device (MI355X) from the extended-precision mirror over the same inputs: d 9.2e-16, T 1.3e-15.  The smallest decision
margin over all inputs is 1.06e-5 (a bucket boundary in "strong m300 q300", norm order).
"""
import math

import numpy as np

MEASURED_D = 5.7e-16
MEASURED_T = 1.1e-15
BOUND_D = 16 * MEASURED_D
BOUND_T = 16 * MEASURED_T


def params(hs):
    """(W, cond, theta, noise_rel) as the library runs them (hsk_qr_params: host only)."""
    out = np.zeros(4)
    hs._lib.check(hs._lib.lib().hsk_qr_params(out.ctypes.data_as(hs._lib.p_f64)))
    return {"W": int(out[0]), "cond": float(out[1]), "theta": float(out[2]), "noise_rel": float(out[3])}


def _ctype(A, prec):
    if np.iscomplexobj(A):
        return np.clongdouble if prec is np.longdouble else np.complex128
    return prec


class Margin:
    def __init__(self):
        self.min = np.inf
        self.where = None

    def note(self, kind, a, b):
        a, b = float(a), float(b)
        s = max(abs(a), abs(b))
        if s == 0.0:
            return
        r = abs(a - b) / s
        if r < self.min:
            self.min, self.where = r, (kind, a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
def select(p, done, m, want, res2, margin=None):
    """qr_select_kernel: returns (the new p, [largest res2 of the tail, largest res2 of the rows not selected])."""
    p = np.array(p, dtype=np.int64)
    nt = m - done
    if nt <= 0:
        return p, [0.0, 0.0]
    tail = p[done:].copy()
    v = res2[tail]
    zero = v.dtype.type(0)
    mx = zero
    for x in v:  # fmax from 0: a NaN never wins
        if x > mx:
            mx = x
    if not (mx > 0) or nt <= want:
        return p, [mx, zero]
    bk = np.full(nt, 15, dtype=np.int64)
    for e in range(nt):
        if v[e] > 0:
            ratio = mx / v[e]
            ex = int(np.frexp(ratio)[1])  # ratio in [2^(ex-1), 2^ex)
            bk[e] = min(max(ex - 1, 0), 15)
            if margin is not None and ex <= 16:
                if ex - 1 >= 1:
                    margin.note("bucket", ratio, 2.0 ** (ex - 1))
                if ex <= 15:
                    margin.note("bucket", ratio, 2.0 ** ex)
    hist = np.bincount(bk, minlength=16)
    cum, cut = 0, 14
    for b in range(15):
        cum += hist[b]
        if cum >= want:
            cut = b
            break
    low, eq = bk < cut, bk == cut
    quota = want - int(low.sum())  # > 0: the buckets below the cut do not fill the window
    take = low | (eq & (np.cumsum(eq) - eq < quota))
    new = np.concatenate([tail[take], tail[~take]])
    rest = res2[tail[~take]]
    mo = zero
    for x in rest:
        if x > mo:
            mo = x
    p[done:] = new
    return p, [mx, mo]


def chol_window(G, b, first, top, atol, rtol, scale_floor, floor_abs, next2, P, prec=np.float64, margin=None):
    """chol_block_kernel on the b x b Gram matrix G.  atol is the job's absolute tolerance already multiplied by atol_scale; next2 None: none.
    Returns a dict: na, perm (new position i holds old candidate perm[i]), L (na x na), Linv (na x na), LinvP (na x b), d (na), top,
    d0 (the window's first pivot)."""
    ct = _ctype(G, prec)
    g = np.array(G[:b, :b], dtype=ct)
    perm = list(range(b))
    rt = prec
    top = rt(top)
    d0 = tau = rt(0)
    out2 = rt(P["theta"]) ** 2 * rt(next2) if next2 is not None else rt(0)
    cond, noise = rt(P["cond"]), rt(P["noise_rel"])
    na = 0
    mg = margin if margin is not None else Margin()
    for k in range(b):
        diag = g.diagonal().real[k:]
        i = int(np.argmax(diag))  # the first of equals, as the kernel's strict >
        bv, pv = diag[i], k + i
        dk = np.sqrt(bv) if bv > 0 else rt(0)
        if k == 0:
            d0 = dk
            if first:
                top = dk
            tau = max(rt(atol), rt(rtol) * max(top, rt(scale_floor)), rt(floor_abs), noise * top)
        mg.note("tau", dk, tau)
        if not (dk > tau):
            break
        mg.note("cond", dk, cond * d0)
        if not (dk > cond * d0):
            break
        if not (dk > 0):
            break
        if k > 0 and next2 is not None:
            mg.note("next2", dk * dk, out2)
            if dk * dk < out2:
                break
        if len(diag) > 1:
            mg.note("pivot", bv, np.max(np.delete(diag, i)))
        if pv != k:
            perm[k], perm[pv] = perm[pv], perm[k]
            g[:, [k, pv]] = g[:, [pv, k]]
            g[[k, pv], :] = g[[pv, k], :]
        g[k, k] = dk
        g[k + 1:, k] = g[k + 1:, k] / dk
        col = g[k + 1:, k]
        g[k + 1:, k + 1:] -= np.outer(col, col.conj())
        na = k + 1
    L = np.tril(g[:na, :na])
    Li = np.zeros((na, na), dtype=ct)
    for i in range(na):
        Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
        Li[i, i] = 1 / L[i, i]
    LiP = np.zeros((na, b), dtype=ct)
    for c in range(na):
        LiP[:, perm[c]] = Li[:, c]
    return {"na": na, "perm": perm, "L": L, "Linv": Li, "LinvP": LiP, "d": L.diagonal().real.copy(), "top": top, "d0": d0}


def _rownorm2(A):
    return (A.real ** 2 + A.imag ** 2).sum(axis=1) if np.iscomplexobj(A) else (A * A).sum(axis=1)


def refine(M, p, rmax, atol, rtol, scale_floor, P, atol_scale=1.0, floor_abs=0.0, norm_select=False, prec=np.float64):
    """qr_refine on one job.  Returns a dict: r, top, p, d, T ((m - r) x r), blocks [(offset, width)], windows, refreshes, decisions (a list a
    second run can be compared with by ==), margin (Margin), d0win (the first pivot of the window that accepted row j), Q (r x q)."""
    m, q = M.shape
    ct = _ctype(M, prec)
    Mx = np.array(M, dtype=ct)
    rmax = max(0, min(rmax, m, q))
    p = np.array(p, dtype=np.int64)
    W = P["W"]
    Q = np.zeros((rmax, q), dtype=ct)
    L = np.zeros((rmax, rmax), dtype=ct)
    d, d0win, blocks, linv, decisions = [], [], [], [], []
    mg = Margin()
    top = prec(0)
    done = windows = refreshes = 0
    res2 = LRS = None
    refmax = prec(0)
    outmax = [prec(0), prec(0)]
    if norm_select and rmax > 0:
        res2 = _rownorm2(Mx)
        p = np.arange(m, dtype=np.int64)
        LRS = np.zeros((m, rmax), dtype=ct)
    active = rmax > 0
    while active:
        b = min(W, rmax - done)
        if norm_select:
            p, outmax = select(p, done, m, b, res2, mg)
        cand = p[done:done + b].copy()
        Wm = Mx[cand]
        C1 = None
        if done > 0:
            Qd = Q[:done]
            C1 = Wm @ Qd.conj().T
            Wm = Wm - C1 @ Qd
            C2 = Wm @ Qd.conj().T
            Wm = Wm - C2 @ Qd
            C1 = C1 + C2
        G = Wm @ Wm.conj().T
        windows += 1
        c = chol_window(G, b, done == 0, top, atol * atol_scale, rtol, scale_floor, floor_abs, outmax[1] if norm_select else None, P, prec, mg)
        if done == 0:
            top = c["top"]
        na, perm = c["na"], c["perm"]
        p[done:done + b] = cand[perm]
        decisions.append(("window", done, tuple(int(x) for x in cand), na, tuple(perm[:na])))
        if na > 0:
            Qn = c["LinvP"] @ Wm
            Q[done:done + na] = Qn
            L[done:done + na, done:done + na] = c["L"]
            if done > 0:
                L[done:done + na, :done] = C1[perm[:na]]
            d += [float(x) for x in c["d"]]
            d0win += [float(c["d0"])] * na
            if norm_select:
                col = Mx @ Qn.conj().T
                LRS[:, done:done + na] = col
                res2 = np.maximum(res2 - _rownorm2(col), 0)
            blocks.append((done, na))
            linv.append(c["Linv"])
            done += na
        if done >= rmax or na == 0:
            active = False
        if active and norm_select:
            if refmax == 0:
                refmax = outmax[0]
            mg.note("refresh", outmax[0], prec(1e-10) * refmax)
            if outmax[0] < prec(1e-10) * refmax and done > 0:
                R = Mx - LRS[:, :done] @ Q[:done]
                res2 = _rownorm2(R)
                refmax = outmax[0]
                refreshes += 1
                decisions.append(("refresh", done))
    r = done
    nR = m - r
    T = np.zeros((nR, r), dtype=ct)
    if nR > 0 and r > 0:
        T = LRS[p[r:], :r].copy() if norm_select else Mx[p[r:]] @ Q[:r].conj().T
        for bi in range(len(blocks) - 1, -1, -1):
            j0, w = blocks[bi]
            j1 = j0 + w
            if r > j1:
                T[:, j0:j1] -= T[:, j1:r] @ L[j1:r, j0:j1]
            T[:, j0:j1] = T[:, j0:j1] @ linv[bi]
    return {"r": r, "top": max(float(top), 0.0), "p": p, "d": np.array(d, dtype=np.float64), "T": T, "blocks": blocks, "windows": windows, "refreshes": refreshes,
            "decisions": decisions, "margin": mg, "d0win": np.array(d0win, dtype=np.float64), "Q": Q[:r]}


def scaled_distances(M, ref, d, T):
    """The scaled distances of section 5 of (d, T) from the run `ref` of `refine` on M (same decisions): (distance of d, distance of T)."""
    r = ref["r"]
    dd = dt = 0.0
    if r > 0:
        rows = np.linalg.norm(np.asarray(M, dtype=np.complex128 if np.iscomplexobj(M) else np.float64)[ref["p"][:r]], axis=1)
        dref = ref["d"]
        dd = float(np.max(np.abs(np.asarray(d, dtype=np.float64) - dref) / (rows + ref["d0win"] ** 2 / dref)))
        if ref["T"].size:
            Ms = np.asarray(M)[ref["p"][:r]]
            cnd = float(np.linalg.cond(Ms))
            Tr = ref["T"]
            dt = float(np.max(np.abs(np.asarray(T) - Tr))) / (cnd * max(1.0, float(np.max(np.abs(Tr)))))
    return dd, dt


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs of the GPU tests: M = L Q with orthonormal rows of Q and a prescribed diagonal of L
# ---------------------------------------------------------------------------------------------------------------------------------
def lq_input(m, q, diag, family, cplx, seed):
    """M (m x q) = L Q: Q k x q with orthonormal rows (k = min(m, q)), L m x k lower trapezoidal with L_jj = diag[j].
    family "weak": |L_ij| <= 0.3 |L_ii| / sqrt(i) (the natural order is the greedy one); "strong": L_ij = g_ij |L_jj| with Gaussian g
    (nearly dependent rows, as sketch rows are).  Rows below the square part (m > q) are scaled like the last diagonal entry."""
    rng = np.random.default_rng(seed)
    k = min(m, q)
    diag = np.asarray(diag, dtype=np.float64)
    assert diag.shape == (k,)

    def randn(*s):
        return rng.standard_normal(s) + 1j * rng.standard_normal(s) if cplx else rng.standard_normal(s)

    Qf = np.linalg.qr(randn(q, k))[0].conj().T  # k x q
    if family == "weak":
        u = rng.uniform(-1.0, 1.0, (m, k))
        if cplx:
            u = u * np.exp(2j * np.pi * rng.random((m, k)))
        rowscale = np.abs(diag[np.minimum(np.arange(m), k - 1)]) / np.sqrt(np.arange(1, m + 1))
        L = 0.3 * u * rowscale[:, None]
    else:
        L = randn(m, k) * np.abs(diag)[None, :]
    L = np.tril(L, -1).astype(np.complex128 if cplx else np.float64)
    L[np.arange(k), np.arange(k)] = diag
    return np.asfortranarray(L @ Qf)


def graded(k, hi, lo):
    return hi * (lo / hi) ** (np.arange(k) / max(k - 1, 1))


def gap_diag(k, rank, tau, hi=1.0):
    """k entries: the first `rank` graded from hi down to 4 tau, the rest from tau / 4 down to tau / 40 (a factor 4 on either side of tau)."""
    d = np.empty(k)
    d[:rank] = graded(rank, hi, 4.0 * tau)
    if rank < k:
        d[rank:] = graded(k - rank, tau / 4.0, tau / 40.0)
    return d


def _case(name, M, rtol, atol=0.0, scale_floor=0.0, atol_scale=1.0, floor_abs=0.0, rmax=None, p=None, rank=None, orders=(0, 1)):
    m, q = M.shape
    return {"name": name, "M": M, "p": np.arange(m) if p is None else np.asarray(p), "rmax": min(m, q) if rmax is None else rmax, "atol": atol, "rtol": rtol,
            "scale_floor": scale_floor, "atol_scale": atol_scale, "floor_abs": floor_abs, "rank": rank, "orders": orders}


SIZES_M = (1, 2, 63, 64, 65, 129, 300)


def size_cases(cplx):
    """m in SIZES_M x q in {1, 40, m, m + 37}: weak and strong families in turn, a designed rank of about 2/3 min(m, q) with a gap of 4 on either
    side of tau = 1e-6 top (weak, natural order), the strong ones in a random given order (no designed rank: the mirror decides)."""
    out = []
    n = 0
    for m in SIZES_M:
        for q in sorted({1, 40, m, m + 37}):
            k = min(m, q)
            n += 1
            seed = 1000 * n + (7 if cplx else 0)
            if n % 2 == 0 and k >= 2:
                M = lq_input(m, q, graded(k, 1.0, 1e-4), "strong", cplx, seed)
                p = np.random.default_rng(seed + 1).permutation(m)
                out.append(_case(f"strong m{m} q{q}", M, 1e-3, p=p))
            else:
                rank = max(1, 2 * k // 3)
                M = lq_input(m, q, gap_diag(k, rank, 1e-6), "weak", cplx, seed)
                out.append(_case(f"weak m{m} q{q}", M, 1e-6, rank=rank))
    return out


def rule_cases(cplx):
    """rmax below / at / above the rank, the five thresholds binding in turn, the conditioning cut-off inside one window, a window that accepts
    nothing, a zero matrix and rmax = 0."""
    s = 50 if cplx else 0
    out = []
    tau = 1e-3
    M = lq_input(80, 100, gap_diag(80, 50, tau), "weak", cplx, 11 + s)
    out.append(_case("rmax below the rank", M, tau, rmax=37, rank=37))
    out.append(_case("rmax at the rank", M, tau, rmax=50, rank=50))
    out.append(_case("tau = rtol * top", M, tau, rank=50))
    out.append(_case("tau = atol * atol_scale", M, 1e-9, atol=tau / 8, atol_scale=8.0, rank=50))
    out.append(_case("tau = rtol * scale_floor", M, tau / 100, scale_floor=100.0, rank=50))
    out.append(_case("tau = floor_abs", M, 1e-9, atol=1e-9, floor_abs=tau, rank=50))
    Mn = lq_input(80, 100, gap_diag(80, 50, 1e-13), "weak", cplx, 12 + s)
    out.append(_case("tau = noise_rel * top", Mn, 0.0, rank=50))
    out.append(_case("full rank r == m", lq_input(70, 90, graded(70, 1.0, 2e-3), "weak", cplx, 13 + s), 1e-8, rank=70))
    out.append(_case("conditioning cut in one window", lq_input(40, 60, graded(40, 1.0, 1e-4), "weak", cplx, 14 + s), 1e-8, rank=40))
    d = np.concatenate([graded(64, 1.0, 0.5), graded(36, 1e-9, 1e-10)])
    out.append(_case("second window accepts nothing", lq_input(100, 120, d, "weak", cplx, 15 + s), 1e-6, rank=64))
    out.append(_case("zero matrix", np.zeros((70, 50), dtype=np.complex128 if cplx else np.float64, order="F"), 1e-6, atol=1e-6, rank=0))
    out.append(_case("rmax = 0", M, tau, rmax=0, rank=0))
    return out


def norm_cases(cplx):
    """norm order only: three chunks of the selection (m = 700) and the refresh (a spectrum graded from 1 to 1e-8 over 100 rows, rtol 1e-10)."""
    s = 50 if cplx else 0
    out = [_case("m700 weak", lq_input(700, 40, gap_diag(40, 30, 1e-6), "weak", cplx, 21 + s), 1e-6, rank=30, orders=(1,)),
           _case("m700 strong", lq_input(700, 40, graded(40, 1.0, 1e-3), "strong", cplx, 22 + s), 1e-2, orders=(1,))]
    d = np.concatenate([graded(100, 1.0, 1e-8), graded(30, 2.5e-11, 2.5e-12)])
    out.append(_case("refresh", lq_input(130, 140, d, "weak", cplx, 23 + s), 1e-10, rank=100, orders=(1,)))
    return out


def batch_cases(cplx):
    """Six jobs of different m, q and rank for one call (the same atol, rtol and scale_floor: they belong to the call), among them an rmax = 0 job and a zero matrix, finishing at different windows."""
    s = 50 if cplx else 0
    tau = 1e-6
    z = np.zeros((33, 47), dtype=np.complex128 if cplx else np.float64, order="F")
    return [_case("batch 0", lq_input(150, 170, gap_diag(150, 120, tau), "weak", cplx, 31 + s), tau, rank=120),
            _case("batch 1", lq_input(20, 64, gap_diag(20, 5, tau), "weak", cplx, 32 + s), tau, rank=5),
            _case("batch 2 rmax = 0", lq_input(40, 40, graded(40, 1.0, 0.1), "weak", cplx, 33 + s), tau, rmax=0, rank=0),
            _case("batch 3 zero", z, tau, rank=0),
            _case("batch 4", lq_input(90, 30, graded(30, 1.0, 1e-3), "strong", cplx, 34 + s), tau),
            _case("batch 5", lq_input(65, 65, gap_diag(65, 64, tau), "weak", cplx, 35 + s), tau, rank=64)]


def refine_cases(cplx):
    return size_cases(cplx) + rule_cases(cplx) + norm_cases(cplx) + batch_cases(cplx)


def run_case(c, order, P, prec=np.float64):
    return refine(c["M"], c["p"], c["rmax"], c["atol"], c["rtol"], c["scale_floor"], P, c["atol_scale"], c["floor_abs"], bool(order), prec)


def chol_cases(cplx, P):
    """Jobs for chol_block_kernel alone: dicts with b, G (W x W, column-major), first, top, thr = (atol, rtol, scale_floor, floor_abs, next2 or -1), p,
    and `nacc` where the design fixes it.  Gram matrices of L Q windows (weak family) for b in {1, 2, 31, 63, 64}, then the stop rules in turn."""
    W = P["W"]
    s = 50 if cplx else 0
    ct = np.complex128 if cplx else np.float64
    out = []

    def job(name, Wm, first=1, top=0.0, atol=0.0, rtol=0.0, scale_floor=0.0, floor_abs=0.0, next2=-1.0, nacc=None, G=None, seed=0):
        b = Wm.shape[0] if G is None else G.shape[0]
        Gf = np.zeros((W, W), dtype=ct, order="F")
        Gb = Wm @ Wm.conj().T if G is None else G
        Gf[:b, :b] = (Gb + Gb.conj().T) / 2  # exactly Hermitian: L L^H can then be compared with it entry by entry
        p = np.random.default_rng(900 + seed + s).permutation(1000)[:b].astype(np.int32)
        out.append({"name": name, "b": b, "G": Gf, "first": first, "top": top, "thr": (atol, rtol, scale_floor, floor_abs, next2), "p": p, "nacc": nacc})

    for n, b in enumerate((1, 2, 31, 63, 64)):
        job(f"b = {b}", lq_input(b, b + 9, graded(b, 1.0, 0.05), "weak", cplx, 41 + n + s), rtol=1e-6, nacc=b, seed=n)
    job("strong b = 64", lq_input(64, 80, graded(64, 1.0, 0.2), "strong", cplx, 47 + s), rtol=1e-6, seed=6)
    job("not first: top comes in", lq_input(31, 40, graded(31, 1e-2, 1e-3), "weak", cplx, 48 + s), first=0, top=7.0, rtol=1e-6, nacc=31, seed=7)
    # tolerance: three rows above tau = 1e-2 top, two below
    job("tolerance", lq_input(5, 9, np.array([1.0, 0.5, 0.25, 2e-3, 1e-3]), "weak", cplx, 49 + s), rtol=1e-2, nacc=3, seed=8)
    job("tolerance from top, not first", lq_input(5, 9, np.array([1.0, 0.5, 0.25, 2e-3, 1e-3]), "weak", cplx, 49 + s), first=0, top=100.0, rtol=1e-3, nacc=3, seed=9)
    # conditioning: graded 1 .. 1e-3, only the rows above cond * d0 are accepted
    cnd = P["cond"]
    dg = np.concatenate([graded(20, 1.0, 2.0 * cnd), graded(12, cnd / 2.0, cnd / 10.0)])
    job("conditioning", lq_input(32, 40, dg, "weak", cplx, 50 + s), rtol=1e-9, nacc=20, seed=10)
    # next2: the rows below theta * sqrt(next2) = 0.4 wait for the next window; the first pivot is always allowed
    th = P["theta"]
    dg = np.concatenate([graded(9, 1.0, 0.55), graded(7, 0.3, 0.1)])
    job("next2", lq_input(16, 20, dg, "weak", cplx, 51 + s), rtol=1e-9, next2=(0.4 / th) ** 2, nacc=9, seed=11)
    job("next2 allows k = 0", lq_input(16, 20, dg, "weak", cplx, 51 + s), rtol=1e-9, next2=1e6, nacc=1, seed=12)
    job("zero Gram matrix", None, G=np.zeros((17, 17), dtype=ct), rtol=1e-6, atol=1e-6, nacc=0, seed=13)
    # a trailing diagonal entry that the update drives below zero: 0.99 - |0.995|^2 < 0 (no threshold: tau = 0)
    x = 0.995 * (np.exp(0.7j) if cplx else 1.0)
    job("diagonal driven below zero", None, G=np.array([[1.0, np.conj(x)], [x, 0.99]], dtype=ct), first=0, top=0.0, nacc=1, seed=14)
    return out


def run_chol_case(c, P, prec=np.float64, margin=None):
    t = c["thr"]
    return chol_window(c["G"], c["b"], c["first"], c["top"], t[0], t[1], t[2], t[3], None if t[4] < 0 else t[4], P, prec, margin)


def residual_norms_along(M, p, r):
    """Extended-precision residual norms along an accepted order, independent of `refine` (modified Gram-Schmidt, each new direction
    orthogonalised twice): (dist, others, resid) with dist[j] = distance of row p[j] from the span of the rows p[:j], others[j] = the largest
    such distance among the rows p[j + 1:] at that step (0 when there is none), j < r, and resid = the rows p[r:] minus their projection
    on the span of the rows p[:r]."""
    ct = _ctype(M, np.longdouble)
    R = np.array(np.asarray(M)[np.asarray(p)], dtype=ct)  # residuals of all rows, in the order p
    m = R.shape[0]
    dist, others = np.zeros(r, dtype=np.longdouble), np.zeros(r, dtype=np.longdouble)
    basis = []
    for j in range(r):
        nrm = np.sqrt(_rownorm2(R[j:]))
        dist[j] = nrm[0]
        others[j] = nrm[1:].max() if m > j + 1 else 0
        v = R[j].copy()
        for _ in range(2):
            for b in basis:
                v = v - (v @ b.conj()) * b
        v = v / np.sqrt(_rownorm2(v[None, :])[0])
        basis.append(v)
        R[j + 1:] -= np.outer(R[j + 1:] @ v.conj(), v)
    return dist, others, R[r:]


def select_cases():
    """(name, m, done, want, p, res2) for qr_select_kernel: nt in {1, want, want + 1, 255, 256, 257, 700} and the edge cases."""
    rng = np.random.default_rng(77)
    out = []

    def add(name, m, done, want, res2, p=None):
        out.append((name, m, done, want, (rng.permutation(m) if p is None else np.asarray(p)).astype(np.int32), np.asarray(res2, dtype=np.float64)))

    for nt in (1, 64, 65, 255, 256, 257, 700):
        add(f"nt = {nt}", nt, 0, 64, 10.0 ** rng.uniform(-3, 0, nt))
        add(f"nt = {nt}, done > 0", nt + 37, 37, 64, 10.0 ** rng.uniform(-2, 0, nt + 37))
    add("want < 64", 300, 20, 17, 10.0 ** rng.uniform(-3, 0, 300))
    add("want + 1 rows", 18, 0, 17, 10.0 ** rng.uniform(-1, 0, 18))
    add("more than 15 buckets", 400, 0, 64, 10.0 ** rng.uniform(-12, 0, 400))
    r = 10.0 ** rng.uniform(-3, 0, 300)
    r[rng.permutation(300)[:120]] = 0.0
    add("zeros in res2", 300, 11, 64, r)
    add("all zeros", 200, 5, 64, np.zeros(200))
    add("exact powers of two", 300, 0, 64, 2.0 ** (-rng.integers(0, 20, 300)).astype(np.float64))
    add("powers of two and neighbours", 300, 0, 64, np.nextafter(2.0 ** (-rng.integers(0, 17, 300)).astype(np.float64), rng.choice([0.0, 4.0], 300)))
    r = np.full(500, 1e-9)
    r[rng.permutation(500)[:9]] = rng.uniform(0.5, 1.0, 9)  # nine rows within 2^-7 in norm of the largest: fewer than want qualify
    add("fewer qualifying rows than want", 500, 0, 64, r)
    r = np.full(300, 1e-30)
    r[5] = 1.0
    add("one row, the rest in bucket 15", 300, 0, 64, r)
    add("nothing left", 10, 10, 64, rng.random(10))
    # the last bucket that may be selected is 14 (2^-7.5 .. 2^-7 in norm); bucket 15 never is, even when the window stays short
    r = np.full(100, 2.0 ** -17.5)
    r[:5], r[5:10], r[10:15], r[15:20] = 1.0 - 0.01 * np.arange(5), 2.0 ** -13.5, 2.0 ** -14.5, 2.0 ** -15.5
    add("buckets 13, 14 and 15 with a short window", 100, 0, 64, r[rng.permutation(100)])
    # the cutoff bucket overflows and the largest rows come last in the list: they belong in the window all the same
    r = np.full(200, 0.2)
    r[[3, 77, 150]] = [1.0, 0.9, 0.45]
    add("largest rows last, cutoff bucket overflows", 200, 0, 64, r, p=[i for i in range(200) if i not in (3, 77, 150)] + [150, 77, 3])
    return out


def check_selection(name, m, done, want, p0, res2, p1, outmax):
    """What a selection must satisfy whatever the cut: the head untouched, the tail a stable partition with the selected rows in front, both maxima."""
    assert np.array_equal(p1[:done], p0[:done]), name
    tail0, tail1 = list(p0[done:]), list(p1[done:])
    assert sorted(tail0) == sorted(tail1), name
    nt = m - done
    v = res2[p0[done:]]
    assert outmax[0] == (v.max() if nt else 0.0), name
    if nt <= want or not v.max() > 0:
        assert tail1 == tail0 and outmax[1] == 0.0, name
        return
    mx = float(v.max())
    bucket = [15 if not res2[row] > 0 else min(max(math.frexp(mx / float(res2[row]))[1] - 1, 0), 15) for row in tail0]
    cut = next((b for b in range(15) if sum(1 for x in bucket if x <= b) >= want), 14)
    nlow = sum(1 for x in bucket if x < cut)
    atcut = [row for row, x in zip(tail0, bucket) if x == cut][:want - nlow]
    sel = [row for row, x in zip(tail0, bucket) if x < cut or row in set(atcut)]
    assert len(sel) <= want and (len(sel) == want or all(x > cut for row, x in zip(tail0, bucket) if row not in set(sel))), name
    rest = [row for row in tail0 if row not in set(sel)]
    assert tail1 == sel + rest, name  # selected rows first, in original order; the rest follow in original order
    assert outmax[1] == (max(res2[row] for row in rest) if rest else 0.0), name
