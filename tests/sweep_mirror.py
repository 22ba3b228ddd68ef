"""Extended-precision mirror of ONE tree level of the ldiv! sweeps (csrc/kernels_solve.hip, kernels_solve_wide.hip, kernels_solve_t.hip), and a
float64 NumPy implementation of the same sweeps that the host test holds the mirror to.

The check is LOCAL: every step of the recurrence is evaluated in longdouble / clongdouble on the implementation's own earlier outputs, so the
only difference a correct implementation can show is the rounding of that one step.  (An exact triangular solve as the reference needs a
condition number in its tolerance, which hides a wrong tile; a propagated componentwise bound grows like 2^ni.)

A level is a dict  n, b0 (length n), fronts;  a front is a dict
  ni, nb, fidx (m global ids, front order [int; bnd]), LF (m x ni: L\\U of P*Aii over Lbi = Abi*U^-1), UR (ni x nb: Uib = L^-1*P*Aib),
  rperm ((P x)[i] = x[rperm[i]]), compressed, blank, inv = {32: (XL, XU), 256: (XL, XU)} with XL / XU of shape (blocks, bs, bs): the stored
  inverses of the diagonal blocks of L (unit lower) and U -- only their own triangle and their leading wl x wl part count.
The outputs of an implementation are a dict  y, x (lists, one ni-vector per front), b_fwd, b_bwd (length n).

With w the gathered right-hand side, a hat on what the implementation returned, blocks of bs = 256 (bs = 32 for the 32-column sweeps):
  N  w = b0[fidx[rperm]];  y^_j  ~ XL_j (w_j - sum_{k<j} L_jk y^_k);  b^[bnd] ~ b0[bnd] - Lbi y^
     v = y^ - Uib b^[bnd]; x^_j  ~ XU_j (v_j - sum_{k>j} U_jk x^_k);  b^[fidx[:ni]] == x^ bitwise
  T  w = b0[fidx[:ni]];    z^_j  ~ XU_j^T (w_j - sum_{k<j} U_kj^T z^_k);  b^[bnd] ~ b0[bnd] - Uib^T z^
     v = z^ - Lbi^T b^[bnd]; x^_j ~ XL_j^T (v_j - sum_{k>j} L_kj^T x^_k);  b^[fidx[rperm[i]]] == x^[i] bitwise
  H  as T with every factor entry conjugated.
Bound, every entry:  |got - mirror| <= c K eps S,  K = ni + nb + 256,  S the same expression on absolute values (v contributes
|y^| + |Uib| |b^[bnd]|),  c = 2 (Float64) / 8 (ComplexF64): the first-order error of a K-term FMA dot product in any order followed by a
256-term product with the stored inverse is (K/2) eps S; a factor 4 for second-order terms and the reduction trees, another 4 for complex
multiply-add.  Nothing in it is measured on an implementation.

Not bounded, but required bitwise unchanged: every entry of a blank front (and of a front without interior DOFs), the boundary of a
compressed front after the forward sweep (its v must equal y^ exactly: the mirror uses v = y^ there), and every entry of b no front names."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD, CLD = np.longdouble, np.clongdouble


def _bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _op(M, trans):
    return M.T if trans == 1 else M.conj().T


class Report:
    """worst[what] = largest |got - mirror| / bound seen; fails = [(what, front, row, ratio)] for every entry beyond the bound and every
    bitwise condition that does not hold; entries = how many entries were held to the bound."""

    def __init__(self):
        self.worst = {}
        self.fails = []
        self.entries = 0

    def ratio(self):
        return max(self.worst.values()) if self.worst else 0.0

    def compare(self, what, front, got, ref, S, K, c, row0=0):
        diff = np.abs(np.asarray(got).astype(ref.dtype) - ref).astype(np.float64)
        bnd = c * K * EPS * np.asarray(S, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bnd > 0, diff / bnd, np.where(diff == 0, 0.0, np.inf))
        r = np.where(np.isfinite(diff), r, np.inf)  # a NaN or Inf never passes
        self.entries += r.size
        if r.size:
            self.worst[what] = max(self.worst.get(what, 0.0), float(r.max()))
            for i in np.flatnonzero(r > 1.0)[:4]:
                self.fails.append((what, front, row0 + int(i), float(r[i])))

    def bitwise(self, what, front, a, b):
        if _bits_equal(a, b):
            return
        bad = []
        if len(a) == len(b) and a.dtype == b.dtype:
            ua = np.ascontiguousarray(a).view(np.uint64).reshape(len(a), -1)
            ub = np.ascontiguousarray(b).view(np.uint64).reshape(len(b), -1)
            bad = [int(i) for i in np.flatnonzero((ua != ub).any(axis=1))[:4]]
        self.fails.append((what, front, bad, float("inf")))

    def assert_ok(self, what=""):
        assert not self.fails, (what, self.fails[:8], self.worst)


def _offdiag(LF, ni, bs):
    """(Loff, Uoff): the parts of L11 / U11 outside the diagonal bs-blocks."""
    blk = np.arange(ni) // bs
    A = LF[:ni]
    return np.where(blk[:, None] > blk[None, :], A, 0), np.where(blk[:, None] < blk[None, :], A, 0)


def _tri_blocks(X, ni, bs, lower):
    out = []
    for j in range((ni + bs - 1) // bs):
        wl = min(bs, ni - j * bs)
        B = np.asarray(X[j])[:wl, :wl]
        out.append(np.tril(B) if lower else np.triu(B))
    return out


def check_level(level, out, trans, bs):
    """Hold the outputs `out` of one level's sweeps (trans 0 / 1 / 2 = N / T / H, diagonal blocks of bs = 32 or 256) to the mirror.  Returns a
    Report; Report.assert_ok() raises with the front, quantity and row of what failed.  EVERY entry of every front is either held to the bound
    or required bitwise unchanged, and so is every entry of b."""
    b0, bf, bb = level["b0"], out["b_fwd"], out["b_bwd"]
    cplx = np.iscomplexobj(b0)
    wide = CLD if cplx else LD
    c = 8.0 if cplx else 2.0
    rep = Report()
    exp_f = b0.copy()  # what b must hold bitwise after each direction wherever no bound applies
    free_f = np.zeros(len(b0), dtype=bool)  # entries held to a bound instead
    int_ids, int_val = [], []
    for f, fr in enumerate(level["fronts"]):
        ni, nb = fr["ni"], fr["nb"]
        if fr.get("blank") or ni == 0:
            continue
        fidx = np.asarray(fr["fidx"])
        ii, bi = fidx[:ni], fidx[ni:]
        rperm = np.asarray(fr["rperm"])
        K = ni + nb + 256
        comp = bool(fr.get("compressed"))
        LF, UR = fr["LF"], fr["UR"]
        Loff, Uoff = _offdiag(LF, ni, bs)
        Lbi, Uib = LF[ni:], UR
        XL = _tri_blocks(fr["inv"][bs][0], ni, bs, True)
        XU = _tri_blocks(fr["inv"][bs][1], ni, bs, False)
        yh, xh = np.asarray(out["y"][f]), np.asarray(out["x"][f])
        if trans == 0:
            w = b0[ii[rperm]]
            Mf, Xf, Bf = Loff, XL, Lbi            # forward: off-diagonal part, inverses, boundary operator (applied to y^)
            Mb, Xb, Vb = Uoff, XU, Uib            # backward
            opx = lambda B: B
        else:
            w = b0[ii]
            Mf, Xf, Bf = _op(Uoff, trans), XU, _op(Uib, trans)
            Mb, Xb, Vb = _op(Loff, trans), XL, _op(Lbi, trans)
            opx = lambda B: _op(B, trans)
        # forward
        t = w.astype(wide) - Mf.astype(wide) @ yh.astype(wide)
        St = np.abs(w) + np.abs(Mf) @ np.abs(yh)
        for j, X in enumerate(Xf):
            s = slice(j * bs, j * bs + X.shape[0])
            Xo = opx(X)
            rep.compare("fwd y" if trans == 0 else "fwd z", f, yh[s], Xo.astype(wide) @ t[s], np.abs(Xo) @ St[s], K, c, j * bs)
        if nb and not comp:
            ref = b0[bi].astype(wide) - Bf.astype(wide) @ yh.astype(wide)
            rep.compare("fwd b[bnd]", f, bf[bi], ref, np.abs(b0[bi]) + np.abs(Bf) @ np.abs(yh), K, c)
            free_f[bi] = True
        # backward
        if nb and not comp:
            v = yh.astype(wide) - Vb.astype(wide) @ bf[bi].astype(wide)
            Sv = np.abs(yh) + np.abs(Vb) @ np.abs(bf[bi])
        else:
            v, Sv = yh.astype(wide), np.abs(yh)
        t = v - Mb.astype(wide) @ xh.astype(wide)
        St = Sv + np.abs(Mb) @ np.abs(xh)
        for j, X in enumerate(Xb):
            s = slice(j * bs, j * bs + X.shape[0])
            Xo = opx(X)
            rep.compare("bwd x", f, xh[s], Xo.astype(wide) @ t[s], np.abs(Xo) @ St[s], K, c, j * bs)
        int_ids.append(ii if trans == 0 else ii[rperm])
        int_val.append(xh)
    # b after the forward sweep: bitwise b0 outside the bounded boundary entries
    rep.bitwise("fwd b elsewhere", -1, bf[~free_f], exp_f[~free_f])
    # b after the backward sweep: the interior entries are x^ (through the permutation), everything else is what the forward sweep left
    exp_b = bf.copy()
    for ids, val in zip(int_ids, int_val):
        exp_b[ids] = val
    rep.bitwise("bwd b", -1, bb, exp_b)
    return rep


def covered_entries(level):
    """How many entries check_level holds to the bound: per live front 2 ni (y, x) + nb (unless compressed)."""
    tot = 0
    for fr in level["fronts"]:
        if fr.get("blank") or fr["ni"] == 0:
            continue
        tot += 2 * fr["ni"] + (0 if fr.get("compressed") else fr["nb"])
    return tot


# ---- a float64 implementation of the same sweeps, for the host test -------------------------------------------------------------------

def host_front(rng, ni, nb, cplx, fidx):
    """A Gaussian front factored with SciPy (partial pivoting) and the NumPy inverses of the diagonal blocks of both sizes."""
    import scipy.linalg as sla

    m = ni + nb
    F = rng.standard_normal((m, m)) + (1j * rng.standard_normal((m, m)) if cplx else 0)
    dt = np.complex128 if cplx else np.float64
    LF = np.zeros((m, ni), dtype=dt)
    UR = np.zeros((ni, nb), dtype=dt)
    rperm = np.arange(ni)
    if ni:
        lu, piv = sla.lu_factor(F[:ni, :ni])
        for i, p in enumerate(piv):
            rperm[[i, p]] = rperm[[p, i]]
        L = np.tril(lu, -1) + np.eye(ni)
        U = np.triu(lu)
        LF[:ni] = lu
        LF[ni:] = sla.solve_triangular(U, F[ni:, :ni].T, trans=1, lower=False).T
        UR[:] = sla.solve_triangular(L, F[:ni, ni:][rperm], lower=True, unit_diagonal=True)
    inv = {}
    for bs in (32, 256):
        nblk = (ni + bs - 1) // bs
        XL = np.zeros((nblk, bs, bs), dtype=dt)
        XU = np.zeros((nblk, bs, bs), dtype=dt)
        for j in range(nblk):
            wl = min(bs, ni - j * bs)
            D = LF[j * bs:j * bs + wl, j * bs:j * bs + wl]
            XL[j, :wl, :wl] = np.linalg.inv(np.tril(D, -1) + np.eye(wl))
            XU[j, :wl, :wl] = np.linalg.inv(np.triu(D))
        inv[bs] = (XL, XU)
    return dict(ni=ni, nb=nb, fidx=np.asarray(fidx), LF=LF, UR=UR, rperm=rperm, inv=inv, compressed=False, blank=False)


def host_sweeps(level, trans, bs, defect=None):
    """The level's sweeps in float64, block by block as the kernels walk them.  defect (None: none) plants one error in the LAST live front:
    "zero_entry"  one entry of the last off-diagonal block of the forward sweep reads as zero
    "skip_column" the last column of the ragged last block is left out of the backward update
    "no_conj"     H: the boundary operator of the backward sweep is transposed but not conjugated
    "rperm_side"  the permutation is applied on the wrong side of the gather (N) / scatter (T, H)"""
    b = level["b0"].copy()
    ys, xs = [], []
    live = [k for k, fr in enumerate(level["fronts"]) if fr["ni"] and not fr.get("blank")]
    state = []
    for k, fr in enumerate(level["fronts"]):
        ni, nb = fr["ni"], fr["nb"]
        bad = defect if live and k == live[-1] else None
        if k not in live:
            ys.append(np.zeros(ni, dtype=b.dtype))
            state.append(None)
            continue
        fidx, rperm = fr["fidx"], fr["rperm"]
        ii, bi = fidx[:ni], fidx[ni:]
        A = fr["LF"][:ni]
        XL, XU = fr["inv"][bs]
        nblk = (ni + bs - 1) // bs
        if trans == 0:
            w = b[ii[rperm]].copy()
            if bad == "rperm_side":
                w = np.empty_like(w)
                w[rperm] = b[ii]
        else:
            w = b[ii].copy()
        y = np.zeros(ni, dtype=b.dtype)
        for j in range(nblk):
            s = slice(j * bs, min(ni, (j + 1) * bs))
            wl = s.stop - s.start
            acc = w[s].copy()
            for q in range(j):
                sq = slice(q * bs, (q + 1) * bs)
                B = A[s, sq] if trans == 0 else _op(A[sq, s], trans)
                if bad == "zero_entry" and j == nblk - 1 and q == j - 1:
                    B = B.copy()
                    B[wl // 2, bs // 2] = 0
                acc -= B @ y[sq]
            X = np.tril(XL[j][:wl, :wl]) if trans == 0 else _op(np.triu(XU[j][:wl, :wl]), trans)
            y[s] = X @ acc
        if nb and not fr.get("compressed"):
            B = fr["LF"][ni:] if trans == 0 else _op(fr["UR"], trans)
            if bad == "zero_entry" and nblk == 1:
                B = B.copy()
                B[nb // 2, ni // 2] = 0
            b[bi] = b[bi] - B @ y
        ys.append(y)
        state.append(bad)
    b_fwd = b.copy()
    for k, fr in enumerate(level["fronts"]):
        ni, nb = fr["ni"], fr["nb"]
        if k not in live:
            xs.append(np.zeros(ni, dtype=b.dtype))
            continue
        bad = state[k]
        fidx, rperm = fr["fidx"], fr["rperm"]
        ii, bi = fidx[:ni], fidx[ni:]
        A = fr["LF"][:ni]
        XL, XU = fr["inv"][bs]
        nblk = (ni + bs - 1) // bs
        v = ys[k].copy()
        if nb and not fr.get("compressed"):
            if trans == 0:
                B = fr["UR"]
            else:
                B = fr["LF"][ni:].T if (bad == "no_conj" or trans == 1) else fr["LF"][ni:].conj().T
            v -= B @ b[bi]
        x = np.zeros(ni, dtype=b.dtype)
        for j in range(nblk - 1, -1, -1):
            s = slice(j * bs, min(ni, (j + 1) * bs))
            wl = s.stop - s.start
            acc = v[s].copy()
            for q in range(nblk - 1, j, -1):
                sq = slice(q * bs, min(ni, (q + 1) * bs))
                B = A[s, sq] if trans == 0 else _op(A[sq, s], trans)
                xq = x[sq]
                if bad == "skip_column" and q == nblk - 1:
                    B, xq = B[:, :-1], xq[:-1]
                acc -= B @ xq
            X = np.triu(XU[j][:wl, :wl]) if trans == 0 else _op(np.tril(XL[j][:wl, :wl]), trans)
            x[s] = X @ acc
        if trans == 0:
            b[ii] = x
        elif bad == "rperm_side":
            b[ii] = x[rperm]
        else:
            b[ii[rperm]] = x
        xs.append(x)
    return dict(y=ys, x=xs, b_fwd=b_fwd, b_bwd=b)


def make_ids(rng, sizes, slack=1.3):
    """Disjoint global ids for fronts of sizes (ni, nb): a random permutation of a subset of range(n), n about `slack` times the ids used.
    Returns (n, [ids of front k])."""
    tot = sum(ni + nb for ni, nb in sizes)
    n = max(int(slack * tot) + 1, 1)
    ids = rng.permutation(n)[:tot]
    out, o = [], 0
    for ni, nb in sizes:
        out.append(ids[o:o + ni + nb].astype(np.int64))
        o += ni + nb
    return n, out
