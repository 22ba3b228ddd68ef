"""The rank-revealing orthogonalisation of the HSS module (qr_refine, csrc/hs_hss.hip: chol_block_kernel, qr_select_kernel, rownorm2_kernel
and the host state machine) against its NumPy mirror in extended precision (tests/qr_mirror.py), through the hooks hsk_qr_* that call the
production launches.  Decisions (ranks, row orders, accepted blocks, counters) are compared exactly: tests/test_qr_refine_host.py has checked
on the CPU that every input here decides each comparison by a relative margin >= 1e-6.  Numbers are compared within BOUND_D / BOUND_T of
qr_mirror.py (16 times the distance between the float64 and the extended-precision mirror), never within something the device gave."""
import ctypes as C

import numpy as np
import pytest

import qr_mirror as Q

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


@pytest.fixture(scope="module")
def P(hs):
    return Q.params(hs)


_REF = {}


def ref(c, order, P):
    """The extended-precision mirror of a case, computed once for the module."""
    key = (id(c["M"]), c["name"], c["rmax"], c["atol"], c["rtol"], c["scale_floor"], c["atol_scale"], c["floor_abs"], order)
    if key not in _REF:
        _REF[key] = (c, Q.run_case(c, order, P, np.longdouble))  # (holds c: the id stays unique)
    return _REF[key][1]


_CASES = {}


def cases(cplx):
    if cplx not in _CASES:
        _CASES[cplx] = Q.refine_cases(cplx)
    return _CASES[cplx]


def by_name(cplx, name):
    return next(c for c in cases(cplx) if c["name"] == name)


# ---------------------------------------------------------------------------------------------------------------------------------
# hooks
# ---------------------------------------------------------------------------------------------------------------------------------
def dev_chol(hs, jobs, cplx, W, sentinel=-7.5):
    """hsk_qr_chol_* on a list of chol_cases jobs (one launch).  Outputs start as `sentinel` (ints: -7): what the kernel leaves alone shows."""
    n = len(jobs)
    dt = np.complex128 if cplx else np.float64
    b = np.array([j["b"] for j in jobs], dtype=np.int32)
    first = np.array([j["first"] for j in jobs], dtype=np.int32)
    G = np.concatenate([np.asfortranarray(j["G"]).ravel(order="F") for j in jobs]).astype(dt)
    thr = np.array([j["thr"] for j in jobs], dtype=np.float64).ravel()
    top = np.array([j["top"] for j in jobs], dtype=np.float64)
    p = np.full(n * W, -7, dtype=np.int32)
    for a, j in enumerate(jobs):
        p[a * W:a * W + j["b"]] = j["p"]
    L, Li, LiP = (np.full(n * W * W, sentinel, dtype=dt) for _ in range(3))
    d = np.full(n * W, sentinel)
    lperm = np.full(n * W, -7, dtype=np.int32)
    nacc = np.full(n, -7, dtype=np.int32)
    lib = hs._lib.lib()
    fn = lib.hsk_qr_chol_z if cplx else lib.hsk_qr_chol_d
    hs._lib.check(fn(n, _pi(b), _pi(first), _pd(G), _pd(thr), _pd(top), _pi(p), _pd(L), _pd(Li), _pd(LiP), _pd(d), _pi(lperm), _pi(nacc)))
    sq = lambda x, a: x[a * W * W:(a + 1) * W * W].reshape((W, W), order="F")
    return [{"L": sq(L, a), "Linv": sq(Li, a), "LinvP": sq(LiP, a), "d": d[a * W:(a + 1) * W], "top": top[a], "p": p[a * W:(a + 1) * W],
             "lperm": lperm[a * W:(a + 1) * W], "nacc": int(nacc[a])} for a in range(n)]


def dev_select(hs, sel):
    """hsk_qr_select on a list of (name, m, done, want, p, res2) (one launch): [(p, outmax)]."""
    n = len(sel)
    m = np.array([s[1] for s in sel], dtype=np.int32)
    done = np.array([s[2] for s in sel], dtype=np.int32)
    want = np.array([s[3] for s in sel], dtype=np.int32)
    p = np.concatenate([s[4] for s in sel]).astype(np.int32)
    res2 = np.concatenate([s[5] for s in sel]).astype(np.float64)
    om = np.full(2 * n, -7.5)
    hs._lib.check(hs._lib.lib().hsk_qr_select(n, _pi(m), _pi(done), _pi(want), _pi(p), _pd(res2), _pd(om)))
    off = np.concatenate([[0], np.cumsum(m)])
    return [(p[off[a]:off[a + 1]], om[2 * a:2 * a + 2]) for a in range(n)]


def dev_refine(hs, cs, order, cplx):
    """hsk_qr_refine_* on a list of cases that share atol, rtol and scale_floor (one qr_refine call): ([per-job dict], windows, refreshes)."""
    n = len(cs)
    assert len({(c["atol"], c["rtol"], c["scale_floor"]) for c in cs}) == 1
    dt = np.complex128 if cplx else np.float64
    m = np.array([c["M"].shape[0] for c in cs], dtype=np.int32)
    q = np.array([c["M"].shape[1] for c in cs], dtype=np.int32)
    M = np.concatenate([np.asarray(c["M"], dtype=dt).ravel(order="F") for c in cs])
    p = np.concatenate([np.arange(mm) if order else c["p"] for c, mm in zip(cs, m)]).astype(np.int32)
    rmax = np.array([c["rmax"] for c in cs], dtype=np.int32)
    asc = np.array([c["atol_scale"] for c in cs], dtype=np.float64)
    fl = np.array([c["floor_abs"] for c in cs], dtype=np.float64)
    tot = int(m.sum())
    offm = np.concatenate([[0], np.cumsum(m)])
    offT = np.concatenate([[0], np.cumsum(m.astype(np.int64) * np.minimum(m, q))])
    r = np.full(n, -7, dtype=np.int32)
    top = np.full(n, -7.5)
    d = np.full(tot, -7.5)
    T = np.full(int(offT[-1]) + 1, -7.5, dtype=dt)
    blocks = np.full(2 * tot, -7, dtype=np.int32)
    nb = np.full(n, -7, dtype=np.int32)
    cnt = np.zeros(2, dtype=np.int64)
    lib = hs._lib.lib()
    fn = lib.hsk_qr_refine_z if cplx else lib.hsk_qr_refine_d
    c0 = cs[0]
    hs._lib.check(fn(n, _pi(m), _pi(q), _pd(M), _pi(p), _pi(rmax), _pd(asc), _pd(fl), int(order), c0["atol"], c0["rtol"], c0["scale_floor"], _pi(r), _pd(top), _pd(d),
                     _pd(T), _pi(blocks), _pi(nb), cnt.ctypes.data_as(C.POINTER(C.c_int64))))
    out = []
    for a in range(n):
        ra, nR = int(r[a]), int(m[a] - r[a])
        bl = blocks[2 * offm[a]:2 * offm[a] + 2 * nb[a]]
        out.append({"r": ra, "top": float(top[a]), "p": p[offm[a]:offm[a + 1]].astype(np.int64), "d": d[offm[a]:offm[a] + ra].copy(),
                    "T": T[offT[a]:offT[a] + nR * ra].reshape((nR, ra), order="F").copy(), "blocks": [(int(bl[2 * i]), int(bl[2 * i + 1])) for i in range(nb[a])]})
    return out, int(cnt[0]), int(cnt[1])


def run_groups(hs, cs, order, cplx):
    """Every case of `cs` that runs in `order`, grouped into one call per (atol, rtol, scale_floor): {name: device result}, windows, refreshes."""
    groups = {}
    for c in cs:
        if order in c["orders"]:
            groups.setdefault((c["atol"], c["rtol"], c["scale_floor"]), []).append(c)
    res, w, f = {}, 0, 0
    for g in groups.values():
        out, gw, gf = dev_refine(hs, g, order, cplx)
        w, f = w + gw, f + gf
        for c, o in zip(g, out):
            res[c["name"]] = o
    return res, w, f


def compare(c, dev, mir, worst):
    """Decisions exactly, numbers within the bound of section 5; worst = [d, T] collects the largest scaled distances."""
    name = c["name"]
    assert dev["r"] == mir["r"], (name, dev["r"], mir["r"])
    assert dev["blocks"] == mir["blocks"], (name, dev["blocks"], mir["blocks"])
    assert np.array_equal(dev["p"], mir["p"]), name
    if c["rank"] is not None:
        assert dev["r"] == c["rank"], (name, dev["r"])
    assert dev["top"] == (dev["d"][0] if dev["r"] > 0 else mir["top"]), name
    assert abs(dev["top"] - mir["top"]) <= (c["M"].shape[1] + 4) * EPS * mir["top"], name  # the norm of a row of q entries
    dd, dt = Q.scaled_distances(c["M"], mir, dev["d"], dev["T"])
    worst[0], worst[1] = max(worst[0], dd), max(worst[1], dt)
    assert dd <= Q.BOUND_D and dt <= Q.BOUND_T, (name, dd, dt)


# ---------------------------------------------------------------------------------------------------------------------------------
# chol_block_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
def test_chol_block_kernel_against_the_mirror(hs, P, cplx):
    W = P["W"]
    jobs = Q.chol_cases(cplx, P)
    assert {j["b"] for j in jobs} >= {1, 2, 31, 63, 64}
    out = dev_chol(hs, jobs, cplx, W)  # a batch mixing every b and every stop rule
    for j, o in zip(jobs, out):
        name = j["name"]
        mir = Q.run_chol_case(j, P, np.longdouble)
        b, na = j["b"], o["nacc"]
        assert na == mir["na"] and (j["nacc"] is None or na == j["nacc"]), (name, na, mir["na"])
        assert list(o["lperm"][:b]) == mir["perm"] and np.all(o["lperm"][b:] == -7), name
        assert list(o["p"][:b]) == [int(j["p"][i]) for i in mir["perm"]] and np.all(o["p"][b:] == -7), name
        # top is written only with first
        assert o["top"] == (o["d"][0] if na > 0 else 0.0) if j["first"] else o["top"] == j["top"], name
        L, Li, LiP = o["L"], o["Linv"], o["LinvP"]
        # outside na x na: L untouched, Linv and LinvP exactly zero; above the diagonal of L exactly zero
        mask = np.zeros((W, W), dtype=bool)
        mask[:na, :na] = True
        assert np.all(L[~mask] == -7.5) and np.all(Li[~mask] == 0) and np.all(LiP[na:, :] == 0) and np.all(LiP[:, b:] == 0), name
        assert np.all(np.triu(L[:na, :na], 1) == 0) and np.all(np.triu(Li[:na, :na], 1) == 0), name
        assert np.all(o["d"][na:] == -7.5), name
        if na == 0:
            continue
        Ln = L[:na, :na]
        assert np.array_equal(o["d"][:na], Ln.diagonal().real) and np.all(Ln.diagonal().imag == 0), name  # d = diag L, copied
        # LinvP = Linv * P: column perm[c] of LinvP is column c of Linv, copied; the other columns are zero
        Pm = np.zeros((na, W))
        Pm[np.arange(na), mir["perm"][:na]] = 1.0
        assert np.array_equal(LiP[:na, :], Li[:na, :na] @ Pm), name
        # L L^H = the permuted Gram block: a Cholesky factorization is backward stable, |G - L L^H| <= (na + 1) eps |L| |L^H| entrywise
        # (Higham, Accuracy and Stability, thm 10.3); 4 for the complex arithmetic
        Gp = j["G"][np.ix_(mir["perm"][:na], mir["perm"][:na])]
        bound = 4 * (na + 1) * EPS * (np.abs(Ln) @ np.abs(Ln).conj().T)
        assert np.all(np.abs(Ln @ Ln.conj().T - Gp) <= bound), (name, np.max(np.abs(Ln @ Ln.conj().T - Gp) / bound))
        # the kernel solves L x = e_c column by column: |L Linv - I| <= na eps |L| |Linv| entrywise (Higham thm 8.5), 4 as above; and
        # Linv L - I = Linv (L Linv - I) L is bounded through that
        Lin = Li[:na, :na]
        bound = 4 * na * EPS * (np.abs(Ln) @ np.abs(Lin))
        assert np.all(np.abs(Ln @ Lin - np.eye(na)) <= bound), name
        assert np.all(np.abs(Lin @ Ln - np.eye(na)) <= np.abs(Lin) @ bound @ np.abs(Ln) + 4 * na * EPS * (np.abs(Lin) @ np.abs(Ln))), name
        # d against the extended-precision mirror: the Gram matrix carries d^2, so eps d0^2 / d_k of absolute error per step
        dref = np.asarray(mir["d"], dtype=np.float64)
        assert np.all(np.abs(o["d"][:na] - dref) <= 4 * (na + 1) * EPS * float(mir["d0"]) ** 2 / dref), name
    # one job alone gives the bits it gave in the batch
    k = next(i for i, j in enumerate(jobs) if j["name"] == "strong b = 64")
    alone = dev_chol(hs, [jobs[k]], cplx, W)[0]
    for key in ("L", "Linv", "LinvP", "d", "p", "lperm"):
        assert np.array_equal(alone[key], out[k][key]), key
    assert alone["nacc"] == out[k]["nacc"] and alone["top"] == out[k]["top"]


# ---------------------------------------------------------------------------------------------------------------------------------
# qr_select_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def test_qr_select_kernel_is_the_mirror_exactly(hs):
    sel = Q.select_cases()
    assert {s[1] - s[2] for s in sel} >= {1, 64, 65, 255, 256, 257, 700}
    out = dev_select(hs, sel)  # one launch
    for s, (p1, om) in zip(sel, out):
        name, m, done, want, p0, res2 = s
        pm, omm = Q.select(p0, done, m, want, res2)
        assert np.array_equal(p1, pm), name
        assert om[0] == float(omm[0]) and om[1] == float(omm[1]), (name, om, omm)
        Q.check_selection(name, m, done, want, p0, res2, p1, [float(om[0]), float(om[1])])
    alone = dev_select(hs, [sel[-1]])[0]
    assert np.array_equal(alone[0], out[-1][0]) and np.array_equal(alone[1], out[-1][1])


# ---------------------------------------------------------------------------------------------------------------------------------
# qr_refine
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
def test_qr_refine_in_a_given_order(hs, P, cplx):
    """m in {1, 2, 63, 64, 65, 129, 300} x q in {1, 40, m, m + 37}; rmax below, at and above the rank; the five thresholds binding in turn; the
    conditioning cut-off inside one window; a window that accepts nothing; a zero matrix; rmax = 0."""
    cs = Q.size_cases(cplx) + Q.rule_cases(cplx)
    res, windows, refreshes = run_groups(hs, cs, 0, cplx)
    worst = [0.0, 0.0]
    for c in cs:
        compare(c, res[c["name"]], ref(c, 0, P), worst)
    print(f"given order, cplx={cplx}: largest scaled distance of the device from the extended-precision mirror: d {worst[0]:.3e}, T {worst[1]:.3e}")
    assert windows == sum(ref(c, 0, P)["windows"] for c in cs) and refreshes == 0
    assert len(res["conditioning cut in one window"]["blocks"]) >= 2 and res["conditioning cut in one window"]["r"] == 40
    assert res["second window accepts nothing"]["blocks"][-1] == (0, 64) or sum(w for _, w in res["second window accepts nothing"]["blocks"]) == 64
    z = res["zero matrix"]
    assert z["r"] == 0 and z["top"] == 0.0 and z["blocks"] == []
    assert res["rmax = 0"]["r"] == 0 and res["rmax below the rank"]["r"] == 37 and res["full rank r == m"]["r"] == 70


def mirror_free_checks(c, dev, theta):
    """What a norm-ordered result must satisfy whatever the mirror says (extended-precision residuals along the device's own order)."""
    name, M, r = c["name"], c["M"], dev["r"]
    if r == 0:
        return
    dist, others, resid = Q.residual_norms_along(M, dev["p"], r)
    # every accepted row is the greedy choice up to theta
    assert np.all(dev["d"] >= theta * (1 - 1e-6) * others.astype(np.float64)), (name, float(np.min(dev["d"] / np.where(others > 0, others, 1).astype(np.float64))))
    if r < M.shape[0]:
        # T is the least-squares interpolation: no row is left with more than its residual against the accepted rows
        ct = np.clongdouble if np.iscomplexobj(M) else np.longdouble
        left = np.asarray(M[dev["p"][r:]], dtype=ct) - np.asarray(dev["T"], dtype=ct) @ np.asarray(M[dev["p"][:r]], dtype=ct)
        ln, rn = np.sqrt(Q._rownorm2(left)), np.sqrt(Q._rownorm2(resid))
        # (a row that lies in the span to rounding has no residual to compare with: the rounding of T M[p_S], eps (|row| + |T| |rows of S|),
        # stands in for it)
        floor = 8 * EPS * (np.linalg.norm(M[dev["p"][r:]], axis=1) + np.abs(dev["T"]) @ np.linalg.norm(M[dev["p"][:r]], axis=1))
        assert np.all(ln <= (1 + 1e-6) * rn + floor), (name, float(np.max((ln - floor) / np.where(rn > 0, rn, 1))))


@pytest.mark.parametrize("cplx", [False, True])
def test_qr_refine_in_norm_order(hs, P, cplx):
    """The same sizes and rules with the windows chosen by downdated residual norms, m = 700 (three chunks of the selection) and the refresh."""
    cs = Q.size_cases(cplx) + Q.rule_cases(cplx) + Q.norm_cases(cplx)
    res, windows, refreshes = run_groups(hs, cs, 1, cplx)
    worst = [0.0, 0.0]
    for c in cs:
        compare(c, res[c["name"]], ref(c, 1, P), worst)
        mirror_free_checks(c, res[c["name"]], P["theta"])
    print(f"norm order, cplx={cplx}: largest scaled distance of the device from the extended-precision mirror: d {worst[0]:.3e}, T {worst[1]:.3e}")
    assert windows == sum(ref(c, 1, P)["windows"] for c in cs)
    assert refreshes == sum(ref(c, 1, P)["refreshes"] for c in cs)
    # the refresh case alone: the recomputation fires, at the mirror's step (same blocks), and the designed rank comes out
    c = by_name(cplx, "refresh")
    out, w, f = dev_refine(hs, [c], 1, cplx)
    mir = ref(c, 1, P)
    assert f >= 1 and f == mir["refreshes"] and w == mir["windows"] and out[0]["r"] == 100 and out[0]["blocks"] == mir["blocks"]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("cplx", [False, True])
def test_a_batch_is_its_jobs_run_alone(hs, P, cplx, order):
    cs = Q.batch_cases(cplx)
    assert len(cs) == 6
    batch, w, f = dev_refine(hs, cs, order, cplx)
    worst = [0.0, 0.0]
    ws = fs = 0
    for c, b in zip(cs, batch):
        (a,), wa, fa = dev_refine(hs, [c], order, cplx)
        ws, fs = ws + wa, fs + fa
        assert a["r"] == b["r"] and a["blocks"] == b["blocks"] and a["top"] == b["top"], c["name"]
        if c["rmax"] > 0:
            assert np.array_equal(a["p"], b["p"]), c["name"]
        compare(c, b, ref(c, order, P), worst)
    assert (w, f) == (ws, fs)
    assert len({ref(c, order, P)["windows"] for c in cs}) >= 3  # the jobs finish at different windows
    assert batch[2]["r"] == 0 and batch[3]["r"] == 0 and batch[3]["top"] == 0.0


@pytest.mark.parametrize("cplx", [False, True])
def test_lowrank_entry_finds_the_designed_rank_in_both_orders(hs, cplx):
    """hsk_lowrank_* on X = L Q with a gap of 100 around the threshold (a factor 10 on either side): the rank is the designed one exactly."""
    def compress(X, atol, rtol, kinit=64, seed=1):
        rows, cols = X.shape
        cap = min(rows, cols)
        Cbuf, Zbuf = np.zeros(rows * cap, dtype=X.dtype), np.zeros(cap * cols, dtype=X.dtype)
        r = C.c_int64(0)
        lib = hs._lib.lib()
        fn = lib.hsk_lowrank_z if cplx else lib.hsk_lowrank_d
        hs._lib.check(fn(rows, cols, _pd(np.asfortranarray(X)), atol, rtol, kinit, seed, C.byref(r), _pd(Cbuf), _pd(Zbuf), cap))
        return r.value, Cbuf[: rows * r.value].reshape((rows, r.value), order="F"), Zbuf[: r.value * cols].reshape((r.value, cols), order="F")

    rows, cols, rank, rtol = 200, 150, 23, 1e-4
    diag = np.concatenate([Q.graded(rank, 1.0, 10 * rtol), Q.graded(cols - rank, rtol / 10, rtol / 100)])
    X = Q.lq_input(rows, cols, diag, "weak", cplx, 61 + cplx)
    try:
        for mode in ("lu", "norm"):
            hs.hss.qr_order(mode)
            r, Cm, Z = compress(X, 0.0, rtol)
            assert r == rank, (mode, r)
            assert np.linalg.norm(X - Cm @ Z, 2) < 50 * rtol
    finally:
        hs.hss.qr_order("lu")
