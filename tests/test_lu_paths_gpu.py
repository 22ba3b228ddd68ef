"""The default LU of a dense front -- optimistic pivoting with diagonal-block-first 256-column groups -- held to tests/lu_mirror.py through
hsk_front_batch_{d,z} (include/hs_kernels.h), which schedules a batch the way hs_numeric schedules a level:

  mode 1  optimistic pivoting without solve descriptors (full-height panels, 32-row TRSM base case)
  mode 2  optimistic pivoting with solve descriptors, the production default: group256 chains, inv256, the 256-row TRSM base case
          (GemmOp::ainv 3..6) and the multipliers below a group (ainv 7 / 8, ComplexF64 16..19), which check the growth bound
  mode 3  tournament pivoting with solve descriptors: what a level runs after its growth flag went up

The pivot order must be the mirror's exactly, the factors within 1e-12; the growth flag must rise for a planted multiplier >= 6 wherever it
sits and stay down for <= 3; the stored inverses must invert the triangular blocks they stand for.  A last test makes a level redo itself."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lu_mirror import find_good_front, optimistic_lu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def front_batch(hs, Fs, nis, mode, inverses=False):
    """Factor the fronts Fs (list of m x m arrays, ni = nis[k]) in ONE hsk_front_batch call; returns one dict per front."""
    cplx = np.iscomplexobj(Fs[0])
    dt = np.complex128 if cplx else np.float64
    ni = np.asarray(nis, dtype=np.int64)
    ms = np.asarray([F.shape[0] for F in Fs], dtype=np.int64)
    nb = ms - ni
    Fp = np.concatenate([np.asarray(F, dtype=dt).ravel(order="F") for F in Fs])
    LF = np.zeros(int((ms * ni).sum()) + 1, dtype=dt)
    UR = np.zeros(int((ni * nb).sum()) + 1, dtype=dt)
    SB = np.zeros(int((nb * nb).sum()) + 1, dtype=dt)
    rp = np.zeros(int(ni.sum()) + 1, dtype=np.int64)
    info = np.zeros(len(Fs), dtype=np.int64)
    growth = np.zeros(len(Fs), dtype=np.int64)
    n32 = (ni + 31) // 32 * 1024
    n256 = (ni + 255) // 256 * 65536
    iL = iU = jL = jU = None
    if inverses:
        iL, iU = np.zeros(int(n32.sum()) + 1, dtype=dt), np.zeros(int(n32.sum()) + 1, dtype=dt)
        jL, jU = np.zeros(int(n256.sum()) + 1, dtype=dt), np.zeros(int(n256.sum()) + 1, dtype=dt)
    L = hs._lib.lib()
    fn = L.hsk_front_batch_z if cplx else L.hsk_front_batch_d
    hs._lib.check(fn(len(Fs), _pi(ni), _pi(nb), mode, _pd(Fp), _pd(LF), _pd(UR), _pd(SB), _pi(rp), _pi(info), _pi(growth),
                     _pd(iL), _pd(iU), _pd(jL), _pd(jU), None))
    out = []
    o = dict(lf=0, ur=0, sb=0, rp=0, i32=0, i256=0)
    for k in range(len(Fs)):
        n, b, m = int(ni[k]), int(nb[k]), int(ms[k])
        r = dict(ni=n, nb=b, info=int(info[k]), growth=int(growth[k]))
        r["LF"] = LF[o["lf"]:o["lf"] + m * n].reshape((m, n), order="F")
        r["UR"] = UR[o["ur"]:o["ur"] + n * b].reshape((n, b), order="F")
        r["SB"] = SB[o["sb"]:o["sb"] + b * b].reshape((b, b), order="F")
        r["rperm"] = rp[o["rp"]:o["rp"] + n]
        if inverses:
            r["invL"] = iL[o["i32"]:o["i32"] + n32[k]].reshape((-1, 32, 32)).transpose(0, 2, 1)  # block b: column-major 32 x 32
            r["invU"] = iU[o["i32"]:o["i32"] + n32[k]].reshape((-1, 32, 32)).transpose(0, 2, 1)
            r["inv256L"] = jL[o["i256"]:o["i256"] + n256[k]].reshape((-1, 256, 256)).transpose(0, 2, 1)
            r["inv256U"] = jU[o["i256"]:o["i256"] + n256[k]].reshape((-1, 256, 256)).transpose(0, 2, 1)
        o["lf"] += m * n; o["ur"] += n * b; o["sb"] += b * b; o["rp"] += n; o["i32"] += int(n32[k]); o["i256"] += int(n256[k])
        out.append(r)
    return out


def _rel(a, b):
    nb_ = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb_ if nb_ > 0 else np.linalg.norm(a)


def check_against_mirror(F, ni, r, mir, what):
    """rperm exactly the mirror's, L / U / Lbi within 1e-12, no flag, the Schur complement within 1e-13 cond(Aii)."""
    m = F.shape[0]
    nb = m - ni
    assert r["info"] == 0 and r["growth"] == 0, (what, r["info"], r["growth"], mir["lmax"])
    assert np.array_equal(r["rperm"], mir["rperm"]), (what, np.flatnonzero(r["rperm"] != mir["rperm"])[:8])
    lf = r["LF"]
    L = np.tril(lf[:ni], -1) + np.eye(ni)
    U = np.triu(lf[:ni])
    e = (_rel(L, mir["L"]), _rel(U, mir["U"]), _rel(lf[ni:], mir["Lbi"]) if nb else 0.0)
    assert max(e) <= 1e-12, (what, e)
    if nb:
        Aii, Aib, Abi, Abb = F[:ni, :ni], F[:ni, ni:], F[ni:, :ni], F[ni:, ni:]
        Sref = Abb - Abi @ np.linalg.solve(Aii, Aib) if ni else Abb
        cond = np.linalg.cond(Aii) if ni else 1.0
        assert _rel(r["SB"], Sref) <= 1e-13 * max(cond, 10.0), (what, _rel(r["SB"], Sref), cond)
        if ni:
            assert _rel(L @ r["UR"], Aib[r["rperm"]]) <= 1e-13, what


def check_inverses(r, what):
    """Every stored inverse X of a triangular diagonal block T of the returned factors (L unit lower, U upper), partial last blocks
    included: ||T X - I||_F <= 64 n eps || |T| |X| ||_F."""
    ni = r["ni"]
    lf = r["LF"][:ni]
    L = np.tril(lf, -1) + np.eye(ni)
    U = np.triu(lf)
    for bs, kl, ku in ((32, "invL", "invU"), (256, "inv256L", "inv256U")):
        for blk in range((ni + bs - 1) // bs):
            c0 = blk * bs
            w = min(bs, ni - c0)
            for T, X, nm in ((L[c0:c0 + w, c0:c0 + w], r[kl][blk][:w, :w], kl), (U[c0:c0 + w, c0:c0 + w], r[ku][blk][:w, :w], ku)):
                res = np.linalg.norm(T @ X - np.eye(w))
                bound = 64 * w * EPS * np.linalg.norm(np.abs(T) @ np.abs(X))
                assert res <= bound, (what, nm, blk, w, res, bound)


SIZES = [1, 31, 32, 33, 255, 256, 257, 288, 300, 511, 512, 513, 1000]


def _front_pair(ni, cplx):
    """Two nb values per ni (cycled through {0, 1, 37, 300}), so every ni meets two and every nb most ni."""
    nbs = (0, 1, 37, 300)
    i = SIZES.index(ni)
    return nbs[(i + cplx) % 4], nbs[(i + 2 + cplx) % 4]


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ni", SIZES)
def test_optimistic_matches_mirror(hs, ni, cplx):
    rng = np.random.default_rng(1000 * cplx + ni)
    fronts = [find_good_front(rng, ni, nb, cplx) for nb in _front_pair(ni, cplx)]
    for mode in (1, 2):
        res = front_batch(hs, [F for F, _ in fronts], [ni, ni], mode, inverses=(mode == 2))
        for (F, mir), r in zip(fronts, res):
            check_against_mirror(F, ni, r, mir, (mode, ni, F.shape[0] - ni, cplx))
            if mode == 2:
                check_inverses(r, (ni, cplx))
    assert ni < 4 or any(np.any(mir["rperm"] != np.arange(ni)) for _, mir in fronts)  # the fronts do pivot


@pytest.mark.parametrize("wl", [1, 64, 65, 128, 129, 192, 193])
def test_optimistic_complex_group_widths(hs, wl):
    """ComplexF64 forms the multipliers below a group one 64-column block q at a time (ainv 16 + q): every partial width of the last group."""
    rng = np.random.default_rng(77 + wl)
    ni = 256 + wl
    fronts = [find_good_front(rng, ni, nb, True) for nb in (0, 40)]
    res = front_batch(hs, [F for F, _ in fronts], [ni, ni], 2, inverses=True)
    for (F, mir), r in zip(fronts, res):
        check_against_mirror(F, ni, r, mir, (ni, F.shape[0] - ni))
        check_inverses(r, ni)


MIXED = [(600, 300), (40, 0), (257, 7), (513, 129), (1, 1), (0, 5)]


@pytest.mark.parametrize("cplx", [False, True])
def test_mixed_batch(hs, cplx):
    """One call, fronts of different sizes: every op is clipped per front (resolve_op), every front keeps its own flag.  A front without
    interior DOFs passes its Abb through."""
    rng = np.random.default_rng(5 + cplx)
    fronts = [find_good_front(rng, ni, nb, cplx) if ni else (rng.standard_normal((nb, nb)) * (1 + 1j if cplx else 1), None) for ni, nb in MIXED]
    nis = [ni for ni, _ in MIXED]
    for mode in (1, 2):
        res = front_batch(hs, [F for F, _ in fronts], nis, mode, inverses=(mode == 2))
        for (F, mir), r, ni in zip(fronts, res, nis):
            if ni == 0:
                assert np.array_equal(r["SB"], F) and r["info"] == 0 and r["growth"] == 0
                continue
            check_against_mirror(F, ni, r, mir, (mode, ni, cplx))
            if mode == 2:
                check_inverses(r, (ni, cplx))


# ---- the growth flag, by position -------------------------------------------------------------------------------------------------------

def _plant(F, mir, row, col, target):
    """Change F[row, col] so that the multiplier of row `row` at column `col` becomes `target` (abs1), row in a later 32-row block than
    column col (so not one of its pivot candidates).  Exact: l[row, col] = (a[row, col] - sum_j<col l[row, j] u[j, col]) / u[col, col]
    with every earlier multiplier of the row and every pivot unchanged."""
    assert row // 32 > col // 32
    G = F.copy()
    d = (1 - 0.5j) / 1.5 if np.iscomplexobj(F) else 1.0  # abs1(d) = 1
    G[row, col] += (target * d - mir["L"][row, col]) * mir["U"][col, col]
    return G


def _growth_cases(cplx):
    """(row, column) of planted multipliers for a front of 600 interior DOFs (groups 0..255, 256..511, 512..599)."""
    cases = [(40, 3, "same group, next 32-block (panel chain under rlim)"), (200, 100, "same group, other 32-block")]
    for off in (0, 127, 128, 255):
        cases.append((256 + off, 17, f"below group 0, offset {off}"))
    cases.append((599, 300, "last partial group, below group 1"))
    for c in ((0, 127, 128, 255) if not cplx else (0, 63, 64, 127, 128, 191, 192, 255)):
        cases.append((300, c, f"group 0 column {c}"))
    return cases


# planted multipliers of 2.9 that must NOT raise the flag: the last column of a 32-block, so nothing else in the row moves much
LOW_CASES = [(40, 31, "same group"), (300, 127, "below group 0, column 127"), (383, 255, "below group 0, column 255"), (599, 287, "below group 1")]


@pytest.mark.parametrize("cplx", [False, True])
def test_growth_flag_by_position(hs, cplx):
    """A multiplier of 8 must raise the flag wherever it sits -- in the group's own rows (panel_l21 under rlim), below the group
    (ainv 7 / 8, 16..19, every column block and row offset), in the last partial group -- in modes 1 and 2; 2.9 must not.  All planted
    fronts go in one batch beside a clean one, so only the planted fronts may raise their flags."""
    ni, nb = 600, 20
    rng = np.random.default_rng(31 + cplx)
    F0, mir0 = find_good_front(rng, ni, nb, cplx, lmax_max=2.0)
    fronts, expect, what = [F0], [0], ["clean"]
    for row, col, nm in _growth_cases(cplx):
        fronts.append(_plant(F0, mir0, row, col, 8.0))
        expect.append(1)
        what.append(nm + " (8)")
    lows = []
    for row, col, nm in LOW_CASES:
        G = _plant(F0, mir0, row, col, 2.9)
        mir = optimistic_lu(G, ni)
        assert 2.8 <= mir["lmax"] <= 3.0 and mir["gap"] >= 1e-10, (nm, mir["lmax"])
        fronts.append(G)
        expect.append(0)
        what.append(nm + " (2.9)")
        lows.append((G, mir))
    for mode in (1, 2):
        res = front_batch(hs, fronts, [ni] * len(fronts), mode)
        got = [r["growth"] for r in res]
        assert got == expect, (mode, [(w, g) for w, g, e in zip(what, got, expect) if g != e])
        assert all(r["info"] == 0 for r in res)
        check_against_mirror(F0, ni, res[0], mir0, (mode, "clean"))
        for (G, mir), r in zip(lows, res[-len(lows):]):
            check_against_mirror(G, ni, r, mir, (mode, "planted 2.9"))


@pytest.mark.parametrize("cplx", [False, True])
def test_growth_flag_nan_zero_column_and_abi(hs, cplx):
    """A NaN below the diagonal block and a diagonal-block column that is zero on its own rows only must raise the flag; huge entries in
    the Abi rows (rows >= ni) must not, and the factors must still match."""
    ni, nb = 300, 30
    rng = np.random.default_rng(41 + cplx)
    F0, mir0 = find_good_front(rng, ni, nb, cplx)
    nan_in_group = F0.copy()
    nan_in_group[100, 40] = np.nan
    nan_below = F0.copy()
    nan_below[290, 10] = np.nan
    zero_col = F0.copy()
    c = 32 + 5  # panel 32..63: clear the block's rows left of it and column c on the block's rows -> no candidate; nonzero below
    zero_col[32:64, :32] = 0.0
    zero_col[32:64, c] = 0.0
    zero_col[100, c] = 1.0
    assert optimistic_lu(zero_col, ni)["bad"]
    abi = F0.copy()
    abi[ni + 3, 7] = 1e8
    abi[ni + nb - 1, 290] = -1e8
    mir_abi = optimistic_lu(abi, ni)
    assert not mir_abi["flag"]
    fronts = [nan_in_group, F0, nan_below, zero_col, abi]
    for mode in (1, 2):
        res = front_batch(hs, fronts, [ni] * len(fronts), mode)
        assert [r["growth"] for r in res] == [1, 0, 1, 1, 0], mode
        check_against_mirror(F0, ni, res[1], mir0, (mode, "clean"))
        check_against_mirror(abi, ni, res[4], mir_abi, (mode, "abi"))


# ---- tournament pivoting with descriptors (a redone level) ------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
def test_tournament_with_descriptors(hs, cplx):
    """Mode 3 on fronts that need pivots from outside their diagonal blocks: backward error, the stored inverses, and for an exactly zero
    column k of Aii, info == k + 1 (include/hs_kernels.h)."""
    rng = np.random.default_rng(51 + cplx)
    shapes = [(600, 50), (257, 0), (70, 9), (513, 30)]
    fronts = []
    for ni, nb in shapes:
        m = ni + nb
        F = rng.standard_normal((m, m)) + (1j * rng.standard_normal((m, m)) if cplx else 0)
        F[np.arange(ni), np.arange(ni)] = 0.0  # zero diagonal: the diagonal blocks alone do not suffice
        fronts.append(F)
    res = front_batch(hs, fronts, [s[0] for s in shapes], 3, inverses=True)
    for F, r, (ni, nb) in zip(fronts, res, shapes):
        assert r["info"] == 0 and r["growth"] == 0, (ni, r["info"], r["growth"])
        assert sorted(r["rperm"].tolist()) == list(range(ni))
        lf = r["LF"]
        L = np.tril(lf[:ni], -1) + np.eye(ni)
        U = np.triu(lf[:ni])
        Aii = F[:ni, :ni]
        assert np.linalg.norm(L @ U - Aii[r["rperm"]]) <= 1e-13 * np.linalg.norm(Aii), ni
        if nb:
            assert np.linalg.norm(lf[ni:] @ U - F[ni:, :ni]) <= 1e-13 * np.linalg.norm(F), ni
        check_inverses(r, (ni, cplx))
    # exactly zero columns: the FIRST one is reported, 1-based
    sing = []
    for ni, nb, k in ((300, 10, 37), (600, 0, 290), (40, 8, 5)):
        m = ni + nb
        F = rng.standard_normal((m, m)) + (1j * rng.standard_normal((m, m)) if cplx else 0)
        F[:ni, k] = 0.0
        F[:ni, k + 3] = 0.0
        sing.append((F, ni, k))
    res = front_batch(hs, [s[0] for s in sing], [s[1] for s in sing], 3)
    assert [r["info"] for r in res] == [k + 1 for _, _, k in sing]


def test_hook_argument_checks(hs):
    L = hs._lib.lib()
    ni = np.array([4], dtype=np.int64)
    nb = np.array([0], dtype=np.int64)
    F = np.eye(4)
    inv = np.zeros(1024)
    for mode in (-1, 8):  # (0..3 with or without bit 2, Sched::aligned16: tests/test_lu_lookahead_gpu.py)
        assert L.hsk_front_batch_d(1, _pi(ni), _pi(nb), mode, _pd(F), None, None, None, None, None, None, None, None, None, None, None) != 0
    assert L.hsk_front_batch_d(0, _pi(ni), _pi(nb), 1, _pd(F), None, None, None, None, None, None, None, None, None, None, None) != 0
    assert L.hsk_front_batch_d(1, _pi(ni), _pi(nb), 1, _pd(F), None, None, None, None, None, None, _pd(inv), None, None, None, None) != 0
    bad = np.array([-1], dtype=np.int64)
    assert L.hsk_front_batch_d(1, _pi(bad), _pi(nb), 1, _pd(F), None, None, None, None, None, None, None, None, None, None, None) != 0


# ---- group256_kernel (HS_GROUP_FUSED=1, read once per process) --------------------------------------------------------------------------

_FUSED_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, hsamd
import test_lu_paths_gpu as T
from lu_mirror import find_good_front
hs = hsamd.load()
rng = np.random.default_rng(61)
fronts = [find_good_front(rng, ni, nb, False) for ni, nb in ((600, 40), (257, 0), (513, 129), (33, 5))]
res = T.front_batch(hs, [F for F, _ in fronts], [600, 257, 513, 33], 2, inverses=True)
for (F, mir), r in zip(fronts, res):
    T.check_against_mirror(F, r["ni"], r, mir, ("fused", r["ni"]))
    T.check_inverses(r, ("fused", r["ni"]))
F0, mir0 = find_good_front(rng, 600, 20, False, lmax_max=2.0)
cases = [(40, 3), (200, 100), (256, 17), (511, 255)]
G = [F0] + [T._plant(F0, mir0, r, c, 8.0) for r, c in cases] + [T._plant(F0, mir0, 40, 31, 2.9)]
res = T.front_batch(hs, G, [600] * len(G), 2)
assert [r["growth"] for r in res] == [0, 1, 1, 1, 1, 0], [r["growth"] for r in res]
T.check_against_mirror(F0, 600, res[0], mir0, "fused clean")
print("FUSED OK")
"""


def test_group256_fused_kernel():
    code = _FUSED_CHILD % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, HS_GROUP_FUSED="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FUSED OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


# ---- a capped trailing update: workgroups that walk several tiles (HS_LA_GEMM_CAP, read once per process) ---------------------------------

_CAP_CHILD = r"""
import sys, hashlib
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, hsamd
import test_lu_paths_gpu as T
hs = hsamd.load()
rng = np.random.default_rng(71)
ni, nb = 640, 40
F = rng.standard_normal((ni + nb, ni + nb))
F[np.arange(ni), np.arange(ni)] = 0.0
r = T.front_batch(hs, [F], [ni], 0)[0]
assert r["info"] == 0, r["info"]
L = np.tril(r["LF"][:ni], -1) + np.eye(ni)
assert np.linalg.norm(L @ np.triu(r["LF"][:ni]) - F[:ni, :ni][r["rperm"]]) <= 1e-13 * np.linalg.norm(F[:ni, :ni])
h = hashlib.sha256()
for k in ("LF", "UR", "SB", "rperm"):
    h.update(np.ascontiguousarray(r[k]).tobytes())
print("CAP", h.hexdigest())
print("RUNS", hs._lib.lib().hsk_lookahead_runs(0))
"""


def test_capped_update_walks_tiles_bitwise():
    """A lone front (ni = 640, nb = 40: 680 rows) under tournament pivoting with look-ahead in 128-column blocks (HS_LA_MIN, HS_LA_NB): the
    first trailing update that runs next to a panel covers rows 128.. and columns 256.. of LF, 552 x 384 = 5 x 3 = 15 tiles of 128 x 128.
    HS_LA_GEMM_CAP=8 launches it with 8 workgroups, seven of which walk two tiles (GemmOp::cap, gemm_dispatch); the default cap (448) gives
    every tile a workgroup.  Which workgroup computes a tile does not change what is computed: factors, Schur complement and pivots are equal
    bit for bit.
    The capped path is taken only while Sched::factor_fronts looks ahead for this front (a second stream, mode 0 = tournament pivoting,
    ni >= HS_LA_MIN): both children report hsk_lookahead_runs, and it must show that they did."""
    code = _CAP_CHILD % (ROOT, os.path.join(ROOT, "tests"))
    out = []
    for cap in ("8", None):
        env = dict(os.environ, HS_LA_MIN="256", HS_LA_NB="128")
        env.pop("HS_LA_GEMM_CAP", None)
        if cap:
            env["HS_LA_GEMM_CAP"] = cap
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (cap, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        out.append([ln for ln in r.stdout.splitlines() if ln.startswith("CAP")])
        runs = [int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("RUNS")]
        assert len(runs) == 1 and runs[0] >= 1, (cap, r.stdout[-2000:])
    assert len(out[0]) == 1 and out[0] == out[1], out


# ---- a level that redoes itself (end to end) --------------------------------------------------------------------------------------------

_REDO_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, scipy.sparse as sp, scipy.sparse.linalg as spla, hsamd
import test_lu_paths_gpu as T
hs = hsamd.load()
A0, nd = T.redo_matrix(hs)
nd, nd_loc = hs.symfact(nd)
perm = hs.postorder(nd)
nd = hs.permuted(nd, hs.invperm(perm))
rng = np.random.default_rng(3)
for cplx in (False, True):
    A = (A0 * (1 + 0.5j) + 0.1j * sp.identity(A0.shape[0])) if cplx else A0
    A = sp.csc_matrix(A[perm - 1][:, perm - 1])
    b = rng.standard_normal(A.shape[0]) + (1j * rng.standard_normal(A.shape[0]) if cplx else 0)
    print("BEGIN", cplx, file=sys.stderr, flush=True)
    F = hs.factor(A, nd, nd_loc, swlevel=0, verbose=True)
    x = hs.ldiv(F, b)
    berr = np.abs(b - A @ x).max() / (spla.norm(A, np.inf) * np.abs(x).max() + np.abs(b).max())
    xs = spla.splu(A).solve(b)
    print("RES", int(cplx), berr, np.linalg.norm(x - xs) / np.linalg.norm(xs), hs.condest(F), flush=True)
    F.free()
"""


def redo_matrix(hs, n=20, nmax=100):
    """A 7-point pattern on an n^3 grid (x fastest), diagonally dominant except among the DOFs of the root separator (the planes
    x = n/2 - 1 and x = n/2 of the geometric nested dissection): there the diagonal is tiny and the couplings to z +- 1 dominate
    (+10 up, -10 down: a nonsingular skew chain).  In the root front's order a z-neighbour sits 2n rows away -- outside the 32-row diagonal
    block -- so optimistic pivoting must give up on the root, and only there.  Returns (A, raw elimination tree)."""
    import scipy.sparse as sp

    N = n ** 3
    g = np.arange(N)
    x, y, z = g % n, (g // n) % n, g // (n * n)
    sep = (x == n // 2 - 1) | (x == n // 2)
    rows, cols, vals = [g], [g], [np.where(sep, 1e-2, 6.5)]
    for d, ok in ((1, x < n - 1), (n, y < n - 1), (n * n, z < n - 1)):
        i = g[ok]
        j = i + d
        both = sep[i] & sep[j] & (d == n * n)
        rows += [i, j]
        cols += [j, i]
        vals += [np.where(both, 10.0, -1.0), np.where(both, -10.0, -1.0)]
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    nd = hs.problems.grid_nested_dissection((n, n, n), nmax)
    return A, nd


def test_level_redoes_itself():
    """No forcing: the root of a real factorization needs pivots from outside its diagonal blocks, the growth flag rises, the root level
    -- and only it -- is redone with tournament pivoting, Float64 and ComplexF64, and the solution is backward stable.  The root is level 1
    of the handle (level 0 would hold a pseudo-root for a boundary of the root; this tree has none)."""
    code = _REDO_CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    for part in r.stderr.split("BEGIN")[1:]:
        lines = [ln for ln in part.splitlines() if "redoing the level with tournament pivoting" in ln]
        assert len(lines) == 1 and "level 1:" in lines[0], lines
    res = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("RES")]
    assert len(res) == 2, r.stdout
    for _, cplx, berr, err, cond in res:
        berr, err, cond = float(berr), float(err), float(cond)
        assert berr <= 1e-13, (cplx, berr)
        assert err <= 1e-12 * cond, (cplx, err, cond)
