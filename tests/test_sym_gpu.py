"""The symmetric mode on the device (hs_options.symmetric; Sched::sym, csrc/hs_sched.h; csrc/kernels_sym.hip).

  a  hsk_front_batch_sym_{d,z}: symmetric fronts (sym_mirror.find_sym_front) against lu_mirror.optimistic_lu through check_against_mirror /
     check_inverses of tests/test_lu_paths_gpu.py -- pivots exact, factors within 1e-12 --, the returned Schur complement equal to its
     transpose bit for bit, the look-ahead counter for the fronts large enough to look ahead
  b  executed flops (hsk_op_flops) of a lone Float64 front ni = nb = 2048: at most 0.85 of the general schedule's (the host count of
     tests/test_sym_host.py is 0.8218; measured on an MI355X: 0.8221), and the same factors
  c  the strips compose with the block envelopes: envelope on == envelope off within 1e-12 on the public path
  d  the public path: Poisson and Helmholtz, the option on against the option off -- solution, node blocks, logabsdet, transposed block
     solve, diag(A^-1), hs.sym_info, gemm_flops
  e  a compressed handle: compressed fronts and the dense fronts they feed keep the general path, and sym_info says so
  f  refusals (a matrix that is not symmetric, named by entry; several ranks) and fallbacks (tournament pivoting, a redone level)

Fronts are built once per process and never modified."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from helpers import prepare, relerr
from sym_mirror import find_sym_front, sym_front
from test_lu_paths_gpu import _pd, _pi, check_against_mirror, check_inverses

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGNED = 4
SOL_TOL = 1e-10


@functools.lru_cache(maxsize=None)
def sym_pair(ni, nb, cplx):
    """(F, mirror) of one symmetric front, built once per process and shared: callers must not modify either."""
    return find_sym_front(np.random.default_rng(9000 + 1000 * cplx + ni), ni, nb, cplx)


def batch(hs, Fs, nis, mode, inverses=False, sym=True):
    """front_batch of tests/test_lu_paths_gpu.py through hsk_front_batch_sym_* (sym) or hsk_front_batch_*: one dict per front."""
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
    fn = getattr(L, "hsk_front_batch" + ("_sym" if sym else "") + ("_z" if cplx else "_d"))
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
            r["invL"] = iL[o["i32"]:o["i32"] + n32[k]].reshape((-1, 32, 32)).transpose(0, 2, 1)
            r["invU"] = iU[o["i32"]:o["i32"] + n32[k]].reshape((-1, 32, 32)).transpose(0, 2, 1)
            r["inv256L"] = jL[o["i256"]:o["i256"] + n256[k]].reshape((-1, 256, 256)).transpose(0, 2, 1)
            r["inv256U"] = jU[o["i256"]:o["i256"] + n256[k]].reshape((-1, 256, 256)).transpose(0, 2, 1)
        o["lf"] += m * n; o["ur"] += n * b; o["sb"] += b * b; o["rp"] += n; o["i32"] += int(n32[k]); o["i256"] += int(n256[k])
        out.append(r)
    return out


# ---- a. the hook against the mirror ---------------------------------------------------------------------------------------------------------

# the shapes of tests/test_sym_host.py; (1000, 37): the recursive schedule with strips inside the interior (768 < ni < the look-ahead
# threshold); the mixed batch: smaller fronts clipped out of the later strips, block columns and transpositions
LONE = {False: [(33, 5), (257, 40), (300, 300), (600, 0), (1000, 37), (1537, 37)], True: [(33, 5), (257, 40), (300, 300), (600, 0), (1000, 37), (1200, 37)]}
MIXED = [(700, 40), (257, 0), (1537, 37)]
LOOKAHEAD = {(False, 1537, 37), (True, 1200, 37)}  # these fronts look ahead (Float64 from 1536, ComplexF64 from 1200 interior columns)


def check_batch(hs, shapes, cplx, mode, expect_la):
    L = hs._lib.lib()
    fronts = [sym_pair(ni, nb, cplx) for ni, nb in shapes]
    before = L.hsk_lookahead_runs(0)
    res = batch(hs, [F for F, _ in fronts], [ni for ni, _ in shapes], mode, inverses=bool(mode & 2))
    assert L.hsk_lookahead_runs(0) - before == expect_la, (shapes, mode, L.hsk_lookahead_runs(0) - before)
    for (F, mir), r, (ni, nb) in zip(fronts, res, shapes):
        what = ("sym", mode, ni, nb, cplx)
        check_against_mirror(F, ni, r, mir, what)
        if mode & 2:
            check_inverses(r, what)
        assert np.array_equal(r["SB"], r["SB"].T), what  # plain transpose, bit for bit
        assert np.any(mir["rperm"] != np.arange(ni)), what  # the front pivots


@pytest.mark.parametrize("cplx,mode", [(False, 1), (False, 2), (False, 2 | ALIGNED), (True, 1), (True, 2)])
def test_sym_hook_matches_mirror(hs, cplx, mode):
    """One call per front and mode for the lone shapes; Float64 also the mixed batch in one call."""
    for ni, nb in LONE[cplx]:
        check_batch(hs, [(ni, nb)], cplx, mode, 1 if (cplx, ni, nb) in LOOKAHEAD else 0)
    if cplx:
        check_batch(hs, [(1200, 37), (300, 300), (257, 40)], cplx, mode, 1)
    else:
        check_batch(hs, MIXED, cplx, mode, 1)


def test_sym_hook_refuses_other_modes(hs):
    L = hs._lib.lib()
    ni, nb = np.array([3], dtype=np.int64), np.array([1], dtype=np.int64)
    F = np.eye(4)
    none = (None,) * 11
    for mode in (0, 3, 1 | ALIGNED, 3 | ALIGNED, 8, 12, -1):
        assert L.hsk_front_batch_sym_d(1, _pi(ni), _pi(nb), mode, _pd(F), *none) == hs._lib.HS_ERR_ARGUMENT, mode
        assert L.hsk_front_batch_sym_z(1, _pi(ni), _pi(nb), mode, _pd(np.eye(4, dtype=np.complex128)), *none) == hs._lib.HS_ERR_ARGUMENT, mode
    for mode in (1, 2, 2 | ALIGNED):
        assert L.hsk_front_batch_sym_d(1, _pi(ni), _pi(nb), mode, _pd(F), *none) == 0, mode


# ---- b. executed flops ------------------------------------------------------------------------------------------------------------------------

def test_sym_executed_flops(hs):
    """Lone Float64 front ni = nb = 2048, mode 2: the device's own count of the K-steps it ran (hsk_op_flops) with the strips is at most 0.85
    of the general schedule's (host count 0.8218, tests/test_sym_host.py; measured on an MI355X: 0.8221), and the factors agree.  No NumPy mirror at this size."""
    L = hs._lib.lib()
    ni = nb = 2048
    F = sym_front(np.random.default_rng(9000 + ni), ni, nb, False)
    flops, res = [], []
    assert L.hsk_op_flops_mode(1) == 0
    try:
        for sym in (True, False):
            res.append(batch(hs, [F], [ni], 2, sym=sym)[0])
            out = C.c_double()
            assert L.hsk_op_flops(C.byref(out)) == 0
            flops.append(out.value)
            assert L.hsk_op_flops_mode(1) == 0  # (switching it on again clears the counter)
    finally:
        L.hsk_op_flops_mode(0)
    print(f"[sym flops] device count: symmetric {flops[0]:.6e} general {flops[1]:.6e} ratio {flops[0] / flops[1]:.4f}")
    assert flops[1] > 0 and flops[0] <= 0.85 * flops[1], flops
    a, b = res
    assert a["info"] == 0 and a["growth"] == 0 and b["info"] == 0 and b["growth"] == 0
    assert np.array_equal(a["rperm"], b["rperm"])
    for key in ("LF", "UR", "SB"):
        e = np.abs(a[key] - b[key]).max() / np.abs(b[key]).max()
        assert e <= 1e-12, (key, e)
    assert np.array_equal(a["SB"], a["SB"].T)


# ---- d. the public path -----------------------------------------------------------------------------------------------------------------------

PUBLIC = [((16, 16, 16), "poisson"), ((20, 20, 20), "poisson"), ((12, 12, 12), "helmholtz"), ((16, 16, 16), "helmholtz")]


@functools.lru_cache(maxsize=None)
def problem(shape, kind):
    import hsamd

    return prepare(hsamd.load(), shape, kind=kind, rhs="randn")


def _blocks_agree(F1, F0, tol):
    assert F1.nnodes == F0.nnodes
    for k in range(F1.nnodes):
        b1, b0 = F1.node_blocks(k, with_schur=True), F0.node_blocks(k, with_schur=True)
        assert np.array_equal(b1["rperm"], b0["rperm"]), (k, F1.node_info(k))
        for name in ("LU", "Lbi", "Uib", "S"):
            if b0[name].size:
                assert relerr(b1[name], b0[name]) <= tol, (k, name, F1.node_info(k), relerr(b1[name], b0[name]))


@pytest.mark.parametrize("shape,kind", PUBLIC)
def test_sym_public_path(hs, shape, kind):
    P = problem(shape, kind)
    A, b = P["A"], P["b"]
    assert (A != A.T).nnz == 0
    F1 = hs.factor(A, P["nd"], P["nd_loc"], swlevel=0, keep_schur=True, symmetric=True)
    F0 = hs.factor(A, P["nd"], P["nd_loc"], swlevel=0, keep_schur=True)
    xr = spla.splu(A).solve(b)
    x1, x0 = hs.ldiv(F1, b), hs.ldiv(F0, b)
    assert relerr(x1, xr) <= SOL_TOL and relerr(x0, xr) <= SOL_TOL, (relerr(x1, xr), relerr(x0, xr))
    _blocks_agree(F1, F0, 1e-11)
    i1, i0 = hs.sym_info(F1), hs.sym_info(F0)
    assert i1["option"] and i1["fronts_lower"] >= F1.nnodes and i1["fronts_general"] == 0, i1  # (+ the pseudo-root, if the tree has one)
    assert not i0["option"] and i0["fronts_lower"] == 0 and i0["fronts_general"] == i1["fronts_lower"], (i0, i1)
    s1, s0 = F1.stats(), F0.stats()
    print(f"[sym] {kind} {shape}: gemm_flops on {s1['gemm_flops']:.6e} off {s0['gemm_flops']:.6e} ratio {s1['gemm_flops'] / s0['gemm_flops']:.4f}")
    assert s1["gemm_flops"] <= s0["gemm_flops"]
    if shape == (20, 20, 20):
        assert s1["gemm_flops"] < s0["gemm_flops"]
    # the solve phase reads the same layout
    (l1, g1), (l0, g0) = hs.logabsdet(F1), hs.logabsdet(F0)
    assert abs(l1 - l0) <= 1e-11 * abs(l0) and abs(g1 - g0) <= 1e-11, (l1, l0, g1, g0)
    B = np.asfortranarray(np.stack([b, b[::-1]], axis=1))
    assert relerr(hs.ldiv_block_t(hs.transpose(F1), B), hs.ldiv_block_t(hs.transpose(F0), B)) <= 1e-11
    assert relerr(hs.selinv_diag(F1), hs.selinv_diag(F0)) <= 1e-11
    F1.free()
    F0.free()


# ---- c. envelopes -------------------------------------------------------------------------------------------------------------------------------

def test_sym_composes_with_envelopes(hs):
    """Poisson 20^3 with the option on: leaf and branch fronts inside their block envelopes (the default) against the same with the envelope
    off (hsk_envelope_enable).  The strips go through Sched::gemm, which clips each of them; the results agree to 1e-12."""
    L = hs._lib.lib()
    P = problem((20, 20, 20), "poisson")
    Fs = []
    prev = L.hsk_envelope_enable(1)
    try:
        for on in (1, 0):
            L.hsk_envelope_enable(on)
            Fs.append(hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0, keep_schur=True, symmetric=True))
    finally:
        L.hsk_envelope_enable(prev)
    F1, F0 = Fs
    assert hs.sym_info(F1)["fronts_general"] == 0 and hs.sym_info(F0)["fronts_general"] == 0
    assert F1.stats()["gemm_flops"] < F0.stats()["gemm_flops"]  # the envelope did clip
    _blocks_agree(F1, F0, 1e-12)
    assert relerr(hs.ldiv(F1, P["b"]), hs.ldiv(F0, P["b"])) <= 1e-12
    F1.free()
    F0.free()


# ---- e. a compressed handle -----------------------------------------------------------------------------------------------------------------------

def test_sym_compressed_handle(hs):
    """Poisson 20^3, swlevel 2, tolerance 1e-6: the compressed fronts and the dense fronts assembled from their Schur complements (symmetric
    to the tolerance only) keep the general path, the dense levels below run on their lower triangles; the solve error stays within 2x."""
    P = problem((20, 20, 20), "poisson")
    A, b = P["A"], P["b"]
    xr = spla.splu(A).solve(b)
    errs, infos = [], []
    for sym in (True, False):
        F = hs.factor(A, P["nd"], P["nd_loc"], swlevel=2, atol=1e-6, rtol=1e-6, symmetric=sym)
        errs.append(relerr(hs.ldiv(F, b), xr))
        infos.append(hs.sym_info(F))
        F.free()
    print(f"[sym compressed] solve error on {errs[0]:.3e} off {errs[1]:.3e}; {infos}")
    assert infos[0]["option"] and infos[0]["fronts_lower"] > 0 and infos[0]["fronts_general"] > 0, infos
    assert infos[0]["fronts_lower"] + infos[0]["fronts_general"] == infos[1]["fronts_general"] and infos[1]["fronts_lower"] == 0, infos
    assert errs[0] <= 2.0 * errs[1], errs


# ---- f. refusals and fallbacks ----------------------------------------------------------------------------------------------------------------------

def _entry(msg):
    """(row, column) named by the message of the symmetry check (1-based)."""
    import re

    m = re.search(r"\(row (\d+), column (\d+)\)", msg)
    assert m, msg
    return int(m.group(1)), int(m.group(2))


def test_sym_refuses_a_matrix_that_is_not_symmetric(hs):
    P = problem((16, 16, 16), "poisson")
    A = sp.csc_matrix(P["A"], copy=True)
    A.sort_indices()
    c = 1234
    e = A.indptr[c] + 1 if A.indices[A.indptr[c]] != c else A.indptr[c]  # an off-diagonal entry of column c ...
    if A.indices[e] == c:
        e += 1
    r = int(A.indices[e])
    A.data[e] = np.nextafter(A.data[e], 0.0)  # ... changed by one ulp on one side of the diagonal
    with pytest.raises(ValueError) as ei:
        hs.factor(A, P["nd"], P["nd_loc"], swlevel=0, symmetric=True)
    assert "symmetric" in str(ei.value)
    assert _entry(str(ei.value)) in ((r + 1, c + 1), (c + 1, r + 1)), (str(ei.value), r, c)
    # an entry without a partner in the pattern: (r, c) is dropped, (c, r) stays
    coo = sp.coo_matrix(P["A"])
    keep = ~((coo.row == r) & (coo.col == c))
    B = sp.csc_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=coo.shape)
    assert B.nnz == P["A"].nnz - 1
    with pytest.raises(ValueError) as ei:
        hs.factor(B, P["nd"], P["nd_loc"], swlevel=0, symmetric=True)
    assert _entry(str(ei.value)) == (c + 1, r + 1), (str(ei.value), r, c)
    # without the option both matrices factor
    hs.factor(A, P["nd"], P["nd_loc"], swlevel=0).free()


def test_sym_refuses_convdiff(hs):
    """Pattern symmetric, values not."""
    P = problem((12, 12, 12), "convdiff")
    assert (P["A"] != P["A"].T).nnz > 0
    with pytest.raises(ValueError) as ei:
        hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0, symmetric=True)
    r, c = _entry(str(ei.value))
    assert P["A"][r - 1, c - 1] != P["A"][c - 1, r - 1]


def test_sym_refuses_several_ranks(hs):
    P = problem((16, 16, 16), "poisson")
    with pytest.raises(hs._lib.UnsupportedError):
        hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=2, symmetric=True)
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=1, symmetric=True)
    hs._lib.lib().hs_free(h)


_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, scipy.sparse.linalg as spla, hsamd
from helpers import prepare
hs = hsamd.load()
P = prepare(hs, (16, 16, 16), kind="poisson", rhs="randn")
F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0, symmetric=True)
x = hs.ldiv(F, P["b"])
xr = spla.splu(P["A"]).solve(P["b"])
i = hs.sym_info(F)
print("RES", np.linalg.norm(x - xr) / np.linalg.norm(xr), int(i["option"]), i["fronts_lower"], i["fronts_general"], F.nnodes)
"""


@pytest.mark.parametrize("var", ["HS_OPTIMISTIC=0", "HS_OPTIMISTIC_FORCE_REDO=1"])
def test_sym_falls_back_without_optimistic_pivoting(var):
    """Tournament pivoting swaps rows across blocks: with HS_OPTIMISTIC=0, and after a level had to be redone (here: forced, the first one),
    every front runs as without the option.  Both switches are read once per process: a fresh child."""
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"))
    k, v = var.split("=")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{k: v}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    res = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("RES")]
    assert len(res) == 1, r.stdout
    err, option, lower, general, nnodes = float(res[0][1]), int(res[0][2]), int(res[0][3]), int(res[0][4]), int(res[0][5])
    assert err <= SOL_TOL and option == 1 and lower == 0 and general >= nnodes, res


def sym_redo_matrix(hs, n=20, nmax=100):
    """redo_matrix of tests/test_lu_paths_gpu.py made symmetric: a 7-point pattern on an n^3 grid, diagonally dominant except among the DOFs
    of the root separator, where the diagonal is tiny and the couplings to z +- 1 are +10 on both sides.  In the root front's order a
    z-neighbour sits 2n rows away, outside the 32-row diagonal block: optimistic pivoting must give up on the root, and only there."""
    N = n ** 3
    g = np.arange(N)
    x, y, z = g % n, (g // n) % n, g // (n * n)
    sep = (x == n // 2 - 1) | (x == n // 2)
    rows, cols, vals = [g], [g], [np.where(sep, 1e-2, 6.5)]
    for d, ok in ((1, x < n - 1), (n, y < n - 1), (n * n, z < n - 1)):
        i = g[ok]
        j = i + d
        both = sep[i] & sep[j] & (d == n * n)
        v = np.where(both, 10.0, -1.0)
        rows += [i, j]
        cols += [j, i]
        vals += [v, v]
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    return A, hs.problems.grid_nested_dissection((n, n, n), nmax)


def test_sym_level_that_redoes_itself(hs, capfd):
    """A symmetric matrix whose root needs a pivot from outside its diagonal blocks: the levels below ran on their lower triangles, the root
    level is redone with the tournament as without the option, and the solution holds."""
    A0, nd = sym_redo_matrix(hs)
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    nd = hs.permuted(nd, hs.invperm(perm))
    A = sp.csc_matrix(A0[perm - 1][:, perm - 1])
    assert (A != A.T).nnz == 0
    b = np.random.default_rng(3).standard_normal(A.shape[0])
    F = hs.factor(A, nd, nd_loc, swlevel=0, symmetric=True, verbose=True)
    err = capfd.readouterr().err
    assert err.count("redoing the level with tournament pivoting") == 1, err[-2000:]
    i = hs.sym_info(F)
    assert i["fronts_lower"] > 0 and i["fronts_general"] == 1, i  # the root alone
    xr = spla.splu(A).solve(b)
    assert relerr(hs.ldiv(F, b), xr) <= SOL_TOL
    F.free()
