"""Branch fronts eliminated inside their block envelope (csrc/hs_envelope.h: hs_branch_envelope) against the same process
with the branch tables switched off (hsk_branch_envelope_enable), the leaf envelope on in both: the clipped K loops add the same numbers in
the same order, so every stored block and the solution must be EQUAL, not close.  Also the flop accounting (device count == host count),
the exact zeros of L[bnd2, int1] and U[int1, bnd2], the forced redo of a level, and one synthetic batch with caller-made tables on the
look-ahead schedule (hsk_front_batch_env_d)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import prepare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOL_TOL = 1e-10  # tests/test_factor_gpu.py


class branch_envelope:
    """with branch_envelope(hs, on): ... -- leaf envelope on, branch tables on / off; the previous settings come back afterwards"""

    def __init__(self, hs, on):
        self.L, self.on = hs._lib.lib(), on

    def __enter__(self):
        self.prev_leaf = self.L.hsk_envelope_enable(1)
        self.prev = self.L.hsk_branch_envelope_enable(1 if self.on else 0)

    def __exit__(self, *a):
        self.L.hsk_branch_envelope_enable(self.prev)
        self.L.hsk_envelope_enable(self.prev_leaf)


def _factor(hs, P, on, count=False, **kw):
    L = hs._lib.lib()
    with branch_envelope(hs, on):
        if not count:
            return hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0, **kw), None
        assert L.hsk_op_flops_mode(1) == 0
        try:
            F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0, **kw)
            out = C.c_double()
            assert L.hsk_op_flops(C.byref(out)) == 0
        finally:
            L.hsk_op_flops_mode(0)
    return F, out.value


def _assert_same_factors(F1, F0):
    assert F1.nnodes == F0.nnodes
    for k in range(F1.nnodes):
        b1, b0 = F1.node_blocks(k, with_schur=True), F0.node_blocks(k, with_schur=True)
        for name in ("LU", "Lbi", "Uib", "S", "rperm"):
            assert np.array_equal(b1[name], b0[name]), (k, name, F1.node_info(k))


def _walk(nd):
    out, stack = [], [nd]
    while stack:
        x = stack.pop()
        out.append(x)
        stack += [c for c in (x.left, x.right) if c is not None]
    return out


def _odd_cube(hs):
    """A 23 x 24 x 25 Poisson box with one DOF of a level-2 separator taken out of the matrix and of the tree (still a nested dissection: a
    vertex less separates no worse): that branch front has an odd ni, so its Schur update has its A at an odd row (shifted edge route)."""
    A, b, nd = hs.problems.make_problem((23, 24, 25), kind="poisson", nmax=1024, rhs="randn")
    g = int(np.asarray(nd.left.int)[0])  # 1-based
    keep = np.r_[0 : g - 1, g : A.shape[0]]
    A = sp.csc_matrix(A)[keep][:, keep]
    for x in _walk(nd):
        for name in ("int", "bnd"):
            v = np.asarray(getattr(x, name), dtype=np.int64)
            v = v[v != g]
            setattr(x, name, np.where(v > g, v - 1, v))
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    Ap = sp.csc_matrix(A[perm - 1][:, perm - 1])
    nd = hs.permuted(nd, hs.invperm(perm))
    odd = [len(x.int) for x in _walk(nd) if x.left is not None and len(x.int) % 2]
    assert odd, "no branch front with an odd ni"
    return dict(A=Ap, nd=nd, nd_loc=nd_loc, b=b[keep][perm - 1])


def _problem(hs, name):
    return _odd_cube(hs) if name == "odd_cube" else prepare(hs, name, rhs="randn")


def _splits(hs, P):
    """(post-order node id, ni, nb, ni1, nb1) of the branch fronts (post-order = the library's node numbering)"""
    out = []
    for k, x in enumerate(hs.postorder_nodes(P["nd"])):
        if x.left is None or x.right is None:
            continue
        lb = np.asarray(x.left.bnd)
        out.append((k, len(x.int), len(x.bnd), int(np.isin(x.int, lb).sum()), int(np.isin(x.bnd, lb).sum())))
    return out


@pytest.mark.parametrize("name", ["poisson3d_32", "odd_cube", "helmholtz3d_32"])
def test_branch_on_equals_off_bitwise(hs, name):
    """poisson3d_32: the root (ni = 2048) takes the look-ahead schedule, level 2 (960) the recursive one.  Also: fewer flops with the tables,
    and L[bnd2, int1] = U[int1, bnd2] = 0 exactly."""
    P = _problem(hs, name)
    L = hs._lib.lib()
    la0 = L.hsk_lookahead_runs(0)
    L.hsk_gemm_lds_launches(1)
    L.hsk_gemm_lds_edge_launches(1)
    F1, _ = _factor(hs, P, True, keep_schur=True)
    la1, lds1, edge1 = L.hsk_lookahead_runs(0), L.hsk_gemm_lds_launches(1), L.hsk_gemm_lds_edge_launches(1)
    F0, _ = _factor(hs, P, False, keep_schur=True)
    lds0 = L.hsk_gemm_lds_launches(1)
    if name == "poisson3d_32":
        # the root looked ahead; updates that clip ran the enveloped twin of the edge tile, so fewer went to the dense direct-to-LDS kernel
        assert la1 - la0 == 1 and edge1 > 0 and 0 < lds1 < lds0, (la1 - la0, lds1, edge1, lds0)
    if name == "odd_cube":  # the Schur update of the front with an odd ni has its A at an odd row: the edge route, enveloped or not
        assert edge1 > 0 and L.hsk_gemm_lds_edge_launches(0) > 0, (edge1, lds1, lds0)
    _assert_same_factors(F1, F0)
    x1, x0 = hs.ldiv(F1, P["b"]), hs.ldiv(F0, P["b"])
    assert np.array_equal(x1, x0)
    assert np.all(np.isfinite(x1))
    s1, s0 = F1.stats(), F0.stats()
    print(f"[branch envelope] {name}: gemm_flops on {s1['gemm_flops']:.6e} off {s0['gemm_flops']:.6e} ratio {s1['gemm_flops'] / s0['gemm_flops']:.4f}")
    assert s1["gemm_flops"] < s0["gemm_flops"]
    checked = 0
    for k, ni, nb, ni1, nb1 in _splits(hs, P):
        if nb - nb1 == 0 or ni1 == 0:
            continue
        assert F1.node_info(k)[:2] == (ni, nb), (k, F1.node_info(k))
        blk = F1.node_blocks(k)
        Lbi, Uib = np.asarray(blk["Lbi"]), np.asarray(blk["Uib"])
        assert Lbi.shape == (nb, ni) and Uib.shape == (ni, nb)
        assert np.count_nonzero(Lbi[nb1:, :ni1]) == 0 and np.count_nonzero(Uib[:ni1, nb1:]) == 0, (k, ni, nb, ni1, nb1)
        checked += 1
    assert checked >= 3
    F1.free()
    F0.free()


@pytest.mark.parametrize("name", ["poisson3d_32", "helmholtz3d_32"])
def test_accounting(hs, name):
    """The kernels' own count of the K-steps they ran == the host's gemm_flops, exactly, with the branch tables (real tile and the complex
    tile, 64 columns wide; look-ahead launches at the root of poisson3d_32)."""
    P = prepare(hs, name, rhs="randn")
    F1, dev1 = _factor(hs, P, True, count=True)
    F0, dev0 = _factor(hs, P, False, count=True)
    s1, s0 = F1.stats(), F0.stats()
    print(f"[branch envelope] {name}: gemm_flops on {s1['gemm_flops']:.17g} off {s0['gemm_flops']:.17g} device on {dev1:.17g} off {dev0:.17g}")
    assert dev1 == s1["gemm_flops"] and dev0 == s0["gemm_flops"]
    assert s1["gemm_flops"] < s0["gemm_flops"]
    F1.free()
    F0.free()


_FORCE_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, scipy.sparse.linalg as spla, hsamd
from helpers import prepare
hs = hsamd.load()
L = hs._lib.lib()
P = prepare(hs, "poisson3d_32", rhs="randn")
L.hsk_envelope_enable(1)
xs, blocks = [], []
for on in (1, 0):
    L.hsk_branch_envelope_enable(on)
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0, keep_schur=True)
    xs.append(hs.ldiv(F, P["b"]))
    blocks.append([F.node_blocks(k, with_schur=True) for k in range(F.nnodes)])
    F.free()
assert np.array_equal(xs[0], xs[1])
for k, (b1, b0) in enumerate(zip(*blocks)):
    for name in ("LU", "Lbi", "Uib", "S", "rperm"):
        assert np.array_equal(b1[name], b0[name]), (k, name)
xr = spla.splu(P["A"]).solve(P["b"])
err = np.linalg.norm(xs[0] - xr) / np.linalg.norm(xr)
print("err", err)
assert err < 1e-10
print("FORCE OK")
"""


def test_forced_redo_with_the_branch_tables_on():
    """HS_OPTIMISTIC_FORCE_REDO (read once per process): the first level is eliminated inside the envelope, thrown away and redone densely,
    and every level after it runs the tournament (dense) -- the same bits either way, and the SuperLU solution to SOL_TOL."""
    code = _FORCE_CHILD % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, HS_OPTIMISTIC_FORCE_REDO="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FORCE OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


# ---- a synthetic batch on the look-ahead schedule, with tables that do not come from hs_branch_envelope ---------------------------------------

ALIGNED = 4  # bit 2 of the hook's mode: Sched::aligned16, as hs_numeric runs a level


def _synthetic_front(ni, nb, seed):
    """Two dense diagonal blocks (child 1 = positions < ni1 and ni <= p < ni + nb1) plus a diagonal coupling int1 <-> int2, bnd1 <-> bnd2;
    strongly diagonally dominant, so no multiplier comes near the growth bound.  Returns F and its tables from the NumPy mirror."""
    from test_leaf_envelope_host import envelope_numpy

    rng = np.random.default_rng(seed)
    m, ni1, nb1 = ni + nb, ni // 2 + 1, nb // 2
    p = np.arange(m)
    side = np.where(p < ni, p >= ni1, p - ni >= nb1)
    F = np.where(side[:, None] == side[None, :], rng.standard_normal((m, m)), 0.0)
    for lo, n1, n in ((0, ni1, ni), (ni, nb1, nb)):
        k = np.arange(min(n1, n - n1))
        F[lo + k, lo + n1 + k] = rng.standard_normal(k.size)
        F[lo + n1 + k, lo + k] = rng.standard_normal(k.size)
    F[p, p] += 4.0 * m
    fL, fU = envelope_numpy(sp.csr_matrix(F != 0), p, ni)
    return F, np.concatenate([fL, fU]).astype(np.int32)


def _batch_env(hs, Fs, nis, mode, env):
    L = hs._lib.lib()
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    ni = np.asarray(nis, dtype=np.int64)
    ms = np.asarray([F.shape[0] for F in Fs], dtype=np.int64)
    nb = ms - ni
    Fp = np.concatenate([np.asarray(F, dtype=np.float64).ravel(order="F") for F in Fs])
    out = dict(LF=np.zeros(int((ms * ni).sum()) + 1), UR=np.zeros(int((ni * nb).sum()) + 1), SB=np.zeros(int((nb * nb).sum()) + 1))
    rp = np.zeros(int(ni.sum()) + 1, dtype=np.int64)
    info, growth = np.zeros(len(Fs), dtype=np.int64), np.zeros(len(Fs), dtype=np.int64)
    e = None if env is None else np.ascontiguousarray(np.concatenate(env), dtype=np.int32)
    hs._lib.check(L.hsk_front_batch_env_d(len(Fs), ni.ctypes.data_as(pi), nb.ctypes.data_as(pi), mode, Fp.ctypes.data_as(pd),
                                          None if e is None else e.ctypes.data_as(C.POINTER(C.c_int32)), out["LF"].ctypes.data_as(pd),
                                          out["UR"].ctypes.data_as(pd), out["SB"].ctypes.data_as(pd), rp.ctypes.data_as(pi),
                                          info.ctypes.data_as(pi), growth.ctypes.data_as(pi)))
    assert not info.any() and not growth.any(), (info, growth)
    out["rperm"] = rp
    return out


@pytest.mark.parametrize("shapes", [[(1536, 304)], [(2049, 300), (1600, 0)]])
def test_synthetic_batch_on_the_lookahead_schedule(hs, shapes):
    """Tables on against off (null), bitwise, in the production mode (optimistic, descriptors, aligned16); the batch looks ahead both times,
    and with the tables the clipped updates run the enveloped kernels."""
    L = hs._lib.lib()
    fronts = [_synthetic_front(ni, nb, 100 + ni) for ni, nb in shapes]
    Fs, envs, nis = [f for f, _ in fronts], [e for _, e in fronts], [ni for ni, _ in shapes]
    res, counts = [], []
    for env in (envs, None):
        la = L.hsk_lookahead_runs(0)
        L.hsk_gemm_lds_launches(1), L.hsk_gemm_lds_edge_launches(1)
        res.append(_batch_env(hs, Fs, nis, 2 | ALIGNED, env))
        counts.append((L.hsk_lookahead_runs(0) - la, L.hsk_gemm_lds_launches(1), L.hsk_gemm_lds_edge_launches(1)))
    for name in ("LF", "UR", "SB", "rperm"):
        assert np.array_equal(res[0][name], res[1][name]), name
    (la1, lds1, edge1), (la0, lds0, edge0) = counts
    print(f"[branch envelope] synthetic {shapes}: tables: lds {lds1} edge/enveloped {edge1}; dense: lds {lds0} edge {edge0}")
    assert la1 == 1 and la0 == 1
    # an enveloped plain update runs gemm_op_env_lds_kernel, counted with the edge kernel; every launch that clips left the dense LDS kernel
    assert edge1 > edge0 and lds1 < lds0 and lds1 + edge1 == lds0 + edge0, counts
    if shapes == [(1536, 304)]:
        assert edge0 == 0  # every K a multiple of 16, every row offset even: without tables nothing takes the edge route
