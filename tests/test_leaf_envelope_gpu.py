"""Leaf fronts eliminated inside their block envelope against the same process with the envelope switched off
(hsk_envelope_enable): the clipped K loops add the same numbers in the same order, so every stored block and the solution must be EQUAL,
not close -- np.array_equal, which ignores only the sign of zero.  Also: levels that redo themselves with tournament pivoting (the envelope
is then not used), a leaf whose interior order is scrambled, the growth flag of a leaf, and the flop accounting (device count == host count).

The flops expected with the envelope off are the counts of the commit before the envelope existed (the dense formula of Sched::gemm)."""
import os
import subprocess
import sys

import ctypes as C
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from helpers import prepare, relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOL_TOL = 1e-10  # tests/test_factor_gpu.py

# hs_stats.gemm_flops of the parent commit (dense rectangles), recorded on an MI355X
PARENT_GEMM_FLOPS = {"poisson3d_64": 4706642719952.0, "helmholtz3d_32": 111500879168.0}


class envelope:
    """with envelope(hs, on): ... -- the previous setting comes back afterwards"""

    def __init__(self, hs, on):
        self.L, self.on = hs._lib.lib(), on

    def __enter__(self):
        self.prev = self.L.hsk_envelope_enable(1 if self.on else 0)

    def __exit__(self, *a):
        self.L.hsk_envelope_enable(self.prev)


def _factor(hs, P, on, count=False, **kw):
    """Factor with the envelope on / off.  count: with the device-side flop count on (which sends every plain update, of dense fronts too,
    through gemm_op_env_kernel -- so the bitwise comparisons below factor WITHOUT it, to meet the real dense kernels)."""
    L = hs._lib.lib()
    with envelope(hs, on):
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


@pytest.mark.parametrize("name", ["poisson3d_64", "helmholtz3d_64", "poisson3d_32"])
def test_envelope_on_equals_off_bitwise(hs, name):
    P = prepare(hs, name, rhs="randn")
    F1, _ = _factor(hs, P, True, keep_schur=True)
    F0, _ = _factor(hs, P, False, keep_schur=True)
    _assert_same_factors(F1, F0)
    x1, x0 = hs.ldiv(F1, P["b"]), hs.ldiv(F0, P["b"])  # (multiplies by the stored 256-inverses)
    assert np.array_equal(x1, x0)
    assert np.all(np.isfinite(x1))
    s1, s0 = F1.stats(), F0.stats()
    print(f"[envelope] {name}: gemm_flops on {s1['gemm_flops']:.6e} off {s0['gemm_flops']:.6e} ratio {s1['gemm_flops'] / s0['gemm_flops']:.4f}; "
          f"gemm_bytes on {s1['gemm_bytes']:.6e} off {s0['gemm_bytes']:.6e}")
    assert s1["gemm_flops"] < s0["gemm_flops"] and s1["gemm_bytes"] < s0["gemm_bytes"]
    if name in PARENT_GEMM_FLOPS:
        assert s0["gemm_flops"] == PARENT_GEMM_FLOPS[name]
    F1.free()
    F0.free()


@pytest.mark.parametrize("name", ["poisson3d_64", "helmholtz3d_32"])
def test_accounting(hs, name):
    """The kernel's own count of the K-steps it ran == the host's gemm_flops, exactly, envelope on and off (real tile, and the complex tile, 64
    columns wide); off == the parent commit's figure; on it is smaller."""
    P = prepare(hs, name, rhs="randn")
    F1, dev1 = _factor(hs, P, True, count=True)
    F0, dev0 = _factor(hs, P, False, count=True)
    s1, s0 = F1.stats(), F0.stats()
    print(f"[envelope] {name}: gemm_flops on {s1['gemm_flops']:.17g} off {s0['gemm_flops']:.17g} device on {dev1:.17g} off {dev0:.17g}")
    assert dev1 == s1["gemm_flops"] and dev0 == s0["gemm_flops"]
    assert s0["gemm_flops"] == PARENT_GEMM_FLOPS[name]
    assert s1["gemm_flops"] < s0["gemm_flops"]
    assert np.array_equal(hs.ldiv(F1, P["b"]), hs.ldiv(F0, P["b"]))
    F1.free()
    F0.free()


def _redo_problem(hs):
    import test_lu_paths_gpu as T

    A0, nd = T.redo_matrix(hs)
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    nd = hs.permuted(nd, hs.invperm(perm))
    A = sp.csc_matrix(A0[perm - 1][:, perm - 1])
    return dict(A=A, nd=nd, nd_loc=nd_loc)


def test_level_that_redoes_itself(hs, capfd):
    """The 20^3 problem of tests/test_lu_paths_gpu.py: the root gives up on optimistic pivoting and is redone with the tournament (dense);
    the leaves below it were eliminated inside their envelopes.  Same bits as with the envelope off."""
    P = _redo_problem(hs)
    b = np.random.default_rng(3).standard_normal(P["A"].shape[0])
    xs = []
    for on in (True, False):
        F, _ = _factor(hs, P, on, verbose=True)
        err = capfd.readouterr().err
        assert err.count("redoing the level with tournament pivoting") == 1, err[-2000:]
        xs.append(hs.ldiv(F, b))
        F.free()
    assert np.array_equal(xs[0], xs[1])
    assert relerr(xs[0], spla.splu(P["A"]).solve(b)) < SOL_TOL


_FORCE_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, scipy.sparse.linalg as spla, hsamd
from helpers import prepare
hs = hsamd.load()
L = hs._lib.lib()
P = prepare(hs, "poisson3d_32", rhs="randn")
xs = []
for on in (1, 0):
    L.hsk_envelope_enable(on)
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
    xs.append(hs.ldiv(F, P["b"]))
    F.free()
assert np.array_equal(xs[0], xs[1])
xr = spla.splu(P["A"]).solve(P["b"])
assert np.linalg.norm(xs[0] - xr) / np.linalg.norm(xr) < 1e-10
print("FORCE OK")
"""


def test_forced_redo_with_the_envelope_on():
    """HS_OPTIMISTIC_FORCE_REDO (read once per process): the first level is eliminated inside the envelope, thrown away and redone densely."""
    code = _FORCE_CHILD % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, HS_OPTIMISTIC_FORCE_REDO="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FORCE OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


def _leaves(nd):
    out, stack = [], [nd]
    while stack:
        x = stack.pop()
        if x.left is None and x.right is None:
            out.append(x)
        else:
            stack += [c for c in (x.left, x.right) if c is not None]
    return out


def test_scrambled_leaf_order(hs):
    """A leaf whose interior DOFs come in random order has a nearly full envelope -- a valid answer: the result is still right."""
    from test_leaf_envelope_host import envelope_library

    A, b, nd = hs.problems.make_problem("poisson3d_32", rhs="randn")
    rng = np.random.default_rng(11)
    leaves = _leaves(nd)
    for x in leaves[:3]:
        x.int = np.asarray(x.int)[rng.permutation(len(x.int))]
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    Ap = sp.csc_matrix(A[perm - 1][:, perm - 1])
    nd = hs.permuted(nd, hs.invperm(perm))
    bp = b[perm - 1]
    fulls = []
    for x in _leaves(nd):
        it, bd = np.asarray(x.int) - 1, np.asarray(x.bnd) - 1
        fL, _ = envelope_library(hs, Ap, np.concatenate([it, bd]), len(it))
        nbi = (len(it) + 31) // 32
        fulls.append(np.mean(fL[:nbi] == 0))
    assert sum(f > 0.8 for f in fulls) >= 3, sorted(fulls)[-4:]  # the scrambled leaves: almost every row block starts at column 0
    P = dict(A=Ap, nd=nd, nd_loc=nd_loc)
    F1, _ = _factor(hs, P, True)
    F0, _ = _factor(hs, P, False)
    x1 = hs.ldiv(F1, bp)
    assert relerr(x1, spla.splu(Ap).solve(bp)) < SOL_TOL
    assert np.array_equal(x1, hs.ldiv(F0, bp))
    F1.free()
    F0.free()


def test_growth_flag_of_a_leaf(hs, capfd):
    """A large entry planted in a leaf, in a later 32-row block than its column: the multiplier exceeds the bound whichever row of the
    column's diagonal block becomes the pivot, so the leaf level must raise its flag and redo itself -- with the envelope on as with it off."""
    P = prepare(hs, "poisson3d_32", rhs="randn")
    A = sp.csc_matrix(P["A"]).copy()
    x = _leaves(P["nd"])[0]
    it = np.asarray(x.int) - 1
    ni = len(it)
    sub = sp.coo_matrix(A[it][:, it])
    far = sub.row // 256 > sub.col // 256 if np.any(sub.row // 256 > sub.col // 256) else sub.row // 32 > sub.col // 32
    assert far.any()
    k = int(np.flatnonzero(far)[0])
    A[it[sub.row[k]], it[sub.col[k]]] = 1e3  # (a structural entry: the pattern does not change)
    A = sp.csc_matrix(A)
    assert A.nnz == P["A"].nnz
    Q = dict(A=A, nd=P["nd"], nd_loc=P["nd_loc"])
    xs = []
    for on in (True, False):
        F, _ = _factor(hs, Q, on, verbose=True)
        err = capfd.readouterr().err
        assert "redoing the level with tournament pivoting" in err, (on, err[-2000:])
        xs.append(hs.ldiv(F, P["b"]))
        F.free()
    assert np.array_equal(xs[0], xs[1])
    assert relerr(xs[0], spla.splu(A).solve(P["b"])) < SOL_TOL
