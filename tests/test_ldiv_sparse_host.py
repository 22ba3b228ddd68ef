"""Sparse right-hand sides and selected rows on the CPU: the NumPy statement of the pruned schedule (tests/ldiv_sparse_mirror.py) over the
oracle's exact factorization against the full block schedule (bit for bit) and SuperLU, the plan of the library (hs_ldiv_sparse_plan on a
host-side plan) against a closure computed here from the elimination tree, and the new entry points of the C ABI.  The device
implementation (csrc/hs_solve_sparse.hip) is checked in tests/test_ldiv_sparse_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import ldiv_block_mirror as M
import ldiv_block_t_mirror as MT
import ldiv_sparse_mirror as MS
from helpers import prepare, relerr
from oracle import hs_oracle as O
from test_ldiv_block_host import PROBLEMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hs_ldiv_sparse_d", "hs_ldiv_sparse_z", "hs_ldiv_sparse_dev_d", "hs_ldiv_sparse_dev_z", "hs_ldiv_sparse_plan", "hs_ldiv_sparse_info")


def sources(n, k, where, leaf_rows, cplx, seed, empty=None):
    """n x k CSC block of point sources, one to three stored rows per column: inside one leaf or anywhere; column `empty` stays empty."""
    rng = np.random.default_rng(seed)
    pool = np.asarray(leaf_rows) if where == "leaf" else np.arange(n)
    r, c, v = [], [], []
    for j in range(k):
        if j == empty:
            continue
        for i in rng.choice(pool, size=int(rng.integers(1, 4)), replace=False):
            r.append(int(i))
            c.append(j)
            v.append(rng.standard_normal() + (1j * rng.standard_normal() if cplx else 0.0))
    return sp.csc_matrix((np.array(v, dtype=np.complex128 if cplx else np.float64), (r, c)), shape=(n, k))


@pytest.mark.parametrize("lowrank", [False, True], ids=["dense", "lowrank"])
@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_mirror_of_the_pruned_schedule_is_the_full_schedule_at_the_wanted_rows(hs, kind, shape, nmax, lowrank):
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    A = P["A"]
    n = A.shape[0]
    cplx = np.iscomplexobj(A.data)
    F = O.factor(A, P["ond"], P["ond_loc"], swlevel=0)
    levels = MS.fronts_with_parents(F, lowrank=lowrank)
    assert all(isinstance(f, M.Front) for fr in levels for f in fr)
    nfronts = sum(len(fr) for fr in levels)
    leaf = levels[-1][0]
    lu = spla.splu(A)
    rng = np.random.default_rng(11)
    few = np.sort(rng.choice(leaf.int, size=5, replace=False))
    far = levels[-1][-1].int[:3]  # receivers in another leaf than the sources: fronts only the backward sweep visits (y = 0 there)
    assert nfronts == 3 or MS.closure(MS.owners(levels, n), far) - MS.closure(MS.owners(levels, n), few)
    rowsets = {"few": few, "far": far, "all": None, "repeats": np.array([few[3], few[0], few[3], n - 1, few[0]])}
    for k in (1, 17, 40):
        for where, empty in (("leaf", None), ("anywhere", None), ("leaf", k // 2)):
            B = sources(n, k, where, leaf.int, cplx, 100 * k + (empty or 0), empty)
            Bd = B.toarray()
            # the full block schedule on the same columns.  A column of a NumPy (BLAS) product is rounded differently at another position of
            # the block, so the full schedule sees the columns in the processing order (the device products are position-independent:
            # test_ldiv_block_gpu.py, and test_ldiv_sparse_gpu.py compares in the caller's order); sources of one leaf keep the caller's order
            order = MS.column_order(MS.owners(levels, n), B)
            full = np.empty((n, k), dtype=np.result_type(Bd.dtype, levels[0][0].L11.dtype))
            full[:, order] = M.ldiv_block(levels, Bd[:, order], kc=32)
            if where == "leaf" and empty is None:
                assert np.array_equal(order, np.arange(k)) and np.array_equal(full, M.ldiv_block(levels, Bd, kc=32))
            ref = lu.solve(Bd)
            for name, rows in rowsets.items():
                X, st = MS.ldiv_sparse(levels, B, rows, kc=32)
                assert np.array_equal(st["order"], order)
                sel = slice(None) if rows is None else rows
                assert np.array_equal(X, full[sel]), (k, where, empty, name)
                e = relerr(X, ref[sel])
                assert e < 1e-11, (k, where, empty, name, e)
                if empty is not None:
                    assert np.all(X[:, empty] == 0)
                if where == "leaf":  # the pruned run visits strictly fewer fronts than the tree has
                    assert all(v < nfronts for v in st["forward"])
                    if name != "all":
                        assert all(v < nfronts for v in st["backward"])
                    print(f"{kind} {shape} lowrank={lowrank} k={k} rows={name}: forward {st['forward']} backward {st['backward']} of {nfronts} fronts, vs splu {e:.2e}")
    # trans acts on F, not on B
    B = sources(n, 17, "leaf", leaf.int, cplx, 7)
    for trans in ("T", "H"):
        X, st = MS.ldiv_sparse(levels, B, few, trans=trans, kc=32)
        assert np.array_equal(st["order"], np.arange(17))
        assert np.array_equal(X, MT.ldiv_block_t(levels, B.toarray(), trans=trans, kc=32)[few])
        assert relerr(X, lu.solve(B.toarray(), trans=trans)[few]) < 1e-11


def tree_closure(nd, n):
    """Post-order ids, the owner of every row and the parent of every node, from the elimination tree alone (1-based int sets)."""
    owner, parent = np.full(n, -1), []

    def walk(x):
        kids = [walk(c) for c in (x.left, x.right) if c is not None]
        me = len(parent)
        parent.append(-1)
        for c in kids:
            parent[c] = me
        owner[np.asarray(x.int, dtype=np.int64) - 1] = me
        return me

    walk(nd)
    return owner, np.array(parent)


def expected_plan(owner, parent, B, rows, kc):
    nn = len(parent)

    def up(idx):
        m = np.zeros(nn, dtype=bool)
        for i in idx:
            f = owner[i]
            while f >= 0 and not m[f]:
                m[f] = True
                f = parent[f]
        return m

    B = B.tocsc()
    B.sort_indices()
    k = B.shape[1]
    key = [owner[B.indices[B.indptr[j]]] if B.indptr[j + 1] > B.indptr[j] else nn + 1 for j in range(k)]
    order = np.array(sorted(range(k), key=lambda j: key[j]), dtype=np.int64)
    bwd = np.ones(nn, dtype=bool) if rows is None else up(rows)
    active = np.zeros((-(-k // kc), nn), dtype=np.uint8)
    for c in range(active.shape[0]):
        stored = np.concatenate([B.indices[B.indptr[j] : B.indptr[j + 1]] for j in order[c * kc : (c + 1) * kc]])
        if len(stored):
            active[c] = up(stored) * 1 + bwd * 2
    return order, active


@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_plan_equals_a_closure_computed_from_the_elimination_tree(hs, kind, shape, nmax):
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    A = P["A"]
    n = A.shape[0]
    owner, parent = tree_closure(P["nd"], n)
    assert owner.min() >= 0  # the root keeps no boundary: every row is interior to one node
    leaves = [i for i in range(len(parent)) if i not in set(parent)]
    leaf_rows = np.flatnonzero(owner == leaves[len(leaves) // 2])
    kc = hs.solver._block_cols()
    h = hs.dist.plan_only(A, P["nd"], P["nd_loc"])
    try:
        rng = np.random.default_rng(3)
        few = rng.choice(n, size=6, replace=False)
        cases = [
            (sources(n, 2 * kc + 6, "anywhere", leaf_rows, False, 1, empty=5), None),  # three chunks, every backward bit set
            (sources(n, 2 * kc + 6, "leaf", leaf_rows, False, 2), few),
            (sources(n, 7, "anywhere", leaf_rows, False, 3, empty=0), np.array([few[0], few[0]])),
            (sp.hstack([sources(n, 10, "leaf", leaf_rows, False, 4), sp.csc_matrix((n, kc + 3))]).tocsc(), few),  # the second chunk is empty
        ]
        for B, rows in cases:
            got = hs.ldiv_sparse_plan(h, B, rows)
            order, active = expected_plan(owner, parent, B, rows, kc)
            assert got["nchunks"] == active.shape[0]
            assert np.array_equal(got["order"], order)
            assert got["active"].shape == active.shape and np.array_equal(got["active"], active)
            nonempty = active.any(axis=1)
            if rows is None:
                assert np.all((got["active"][nonempty] & 2) == 2)
            assert np.all(got["active"][~nonempty] == 0)
        assert np.array_equal(hs.ldiv_sparse_plan(h, cases[0][0], None)["active"][:, -1], [3, 3, 3])  # the root is on every path
    finally:
        hs._lib.lib().hs_free(h)


def test_new_entry_points_are_declared_exported_and_bound(hs):
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    lib = hs._lib.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    for f in (hs.ldiv_sparse, hs.inv_entries, hs.ldiv_sparse_info, hs.ldiv_sparse_plan):
        assert callable(f)
    # argument errors need no device: a null handle is refused by every entry point, whatever trans is
    E = hs._lib
    cp = np.array([1, 2], dtype=np.int64)
    rv = np.array([1], dtype=np.int64)
    val = np.ones(2)
    X = np.full(2, 42.0)
    p64, pf = E.p_i64, E.p_f64
    for trans in (0, 1, 2):
        for fn in (lib.hs_ldiv_sparse_d, lib.hs_ldiv_sparse_z):
            assert fn(None, trans, 2, 1, cp.ctypes.data_as(p64), rv.ctypes.data_as(p64), val.ctypes.data_as(pf), None, 0, X.ctypes.data_as(pf), 2) == E.HS_ERR_ARGUMENT
        for fn in (lib.hs_ldiv_sparse_dev_d, lib.hs_ldiv_sparse_dev_z):
            assert fn(None, trans, 2, 1, cp.ctypes.data_as(p64), rv.ctypes.data_as(p64), None, None, 0, None, 2, None) == E.HS_ERR_ARGUMENT
        assert lib.hs_ldiv_sparse_plan(None, trans, 2, 1, cp.ctypes.data_as(p64), rv.ctypes.data_as(p64), None, 0, None, None, None) == E.HS_ERR_ARGUMENT
    assert lib.hs_ldiv_sparse_info(None, (C.c_double * 8)()) == E.HS_ERR_ARGUMENT
    assert np.all(X == 42.0)


def test_plan_refusals_on_host_side_plans(hs):
    E = hs._lib
    P = prepare(hs, (30, 27), kind="convdiff", nmax=450, rhs="randn")
    n = P["A"].shape[0]
    B = sources(n, 3, "anywhere", None, False, 1)
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"])
    try:
        lib = hs._lib.lib()
        cp = np.ascontiguousarray(B.indptr, dtype=np.int64) + 1
        rv = np.ascontiguousarray(B.indices, dtype=np.int64) + 1
        p64 = E.p_i64
        nch = E.i64(0)

        def plan(n_=n, cp_=cp, rv_=rv, rows=None, trans=0):
            pr = None if rows is None else np.asarray(rows, dtype=np.int64).ctypes.data_as(p64)
            return lib.hs_ldiv_sparse_plan(h, trans, n_, 3, cp_.ctypes.data_as(p64), rv_.ctypes.data_as(p64), pr, 0 if rows is None else len(rows), None, C.byref(nch), None)

        assert plan() == E.HS_OK and nch.value == 1
        assert plan(trans=3) == E.HS_ERR_ARGUMENT
        assert plan(n_=n - 1) == E.HS_ERR_DIMENSION
        assert plan(cp_=cp - 1) == E.HS_ERR_ARGUMENT  # 0-based
        bad = cp.copy()
        bad[1] = bad[2] + 1
        assert plan(cp_=bad) == E.HS_ERR_ARGUMENT  # not monotone
        out = rv.copy()
        out[0] = n + 1
        assert plan(rv_=out) == E.HS_ERR_DIMENSION
        two = sp.csc_matrix((np.ones(2), ([4, 9], [0, 0])), shape=(n, 3))
        cp2 = np.ascontiguousarray(two.indptr, dtype=np.int64) + 1
        assert plan(cp_=cp2, rv_=np.array([10, 5], dtype=np.int64)) == E.HS_ERR_ARGUMENT  # rows of a column not strictly increasing
        assert plan(cp_=cp2, rv_=np.array([5, 5], dtype=np.int64)) == E.HS_ERR_ARGUMENT
        assert plan(rows=[0]) == E.HS_ERR_DIMENSION and plan(rows=[n + 1]) == E.HS_ERR_DIMENSION
        assert plan(rows=[n, 1, n]) == E.HS_OK
        with pytest.raises(hs.DimensionMismatch):
            hs.ldiv_sparse_plan(h, B[:-1], None)
        with pytest.raises(TypeError):
            hs.ldiv_sparse_plan(h, B.toarray(), None)
    finally:
        hs._lib.lib().hs_free(h)
    # fronts that keep D as an HSS matrix are refused by the plan call too, as hs_ldiv_block_t_* refuses them
    P3 = prepare(hs, (18, 18, 18), kind="convdiff", nmax=300, rhs="randn")
    h = hs.dist.plan_only(P3["A"], P3["nd"], P3["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    try:
        with pytest.raises(hs.UnsupportedError, match="HSS"):
            hs.ldiv_sparse_plan(h, sources(P3["A"].shape[0], 3, "anywhere", None, False, 1), None)
    finally:
        hs._lib.lib().hs_free(h)
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=2)
    try:
        with pytest.raises(hs.UnsupportedError, match="ranks"):
            hs.ldiv_sparse_plan(h, B, None)
    finally:
        hs._lib.lib().hs_free(h)
