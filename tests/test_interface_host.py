"""Schur-complement mode, the parts that need no GPU: the declared / exported / bound entry points and their null-handle refusals, the
Python argument checks, the tree helper ``graph_nested_dissection(..., interface=...)`` against the oracle's ``F.S``, and
``hs_interface_size`` / ``hs_interface_indices`` on plan-only handles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from interface_cases import dense_schur, interface_ids, interface_problem
from oracle import hs_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASES = ("condense", "solve", "expand")
ENTRY = (["hs_interface_size", "hs_interface_indices", "hs_interface_matrix_d", "hs_interface_matrix_z", "hs_interface_info"]
         + [f"hs_interface_{p}{d}{t}" for p in PHASES for d in ("", "_dev") for t in ("_d", "_z")])
HOOKS = ["hsk_lu_product_d", "hsk_lu_product_z"]
CASES = [("convdiff", (30, 27), 40, 30), ("convdiff_helmholtz", (30, 27), 40, 30), ("convdiff_helmholtz", (12, 12, 12), 100, 147)]


def test_entry_points_are_declared_exported_and_bound(hs):
    assert len(ENTRY) == 17
    lib = hs._lib.lib()
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    ktxt = open(os.path.join(ROOT, "include", "hs_kernels.h")).read()
    for name in ENTRY:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None, name
    for name in HOOKS:
        assert re.search(r"\bint\s+%s\s*\(" % name, ktxt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None, name
    mk = open(os.path.join(ROOT, "hierarchicalsolvers.jl_amd", "csrc", "Makefile")).read()
    assert "kernels_interface.hip" in mk and "hs_interface.hip" in mk
    for name in ("interface_indices", "schur_complement", "condense", "interface_solve", "expand", "interface_info"):
        assert callable(getattr(hs, name))


def test_null_handle_is_an_argument_error_and_writes_nothing(hs):
    L = hs._lib.lib()
    E = hs._lib.HS_ERR_ARGUMENT
    nb = C.c_int64(-5)
    assert L.hs_interface_size(None, C.byref(nb)) == E and nb.value == -5
    idx = np.full(4, -5, dtype=np.int64)
    assert L.hs_interface_indices(None, idx.ctypes.data_as(hs._lib.p_i64)) == E and (idx == -5).all()
    S = np.full((3, 3), 7.0, order="F")
    for fn in (L.hs_interface_matrix_d, L.hs_interface_matrix_z):
        assert fn(None, S.ctypes.data, 3, 0, None) == E and (S == 7.0).all()
    Cb = np.full((4, 2), 7.0, order="F")
    for p in PHASES:
        for t in ("_d", "_z"):
            assert getattr(L, f"hs_interface_{p}{t}")(None, 0, Cb.ctypes.data_as(hs._lib.p_f64), 4, 4, 1) == E
            assert getattr(L, f"hs_interface_{p}_dev{t}")(None, 0, Cb.ctypes.data, 4, 4, 1, None) == E
    assert (Cb == 7.0).all()
    out = np.full(8, 7.0)
    assert L.hs_interface_info(None, out.ctypes.data_as(hs._lib.p_f64)) == E and (out == 7.0).all()
    assert b"null factorization handle" in L.hs_last_error()


def test_hook_refuses_bad_arguments_before_any_device_work(hs):
    L = hs._lib.lib()
    LF = np.ones((4, 3), order="F")
    S = np.full((3, 3), 7.0, order="F")
    fl = C.c_double(-1.0)
    pf = hs._lib.p_f64
    p32 = C.POINTER(C.c_int32)
    good = np.arange(3, dtype=np.int32)
    for rp, ldl, lds in ((np.array([0, 1, 3], dtype=np.int32), 4, 3), (np.array([0, 1, 1], dtype=np.int32), 4, 3), (good, 2, 3), (good, 4, 2)):
        assert L.hsk_lu_product_d(3, LF.ctypes.data_as(pf), ldl, rp.ctypes.data_as(p32), S.ctypes.data_as(pf), lds, C.byref(fl)) == hs._lib.HS_ERR_ARGUMENT
    assert L.hsk_lu_product_z(0, LF.ctypes.data_as(pf), 4, good.ctypes.data_as(p32), S.ctypes.data_as(pf), 3, None) == hs._lib.HS_ERR_ARGUMENT
    assert (S == 7.0).all() and fl.value == -1.0


def test_python_argument_checks_come_first(hs):
    F = hs.FactorNode(None, np.float64, 6, {"nnodes": 0})  # no handle: a library call would be refused there, the Python checks come before it
    for fn in (hs.condense, hs.interface_solve, hs.expand):
        with pytest.raises(TypeError):
            fn(F, np.zeros((6, 2), dtype=np.complex128, order="F"))  # wrong dtype: in place, so no conversion
        with pytest.raises(TypeError):
            fn(F, [[0.0] * 2] * 6)  # not an array
        with pytest.raises(hs.DimensionMismatch):
            fn(F, np.zeros((5, 2), order="F"))
        with pytest.raises(ValueError, match="column-major"):
            fn(F, np.zeros((6, 2), order="C"))
        with pytest.raises(TypeError):
            fn("F", np.zeros((6, 2), order="F"))
    with pytest.raises(ValueError, match="interface ids"):
        hs.problems.graph_nested_dissection(hs.problems.grid_matrix((5, 5), "poisson"), 8, interface=[0, 25])
    with pytest.raises(ValueError, match="distinct"):
        hs.problems.graph_nested_dissection(hs.problems.grid_matrix((5, 5), "poisson"), 8, interface=[3, 3])


def _same_tree(a, b):
    assert np.array_equal(a.int, b.int) and np.array_equal(a.bnd, b.bnd)
    assert (a.left is None) == (b.left is None) and (a.right is None) == (b.right is None)
    if a.left is not None:
        _same_tree(a.left, b.left)
    if a.right is not None:
        _same_tree(a.right, b.right)


@pytest.mark.parametrize("kind,shape,nmax,nb", CASES)
def test_interface_none_is_todays_tree(hs, kind, shape, nmax, nb):
    A = hs.problems.grid_matrix(shape, kind)
    a = hs.problems.graph_nested_dissection(A, nmax)
    _same_tree(a, hs.problems.graph_nested_dissection(A, nmax, interface=None))
    assert len(a.bnd) == 0
    # the rule the function had before the argument existed, restated: bnd(V) = the DOFs of V with a neighbour outside V
    G = ((abs(A) + abs(A).T) > 0).tolil()
    G.setdiag(0)
    G = G.tocsr()
    for x in hs.postorder_nodes(a):
        if x.left is None:
            V = np.sort(np.concatenate([x.int, x.bnd])) - 1
            inside = np.asarray(G[V][:, V].sum(axis=1)).reshape(-1)
            deg = np.asarray(G[V].sum(axis=1)).reshape(-1)
            assert np.array_equal(V[deg > inside] + 1, x.bnd)


@pytest.mark.parametrize("kind,shape,nmax,nb", CASES)
def test_tree_with_interface_and_oracle_schur(hs, kind, shape, nmax, nb):
    P = interface_problem(hs, kind, shape, nmax)
    n = P["n"]
    assert len(P["iface0"]) == nb and np.array_equal(P["iface0"], interface_ids(shape))
    raw = hs.problems.graph_nested_dissection(P["A0"], nmax, interface=P["iface0"])
    root, _ = hs.symfact(raw)
    assert np.array_equal(np.sort(root.bnd), P["iface0"] + 1)
    count = np.zeros(n + 1, dtype=np.int64)
    for x in hs.postorder_nodes(root):
        np.add.at(count, x.int, 1)
    rest = np.setdiff1d(np.arange(1, n + 1), P["iface0"] + 1)
    assert (count[rest] == 1).all() and (count[P["iface0"] + 1] == 0).all()  # every other DOF in exactly one int
    assert np.array_equal(P["perm"][n - nb:], root.bnd)  # postorder puts the interface last, in root.bnd's order
    assert np.array_equal(P["nd"].bnd, np.arange(n - nb + 1, n + 1)) and np.array_equal(P["iface"], np.arange(n - nb, n))
    ond = O.parse_elimtree(*P["arrays"])
    ond, ond_loc = O.symfact(ond)
    operm = O.postorder(ond)
    assert np.array_equal(operm, P["perm"])
    ond = O.permuted(ond, O.invperm(operm))
    S = np.asarray(O.factor(P["A"], ond, ond_loc, swlevel=0).S)
    ref, _ = dense_schur(P["A"], P["iface"])
    err = np.linalg.norm(S - ref) / np.linalg.norm(ref)
    print(f"{kind} {shape}: oracle F.S against the dense Schur complement {err:.2e}")
    assert S.shape == (nb, nb) and err <= 1e-12


def _plan_interface(hs, h):
    L = hs._lib.lib()
    nb = C.c_int64(-1)
    hs._lib.check(L.hs_interface_size(h, C.byref(nb)))
    idx = np.full(nb.value + 1, -9, dtype=np.int64)
    hs._lib.check(L.hs_interface_indices(h, idx.ctypes.data_as(hs._lib.p_i64)))
    assert idx[-1] == -9
    return nb.value, idx[:-1]


def test_plan_only_handles_know_their_interface(hs):
    L = hs._lib.lib()
    for kind, shape, nmax, nb in CASES[1:]:
        P = interface_problem(hs, kind, shape, nmax)
        h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"])
        try:
            got, idx = _plan_interface(hs, h)
            assert got == nb and np.array_equal(idx, P["nd"].bnd)  # 1-based, root.bnd as given
            out = np.zeros(8)
            hs._lib.check(L.hs_interface_info(h, out.ctypes.data_as(hs._lib.p_f64)))
            assert out[2] == nb and not out[[0, 1, 3, 4, 5, 6, 7]].any()
            # everything else needs a factorization: refused as an argument error, nothing written
            S = np.full((nb, nb), 7.0, dtype=np.complex128, order="F")
            assert L.hs_interface_matrix_z(h, S.ctypes.data, nb, 0, None) == hs._lib.HS_ERR_ARGUMENT and (S == 7.0).all()
            Cb = np.full((P["n"], 1), 7.0, dtype=np.complex128, order="F")
            for p in PHASES:
                assert getattr(L, f"hs_interface_{p}_z")(h, 0, Cb.ctypes.data_as(hs._lib.p_f64), P["n"], P["n"], 1) == hs._lib.HS_ERR_ARGUMENT
            assert (Cb == 7.0).all()
        finally:
            L.hs_free(h)
    P = interface_problem(hs, "convdiff", (30, 27), 40, with_interface=False)  # an ordinary tree: no interface
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"])
    try:
        got, idx = _plan_interface(hs, h)
        assert got == 0 and len(idx) == 0
    finally:
        L.hs_free(h)


def test_multi_rank_plan_is_unsupported(hs):
    L = hs._lib.lib()
    P = interface_problem(hs, "convdiff", (30, 27), 40)
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=2)
    try:
        assert _plan_interface(hs, h)[0] == 30  # the sizes are the plan's
        S = np.full((30, 30), 7.0, order="F")
        assert L.hs_interface_matrix_d(h, S.ctypes.data, 30, 0, None) == hs._lib.HS_ERR_UNSUPPORTED and (S == 7.0).all()
        Cb = np.full((P["n"], 2), 7.0, order="F")
        for p in PHASES:
            assert getattr(L, f"hs_interface_{p}_d")(h, 0, Cb.ctypes.data_as(hs._lib.p_f64), P["n"], P["n"], 2) == hs._lib.HS_ERR_UNSUPPORTED
            assert b"ranks" in L.hs_last_error()
        assert (Cb == 7.0).all()
    finally:
        L.hs_free(h)
