"""GMRES on transposed / adjoint systems and on the handle's own A (hs_gmres_t_*, hs_gmres_block_t_*) without a GPU: the entry points of
the C ABI and their bindings, the Python arguments, the refusals the library names from host-side plans (hs_plan) before any device work, and
the reference of the GPU tests (tests/gmres_block_mirror.py on op(A)) against the conditions those tests assert.  The device implementation is
checked in tests/test_gmres_op_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import gmres_block_mirror as M
from helpers import prepare, relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hs_gmres_t_d", "hs_gmres_t_z", "hs_gmres_block_t_d", "hs_gmres_block_t_z")
HOOKS = ("hsk_spmm_op_d", "hsk_spmm_op_z")

# the problems of tests/test_gmres_op_gpu.py
PROBLEMS = [("convdiff", (30, 27), 40), ("convdiff_helmholtz", (30, 27), 40), ("convdiff", (20, 20, 20), 300), ("convdiff_helmholtz", (20, 20, 20), 300)]


def test_new_symbols_are_declared_exported_and_bound(hs):
    lib = hs._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    khdr = open(os.path.join(ROOT, "include", "hs_kernels.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(hs_handle\* Pr, int trans," % name, hdr), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
        f = getattr(lib, name)
        assert f.restype is C.c_int and f.argtypes[1] is C.c_int  # trans
    # the arguments after trans are those of the entry point without _t
    for a, b in (("hs_gmres_t_d", "hs_gmres_d"), ("hs_gmres_t_z", "hs_gmres_z"), ("hs_gmres_block_t_d", "hs_gmres_block_d"), ("hs_gmres_block_t_z", "hs_gmres_block_z")):
        fa, fb = getattr(lib, a), getattr(lib, b)
        assert list(fa.argtypes[:1]) + list(fa.argtypes[2:]) == list(fb.argtypes)
    for name in HOOKS:
        assert re.search(r"\bint\s+%s\s*\(int trans," % name, khdr), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes[0] is C.c_int
    import inspect

    for fn in (hs.gmres, hs.gmres_block):
        sig = inspect.signature(fn)
        assert sig.parameters["trans"].default is None  # "N" unless Pr = transpose(F) / adjoint(F) says otherwise


def test_python_arguments(hs):
    """trans letters, Pr = transpose(F) / adjoint(F) as shorthand, conflicting pairs, A = None without a handle."""
    from hierarchicalsolvers_jl_amd.gmres import _op_of

    Fz = object.__new__(hs.FactorNode)
    Fz._h, Fz.dtype, Fz.n, Fz._flat = None, np.dtype(np.complex128), 7, None
    Fr = object.__new__(hs.FactorNode)
    Fr._h, Fr.dtype, Fr.n, Fr._flat = None, np.dtype(np.float64), 7, None
    assert _op_of(None, None) == (None, 0) and _op_of(Fz, None) == (Fz, 0) and _op_of(Fz, "N") == (Fz, 0)
    assert _op_of(Fz, "T") == (Fz, 1) and _op_of(Fz, "C") == (Fz, 2) and _op_of(None, "T") == (None, 1)
    assert _op_of(hs.transpose(Fz), None) == (Fz, 1) and _op_of(hs.adjoint(Fz), None) == (Fz, 2)
    assert _op_of(hs.transpose(Fz), "T") == (Fz, 1) and _op_of(hs.adjoint(Fz), "C") == (Fz, 2)
    for Pr, t in ((hs.transpose(Fz), "N"), (hs.transpose(Fz), "C"), (hs.adjoint(Fz), "T"), (hs.adjoint(Fz), "N"), (hs.transpose(Fr), "N")):
        with pytest.raises(ValueError, match="conflicts"):
            _op_of(Pr, t)
    assert _op_of(hs.transpose(Fr), "C") == (Fr, 1) and _op_of(hs.adjoint(Fr), "T") == (Fr, 2)  # Float64: adjoint = transpose
    for fn in (hs.gmres, hs.gmres_block):
        with pytest.raises(ValueError, match="trans must be"):
            fn(None, np.zeros(7), Pr=Fr, trans="X")
        with pytest.raises(ValueError, match="A=None"):
            fn(None, np.zeros(7))
        with pytest.raises(ValueError, match="conflicts"):
            fn(None, np.zeros(7), Pr=hs.transpose(Fz), trans="C")


def _plan(hs, P, **kw):
    return hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], **kw)


class _Caller:
    """Calls the four new entry points with A = P["A"] (own=False) or the three arrays NULL (own=True) on host vectors filled with a sentinel."""

    def __init__(self, hs, A):
        from hierarchicalsolvers_jl_amd.gmres import _csc_fields

        self.hs, self.L, self.n = hs, hs._lib.lib(), A.shape[0]
        self.colptr, self.rowval, self.nz = _csc_fields(A, np.float64)
        self.b = np.ones((self.n, 2), order="F")
        self.x = np.full((self.n, 2), 42.0, order="F")
        self.iters = np.zeros(2, dtype=np.int64)
        self.conv = np.zeros(2, dtype=np.int32)

    def __call__(self, h, trans, own=False, block=False, partial=None):
        pi = self.hs._lib.p_i64
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        a3 = [self.colptr.ctypes.data_as(pi), self.rowval.ctypes.data_as(pi), vp(self.nz)]
        if own:
            a3 = [None, None, None]
        if partial is not None:
            a3[partial] = None
        pc = self.conv.ctypes.data_as(C.POINTER(C.c_int))
        if block:
            st = self.L.hs_gmres_block_t_d(h, trans, self.n, *a3, vp(self.b), self.n, vp(self.x), self.n, 2, 0, 0, 1e-8, 0.0, 5, 10, None, self.iters.ctypes.data_as(pi), pc, None)
        else:
            st = self.L.hs_gmres_t_d(h, trans, self.n, *a3, vp(self.b), vp(self.x), 0, 0, 1e-8, 0.0, 5, 10, None, self.iters.ctypes.data_as(pi), pc, None)
        assert np.all(self.x == 42.0)  # refused: x untouched
        return st, self.L.hs_last_error().decode()


def test_refusals_are_named_before_device_work(hs):
    E = hs._lib
    L = E.lib()
    P = prepare(hs, (20, 12), kind="convdiff", nmax=10)
    call = _Caller(hs, P["A"])
    # trans outside 0..2, A passed in part, own A without a handle: argument errors whatever the handle is
    for block in (False, True):
        for trans in (3, -1):
            st, msg = call(None, trans, block=block)
            assert st == E.HS_ERR_ARGUMENT and "trans" in msg
        for trans in (0, 1, 2):
            st, msg = call(None, trans, own=True, block=block)
            assert st == E.HS_ERR_ARGUMENT and "NULL" in msg
            for part in (0, 1, 2):
                st, msg = call(None, trans, block=block, partial=part)
                assert st == E.HS_ERR_ARGUMENT and "all be NULL" in msg
    # more than one rank: transposed solves and the handle's own A
    for kw in (dict(rank=0, nranks=2), dict(rank=1, nranks=2, dist_top=True)):
        h = _plan(hs, P, **kw)
        try:
            for trans in (1, 2):
                st, msg = call(h, trans)
                assert st == E.HS_ERR_UNSUPPORTED and "ranks" in msg, (kw, trans, st, msg)
            for block in (False, True):
                for trans in (0, 1, 2):
                    st, msg = call(h, trans, own=True, block=block)
                    assert st == E.HS_ERR_UNSUPPORTED and "ranks" in msg, (kw, trans, block, st, msg)
                assert call(h, 3, block=block)[0] == E.HS_ERR_ARGUMENT and call(h, -1, own=True, block=block)[0] == E.HS_ERR_ARGUMENT
        finally:
            L.hs_free(h)
    # a single-rank plan passes the refusals and stops at "not complete"
    h = _plan(hs, P)
    try:
        for block in (False, True):
            for trans, own in ((1, False), (2, False), (0, True), (1, True), (2, True)):
                st, msg = call(h, trans, own=own, block=block)
                assert st == E.HS_ERR_ARGUMENT and "not complete" in msg, (trans, own, block, st, msg)
        # a handle of another size
        small = _Caller(hs, P["A"][:50, :50].tocsc())
        assert small(h, 1)[0] == E.HS_ERR_DIMENSION and small(h, 0, own=True)[0] == E.HS_ERR_DIMENSION and small(h, 1, own=True, block=True)[0] == E.HS_ERR_DIMENSION
    finally:
        L.hs_free(h)
    # interior blocks kept as HSS matrices: no transposed ULV solve
    P3 = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512)
    call3 = _Caller(hs, P3["A"])
    for kw in (dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128), dict(swlevel=3, swsize=8, atol=1e-6, rtol=1e-6, mf=3, leafsize=128)):
        h = _plan(hs, P3, **kw)
        try:
            for own in (False, True):
                st, msg = call3(h, 1, own=own)
                assert st == E.HS_ERR_UNSUPPORTED and "HSS" in msg and "ULV" in msg, (kw, own, st, msg)
        finally:
            L.hs_free(h)


@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_reference_meets_the_conditions_of_the_gpu_tests(hs, kind, shape, nmax):
    """gmres_single on transpose(A) and adjoint(A) with an exact LU of op(A) as right preconditioner: at most 2 iterations, the solution of
    op(A) x = b, and a solution that differs from that of A x = b (the problems are nonsymmetric: a dropped `trans` cannot pass)."""
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    A = P["A"]
    b = P["b"]
    cplx = np.iscomplexobj(A.data)
    kw = dict(reltol=1e-9, restart=30, maxiter=30)
    xN = spla.splu(A.tocsc()).solve(b)
    sols = {}
    for name, Aop in (("T", A.T), ("C", A.conj().T)):
        lu = spla.splu(Aop.tocsc())
        x, ch = M.gmres_single(Aop.tocsr(), b, prec=lu.solve, **kw)
        assert ch["isconverged"] and ch["iters"] <= 2, (kind, name, ch)
        assert relerr(x, lu.solve(b)) < 1e-8
        assert np.linalg.norm(Aop @ x - b) <= 1e-8 * np.linalg.norm(b)
        assert relerr(x, xN) > 1e-3
        sols[name] = x
    if cplx:
        assert relerr(sols["C"], sols["T"]) > 1e-3
    else:
        assert np.array_equal(sols["C"], sols["T"])
