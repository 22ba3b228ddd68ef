"""Tangent-linear solves and Gauss-Newton products on the CPU: the NumPy statement of hs_tangent_* / hs_gn_hessvec_* / hs_gn_diag_*
(tests/gn_mirror.py), fed with SuperLU solves, against central finite differences of the fields themselves, the adjoint identity that ties
the forward mode to the reverse mode of tests/sens_mirror.py, the symmetry of the Gauss-Newton product and its diagonal -- and the new entry
points of the C ABI with the refusals that need no device.  The device implementation (csrc/hs_gn.hip, csrc/kernels_gn.hip) is checked in
tests/test_gn_gpu.py.

The bound 64 eps of the three rounding identities: both sides are sums of at most n k <= 273 products of the same solves, so they differ by
rounding alone; measured with SuperLU at most 3.4e-17 (adjoint identity), 4.3e-16 (symmetry) and 8.2e-16 (diagonal), relative to the norm
products named in each test."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import gn_mirror as GM
import sens_mirror as SM
from helpers import prepare
from test_sens_host import H, PROBLEMS, RTOL, _perturbed, _problem, _rand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hs_tangent_d", "hs_tangent_z", "hs_tangent_dev_d", "hs_tangent_dev_z", "hs_gn_hessvec_d", "hs_gn_hessvec_z", "hs_gn_hessvec_dev_d", "hs_gn_hessvec_dev_z",
       "hs_gn_diag_d", "hs_gn_diag_z", "hs_gn_diag_dev_d", "hs_gn_diag_dev_z", "hs_gn_info")
HOOKS = ("hsk_gn_rhs_d", "hsk_gn_rhs_z", "hsk_gn_rowsq_d", "hsk_gn_rowsq_z")
EPS = float(np.finfo(np.float64).eps)
K, NROWS = 3, 7
PATTERNS = ("A", "diag")


def _direction(A, pattern, cplx, rng):
    return _rand(A.nnz if pattern == "A" else A.shape[0], cplx, rng)


def _setup(hs, kind, shape, nmax, seed):
    A, cplx = _problem(hs, kind, shape, nmax)
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    B = _rand((n, K), cplx, rng)
    rows = rng.choice(n, size=NROWS, replace=False)  # distinct, unsorted
    assert np.any(np.diff(rows) < 0)
    return A, cplx, n, rng, B, rows


@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_mirror_tangent_against_central_differences(hs, kind, shape, nmax):
    A, cplx, n, rng, B, rows = _setup(hs, kind, shape, nmax, 21)
    for pattern in PATTERNS:
        E = _direction(A, pattern, cplx, rng)
        Ef = GM.embed(A, E, pattern)
        for trans in (0, 1, 2):
            dX, X = GM.tangent(A, SM.superlu_solver(A), B, E, trans, pattern)
            f = lambda s: SM.forward(SM.superlu_solver(_perturbed(A, Ef, s)), B, trans)
            fd = (f(H) - f(-H)) / (2 * H)
            err = np.linalg.norm(fd - dX) / np.linalg.norm(fd)
            print(f"{kind} pattern={pattern} trans={trans}: ||fd - dX||_F / ||fd||_F = {err:.2e}")
            assert err <= RTOL


@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_mirror_adjoint_identity_with_the_reverse_mode(hs, kind, shape, nmax):
    A, cplx, n, rng, B, rows = _setup(hs, kind, shape, nmax, 22)
    W = _rand((n, K), cplx, rng)
    solve = SM.superlu_solver(A)
    for pattern in PATTERNS:
        E = _direction(A, pattern, cplx, rng)
        for trans in (0, 1, 2):
            dX, X = GM.tangent(A, solve, B, E, trans, pattern)
            G = SM.sensitivity(A, solve, B, W, trans)[0]
            lhs = float(np.real(np.vdot(W, dX)))
            rhs = float(np.real(np.sum(GM.embed(A, E, pattern) * np.conj(G))))
            rel = abs(lhs - rhs) / (np.linalg.norm(W) * np.linalg.norm(dX))
            print(f"{kind} pattern={pattern} trans={trans}: |Re<W, dX> - Re sum E conj(G)| / (||W|| ||dX||) = {rel:.2e}")
            assert rel <= 64 * EPS


@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_mirror_gauss_newton_product_is_symmetric(hs, kind, shape, nmax):
    A, cplx, n, rng, B, rows = _setup(hs, kind, shape, nmax, 23)
    solve = SM.superlu_solver(A)
    for pattern in PATTERNS:
        E1, E2 = _direction(A, pattern, cplx, rng), _direction(A, pattern, cplx, rng)
        for trans in (0, 1, 2):
            H1, J1, X = GM.gn_hessvec(A, solve, B, rows, E1, trans, pattern)
            H2, J2, _ = GM.gn_hessvec(A, solve, B, rows, E2, trans, pattern, X=X)
            assert H1.shape == E1.shape and J1.shape == (NROWS, K)
            jj = float(np.real(np.vdot(J1, J2)))
            scale = np.linalg.norm(J1) * np.linalg.norm(J2)
            r12 = abs(float(np.real(np.vdot(H2, E1))) - jj) / scale  # Re<E1, H E2>
            r21 = abs(float(np.real(np.vdot(H1, E2))) - jj) / scale
            print(f"{kind} pattern={pattern} trans={trans}: |Re<E1, H E2> - Re<J E1, J E2>| = {r12:.2e}, exchanged {r21:.2e} (relative to ||J E1|| ||J E2||)")
            assert r12 <= 64 * EPS and r21 <= 64 * EPS


@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_mirror_diagonal_of_the_gauss_newton_product(hs, kind, shape, nmax):
    A, cplx, n, rng, B, rows = _setup(hs, kind, shape, nmax, 24)
    solve = SM.superlu_solver(A)
    pos = SM.diag_positions(A)
    for pattern in PATTERNS:
        length = A.nnz if pattern == "A" else n
        for trans in (0, 1, 2):
            Hd, z2, x2 = GM.gn_diag(A, solve, B, rows, trans, pattern)
            assert Hd.dtype == np.float64 and Hd.shape == (length,) and np.all(Hd >= 0)
            if pattern == "diag":
                assert np.array_equal(Hd, GM.gn_diag(A, solve, B, rows, trans, "A")[0][pos])
            for p in rng.choice(length, size=6, replace=False):
                for unit in ((1.0, 1j) if cplx else (1.0,)):  # the same for the directions e_p and i e_p
                    e = np.zeros(length, dtype=A.dtype)
                    e[p] = unit
                    HE, JE, _ = GM.gn_hessvec(A, solve, B, rows, e, trans, pattern)
                    r1 = abs(float(np.real(np.conj(unit) * HE[p])) - Hd[p]) / Hd[p]
                    r2 = abs(np.linalg.norm(JE) ** 2 - Hd[p]) / Hd[p]
                    assert r1 <= 64 * EPS and r2 <= 64 * EPS, (pattern, trans, p, r1, r2)


def test_new_entry_points_are_declared_exported_and_bound(hs):
    lib = hs._lib.lib()
    E = hs._lib
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in E.EXPORTS and hasattr(lib, name)
    ktxt = open(os.path.join(ROOT, "include", "hs_kernels.h")).read()
    for name in HOOKS:
        assert re.search(r"\bint\s+%s\s*\(" % name, ktxt), name
        assert name in E.EXPORTS and hasattr(lib, name)
    for f in (hs.tangent, hs.gn_hessvec, hs.gn_diag, hs.gn_info):
        assert callable(f)


def test_refusals_that_need_no_device(hs):
    E = hs._lib
    lib = E.lib()
    P = prepare(hs, (13, 7), kind="convdiff", nmax=10, rhs="randn")
    A = SM.canonical(P["A"])
    n = A.shape[0]
    rng = np.random.default_rng(25)
    B = np.asfortranarray(rng.standard_normal((n, 2)))
    bB = E.hs_block_arg(B.ctypes.data, n, None, None, None)
    Ev = rng.standard_normal(A.nnz)
    rows1 = np.array([3, 1, 2], dtype=np.int64)
    pr = rows1.ctypes.data_as(E.p_i64)
    out = dict(dX=np.full((n, 2), 42.0, order="F"), X=np.full((n, 2), 42.0, order="F"), HE=np.full(A.nnz, 42.0), JE=np.full((3, 2), 42.0, order="F"),
               Hd=np.full(A.nnz, 42.0), z2=np.full(n, 42.0), x2=np.full(n, 42.0))
    o = {k: v.ctypes.data for k, v in out.items()}

    def calls(h, trans=0, pattern=0, itmax=0, B_=C.byref(bB), Xin=None):
        return [lib.hs_tangent_d(h, trans, n, 2, B_, Xin, n, Ev.ctypes.data, pattern, itmax, None, 0, o["dX"], n, o["X"], n),
                lib.hs_tangent_dev_d(h, trans, n, 2, B_, Xin, n, Ev.ctypes.data, pattern, itmax, pr, 3, o["dX"], n, o["X"], n, None),
                lib.hs_gn_hessvec_d(h, trans, n, 2, B_, Xin, n, Ev.ctypes.data, pattern, itmax, pr, 3, o["HE"], o["JE"], 3, o["X"], n),
                lib.hs_gn_hessvec_dev_d(h, trans, n, 2, B_, Xin, n, Ev.ctypes.data, pattern, itmax, pr, 3, o["HE"], o["JE"], 3, o["X"], n, None),
                lib.hs_gn_diag_d(h, trans, n, 2, B_, Xin, n, pr, 3, pattern, itmax, o["Hd"], o["z2"], o["x2"]),
                lib.hs_gn_diag_dev_d(h, trans, n, 2, B_, Xin, n, pr, 3, pattern, itmax, o["Hd"], o["z2"], o["x2"], None)]

    def refused(h, word, **kw):
        for st in calls(h, **kw):
            assert st == E.HS_ERR_ARGUMENT
            assert word in lib.hs_last_error().decode(), (word, lib.hs_last_error())

    refused(None, "null factorization handle")
    assert lib.hs_gn_info(None, (C.c_double * 8)()) == E.HS_ERR_ARGUMENT
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"])
    try:
        refused(h, "trans = 3", trans=3)
        refused(h, "pattern = 2", pattern=2)
        refused(h, "itmax", itmax=-1)
        refused(h, "B and Xin are both NULL", B_=None)
        refused(h, "plan")  # a host-side plan holds no factorization
        refused(h, "plan", B_=None, Xin=B.ctypes.data)
        z = (lib.hs_tangent_z, lib.hs_gn_hessvec_z)
        assert z[0](h, 0, n, 2, C.byref(bB), None, n, Ev.ctypes.data, 0, 0, None, 0, o["dX"], n, None, n) == E.HS_ERR_ARGUMENT  # the element type
        assert "eltype" in lib.hs_last_error().decode()
        assert z[1](h, 0, n, 2, C.byref(bB), None, n, Ev.ctypes.data, 0, 0, pr, 3, o["HE"], None, 3, None, n) == E.HS_ERR_ARGUMENT
        assert lib.hs_gn_diag_z(h, 0, n, 2, C.byref(bB), None, n, pr, 3, 0, 0, o["Hd"], None, None) == E.HS_ERR_ARGUMENT
        for v in out.values():
            assert np.all(v == 42.0)
        # the Python layer: the same refusals by class, shapes and dtypes before the call
        with pytest.raises(ValueError, match="plan"):
            hs.tangent(h, B, np.zeros(0))
        with pytest.raises(ValueError, match="both None"):
            hs.gn_hessvec(h, None, [0, 1], np.zeros(0))
        with pytest.raises(ValueError, match="pattern"):
            hs.gn_diag(h, B, [0, 1], pattern="rows")
        with pytest.raises(ValueError, match="want"):
            hs.gn_hessvec(h, B, [0, 1], np.zeros(0), want=("Lam",))
        with pytest.raises(hs.DimensionMismatch):
            hs.tangent(h, B[:-1], np.zeros(0))
        with pytest.raises(hs.DimensionMismatch):
            hs.tangent(h, B, np.zeros(0), X=B[:, :1])
        with pytest.raises(hs.DimensionMismatch):
            hs.tangent(h, B, np.zeros(n - 1), pattern="diag")
        with pytest.raises(hs.DimensionMismatch):
            hs.gn_hessvec(h, B, [0, n], np.zeros(0))
        with pytest.raises(TypeError, match="MethodError"):
            hs.tangent(h, B + 1j, np.zeros(0))
        with pytest.raises(TypeError, match="MethodError"):
            hs.gn_hessvec(h, B, [0, 1], np.zeros(n) + 1j, pattern="diag")
        with pytest.raises(TypeError, match="MethodError"):
            hs.gn_diag(h, None, [0, 1], X=B + 1j)
    finally:
        lib.hs_free(h)
