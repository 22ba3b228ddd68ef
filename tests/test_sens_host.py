"""Adjoint-state sensitivities on the CPU: the NumPy statement of hs_sens_* / hs_misfit_* (tests/sens_mirror.py), fed with SuperLU solves,
against central finite differences of the objective -- which pins the sign and every conjugation of the three rows of the table in
include/hs_solver.h -- the diagonal mode, and the new entry points of the C ABI with the refusals that need no device.  The device
implementation (csrc/hs_sens.hip, csrc/kernels_sens.hip) is checked in tests/test_sens_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import sens_mirror as SM
from helpers import prepare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hs_sens_d", "hs_sens_z", "hs_sens_dev_d", "hs_sens_dev_z", "hs_misfit_d", "hs_misfit_z", "hs_misfit_dev_d", "hs_misfit_dev_z", "hs_sens_info")
HOOKS = ("hsk_sddmm_d", "hsk_sddmm_z")
PROBLEMS = [("convdiff", (13, 7), 10), ("convdiff_helmholtz", (9, 9), 12)]  # real and complex, both unsymmetric, at most 91 unknowns
H, RTOL = 1e-5, 1e-6  # central differences: the error is the O(h^2) term


def _rand(shape, cplx, rng):
    M = rng.standard_normal(shape)
    return M + 1j * rng.standard_normal(shape) if cplx else M


def _problem(hs, kind, shape, nmax):
    A = SM.canonical(prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")["A"])
    cplx = np.iscomplexobj(A.data)
    assert abs(A - A.T).max() > 1e-3  # unsymmetric
    return A, cplx


def _perturbed(A, E, s):
    return sp.csc_matrix((A.data + s * E, A.indices, A.indptr), shape=A.shape)


@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_mirror_against_central_differences(hs, kind, shape, nmax):
    A, cplx = _problem(hs, kind, shape, nmax)
    n = A.shape[0]
    rng = np.random.default_rng(5)
    k = 3
    B, W = _rand((n, k), cplx, rng), _rand((n, k), cplx, rng)
    E = _rand(A.nnz, cplx, rng)  # random on the pattern
    for trans in (0, 1, 2):
        G, X, Lam = SM.sensitivity(A, SM.superlu_solver(A), B, W, trans)
        assert np.iscomplexobj(G) == cplx
        f = lambda s: float(np.real(np.vdot(W, SM.forward(SM.superlu_solver(_perturbed(A, E, s)), B, trans))))
        fd = (f(H) - f(-H)) / (2 * H)
        pred = float(np.real(np.sum(E * np.conj(G))))
        print(f"{kind} trans={trans}: finite difference {fd:.12e}, Re sum E conj(G) {pred:.12e}, relative {abs(fd - pred) / abs(fd):.2e}")
        assert abs(fd - pred) <= RTOL * abs(fd)


@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_misfit_mirror_against_central_differences(hs, kind, shape, nmax):
    A, cplx = _problem(hs, kind, shape, nmax)
    n = A.shape[0]
    rng = np.random.default_rng(6)
    k = 3
    B = _rand((n, k), cplx, rng)
    rows = rng.choice(n, size=7, replace=False)  # distinct, unsorted
    D = _rand((7, k), cplx, rng)
    E = _rand(A.nnz, cplx, rng)
    for trans in (0, 1, 2):
        J, G, R = SM.misfit(A, SM.superlu_solver(A), B, rows, D, trans)
        assert J.shape == (k,) and np.allclose(J, 0.5 * np.linalg.norm(R, axis=0) ** 2)
        # the misfit form is the general form with W = scatter(R)
        G2, _, _ = SM.sensitivity(A, SM.superlu_solver(A), B, SM.scatter(rows, R, n), trans)
        assert np.array_equal(G, G2)
        f = lambda s: float(SM.misfit(_perturbed(A, E, s), SM.superlu_solver(_perturbed(A, E, s)), B, rows, D, trans)[0].sum())
        fd = (f(H) - f(-H)) / (2 * H)
        pred = float(np.real(np.sum(E * np.conj(G))))
        print(f"{kind} trans={trans}: misfit finite difference {fd:.12e}, Re sum E conj(G) {pred:.12e}, relative {abs(fd - pred) / abs(fd):.2e}")
        assert abs(fd - pred) <= RTOL * abs(fd)


@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_diagonal_mode_is_the_diagonal_of_the_full_pattern(hs, kind, shape, nmax):
    A, cplx = _problem(hs, kind, shape, nmax)
    n = A.shape[0]
    rng = np.random.default_rng(7)
    B, W = _rand((n, 2), cplx, rng), _rand((n, 2), cplx, rng)
    for trans in (0, 1, 2):
        G, X, Lam = SM.sensitivity(A, SM.superlu_solver(A), B, W, trans)
        d = SM.diagonal(A, G)
        assert np.array_equal(d, sp.csc_matrix((G, A.indices, A.indptr), shape=A.shape).diagonal())
        # on the diagonal the index pairs coincide: one formula serves it whatever the swap
        want = {0: -(Lam * np.conj(X)).sum(axis=1), 1: -(Lam * np.conj(X)).sum(axis=1), 2: -(np.conj(Lam) * X).sum(axis=1)}[trans]
        assert np.array_equal(d, want)
    # a missing diagonal entry gives 0 there
    keep = ~((A.indices == 3) & (np.repeat(np.arange(n), np.diff(A.indptr)) == 3))
    i, j = SM.entry_index(A)
    A3 = SM.canonical(sp.csc_matrix((A.data[keep], (i[keep], j[keep])), shape=A.shape))
    assert SM.diag_positions(A3)[3] == -1 and SM.diagonal(A3, np.ones(A3.nnz))[3] == 0


def test_new_entry_points_are_declared_exported_and_bound(hs):
    lib = hs._lib.lib()
    E = hs._lib
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in E.EXPORTS and hasattr(lib, name)
    assert "hs_block_arg" in txt
    ktxt = open(os.path.join(ROOT, "include", "hs_kernels.h")).read()
    for name in HOOKS:
        assert re.search(r"\bint\s+%s\s*\(" % name, ktxt), name
        assert name in E.EXPORTS and hasattr(lib, name)
    for f in (hs.sensitivity, hs.sensitivity_matrix, hs.misfit, hs.sens_info):
        assert callable(f)
    # a null handle is refused by every entry point without a device
    b = E.hs_block_arg(None, 0, None, None, None)
    G = np.full(4, 42.0)
    for fn in (lib.hs_sens_d, lib.hs_sens_z):
        assert fn(None, 0, 2, 1, C.byref(b), C.byref(b), 0, 0, G.ctypes.data, None, 2, None, 2) == E.HS_ERR_ARGUMENT
    for fn in (lib.hs_sens_dev_d, lib.hs_sens_dev_z):
        assert fn(None, 0, 2, 1, C.byref(b), C.byref(b), 0, 0, G.ctypes.data, None, 2, None, 2, None) == E.HS_ERR_ARGUMENT
    for fn in (lib.hs_misfit_d, lib.hs_misfit_z):
        assert fn(None, 0, 2, 1, C.byref(b), None, 0, None, 1, 0, 0, G.ctypes.data, None, 1, G.ctypes.data) == E.HS_ERR_ARGUMENT
    for fn in (lib.hs_misfit_dev_d, lib.hs_misfit_dev_z):
        assert fn(None, 0, 2, 1, C.byref(b), None, 0, None, 1, 0, 0, G.ctypes.data, None, 1, G.ctypes.data, None) == E.HS_ERR_ARGUMENT
    assert lib.hs_sens_info(None, (C.c_double * 8)()) == E.HS_ERR_ARGUMENT
    assert np.all(G == 42.0)


def test_refusals_that_need_no_device(hs):
    E = hs._lib
    lib = E.lib()
    P = prepare(hs, (13, 7), kind="convdiff", nmax=10, rhs="randn")
    A = SM.canonical(P["A"])
    n = A.shape[0]
    rng = np.random.default_rng(8)
    B, W = rng.standard_normal((n, 2)), rng.standard_normal((n, 2))
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"])
    try:
        # a host-side plan holds no factorization: ArgumentError from every entry point, nothing written
        Bf, Wf = np.asfortranarray(B), np.asfortranarray(W)
        bB, bW = E.hs_block_arg(Bf.ctypes.data, n, None, None, None), E.hs_block_arg(Wf.ctypes.data, n, None, None, None)
        G = np.full(A.nnz, 42.0)
        X = np.full((n, 2), 42.0, order="F")
        J = np.full(2, 42.0)
        rows1 = np.array([1, 2, 3], dtype=np.int64)
        D = np.zeros((3, 2), order="F")
        for trans in (0, 1, 2):
            for pattern in (0, 1):
                assert lib.hs_sens_d(h, trans, n, 2, C.byref(bB), C.byref(bW), 0, pattern, G.ctypes.data, X.ctypes.data, n, None, n) == E.HS_ERR_ARGUMENT
                assert lib.hs_misfit_d(h, trans, n, 2, C.byref(bB), rows1.ctypes.data_as(E.p_i64), 3, D.ctypes.data, 3, 0, pattern, J.ctypes.data, None, 3,
                                       G.ctypes.data) == E.HS_ERR_ARGUMENT
        assert lib.hs_sens_z(h, 0, n, 2, C.byref(bB), C.byref(bW), 0, 0, G.ctypes.data, None, n, None, n) == E.HS_ERR_ARGUMENT  # the element type
        assert lib.hs_sens_d(h, 3, n, 2, C.byref(bB), C.byref(bW), 0, 0, G.ctypes.data, None, n, None, n) == E.HS_ERR_ARGUMENT
        assert lib.hs_sens_d(h, 0, n, 2, C.byref(bB), C.byref(bW), 0, 2, G.ctypes.data, None, n, None, n) == E.HS_ERR_ARGUMENT
        assert lib.hs_sens_d(h, 0, n, 2, C.byref(bB), C.byref(bW), -1, 0, G.ctypes.data, None, n, None, n) == E.HS_ERR_ARGUMENT
        assert np.all(G == 42.0) and np.all(X == 42.0) and np.all(J == 42.0)
        with pytest.raises(ValueError, match="plan"):
            hs.sensitivity(h, B, W)
        with pytest.raises(ValueError, match="plan"):
            hs.misfit(h, B, [0, 1, 2], np.zeros((3, 2)))
        # shapes and dtypes are checked by the Python layer
        with pytest.raises(hs.DimensionMismatch):
            hs.sensitivity(h, B[:-1], W)
        with pytest.raises(hs.DimensionMismatch):
            hs.sensitivity(h, B, W[:, :1])
        with pytest.raises(hs.DimensionMismatch):
            hs.sensitivity(h, sp.csc_matrix(B)[:-1], W)
        with pytest.raises(TypeError, match="MethodError"):
            hs.sensitivity(h, B + 1j, W)
        with pytest.raises(TypeError, match="MethodError"):
            hs.sensitivity(h, B, sp.csc_matrix(W) * 1j)
        with pytest.raises(ValueError, match="pattern"):
            hs.sensitivity(h, B, W, pattern="rows")
        with pytest.raises(ValueError, match="want"):
            hs.sensitivity(h, B, W, want=("Y",))
        with pytest.raises(hs.DimensionMismatch):
            hs.misfit(h, B, [0, 1, 2], np.zeros((2, 2)))
        with pytest.raises(hs.DimensionMismatch):
            hs.misfit(h, B, [0, n], np.zeros((2, 2)))
        with pytest.raises(TypeError, match="MethodError"):
            hs.misfit(h, B, [0, 1], np.zeros((2, 2)) + 1j)
    finally:
        lib.hs_free(h)
