"""Transposed and adjoint ULV solves on the CPU: the NumPy statement of the sweeps (tests/ulv_t_mirror.py) on the oracle's factors against
dense solves, the front-level formulas of hs_ldiv_ulv_* on small dense blocks, and the new entry points of the C ABI (exports, bindings,
argument checks that need no device).  The device implementation is checked in tests/test_ulv_t_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ulv_t_mirror as M
from helpers import prepare
from oracle import hs_hss as HS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12  # relative; the mirror measures 2e-15 on these shapes, the bound only allows for other BLAS builds


def kernel_matrix(n, complex_=False, seed=0):
    """Non-symmetric, diagonally dominant matrix with smooth off-diagonal blocks (1-D points)."""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.random(n))
    d = np.abs(x[:, None] - x[None, :])
    A = 1.0 / (1.0 + 40.0 * d) + 0.3 * np.sin(3.0 * x)[:, None] * np.cos(2.0 * x)[None, :]
    if complex_:
        A = A * np.exp(1j * 2.0 * d)
    return A + n * 0.05 * np.eye(n)


def relerr(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def rhs(n, q, complex_, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, q))
    return X + 1j * rng.standard_normal((n, q)) if complex_ else X


def check_mirror(Ho, complex_):
    E = HS.hss_full(Ho)
    assert np.abs(E - E.T).max() > 1e-3  # non-symmetric: a solve in the wrong direction cannot pass
    F = HS.rs_factor(Ho)
    for q in (1, 3):
        B = rhs(Ho.n, q, complex_, q)
        e0 = relerr(HS.rs_solve(F, B), np.linalg.solve(E, B))
        et = relerr(M.rs_solve_t(F, B), np.linalg.solve(E.T, B))
        eh = relerr(M.rs_solve_t(F, B, adjoint=True), np.linalg.solve(E.conj().T, B))
        print(f"n={Ho.n} q={q} complex={complex_}: forward {e0:.1e}  transposed {et:.1e}  adjoint {eh:.1e}")
        assert e0 < TOL and et < TOL and eh < TOL
        assert relerr(HS.rs_solve(F, B), np.linalg.solve(E.T, B)) > 1e-4
    b = rhs(Ho.n, 1, complex_, 9)[:, 0]
    assert M.rs_solve_t(F, b).shape == (Ho.n,)


@pytest.mark.parametrize("complex_", [False, True])
@pytest.mark.parametrize("n,leaf", [(70, 16), (500, 40), (1200, 64)])
def test_mirror_against_dense_solves(n, leaf, complex_):
    Ho = HS.compress(kernel_matrix(n, complex_), leafsize=leaf, atol=1e-8, rtol=1e-8, kest=32)
    assert len(Ho.nodes) >= 3
    check_mirror(Ho, complex_)


@pytest.mark.parametrize("complex_", [False, True])
def test_mirror_single_leaf_and_permuted(complex_):
    H1 = HS.compress(kernel_matrix(48, complex_), leafsize=64)
    assert len(H1.nodes) == 1
    check_mirror(H1, complex_)
    # a permuted matrix: H ~ A[perm][:, perm]; the permutation is symmetric, so gather b[perm], solve, scatter -- as the forward solve does
    n = 300
    perm = np.random.default_rng(11).permutation(n)
    K = kernel_matrix(n, complex_)
    A = np.zeros_like(K)
    A[np.ix_(perm, perm)] = K
    Ho = HS.compress(A[perm][:, perm], leafsize=40, atol=1e-8, rtol=1e-8, kest=32)
    F = HS.rs_factor(Ho)
    Ef = np.zeros_like(K)
    Ef[np.ix_(perm, perm)] = HS.hss_full(Ho)
    B = rhs(n, 3, complex_, 4)
    for adj in (False, True):
        X = np.empty_like(B)
        X[perm] = M.rs_solve_t(F, B[perm], adjoint=adj)
        assert relerr(X, np.linalg.solve(Ef.conj().T if adj else Ef.T, B)) < TOL


@pytest.mark.parametrize("complex_", [False, True])
@pytest.mark.parametrize("block2x2", [False, True])
def test_front_formulas_against_a_dense_solve(complex_, block2x2):
    """One front [D Aib; Abi Abb] above a dense remainder: forward step, a dense solve with the Schur complement, backward step."""
    rng = np.random.default_rng(3)
    ni, nb, rL, rR, q = 23, 17, 5, 4, 3

    def rnd(*s):
        a = rng.standard_normal(s)
        return a + 1j * rng.standard_normal(s) if complex_ else a

    D = rnd(ni, ni) + 6.0 * np.eye(ni)
    n1 = 11
    if block2x2:  # off-diagonal blocks of D of low rank, as the 2 x 2 block form keeps them
        C12, Z12, C21, Z21 = rnd(n1, 3), rnd(3, ni - n1), rnd(ni - n1, 2), rnd(2, n1)
        D[:n1, n1:] = C12 @ Z12
        D[n1:, :n1] = C21 @ Z21
    CL, ZL, CR, ZR = rnd(nb, rL), rnd(rL, ni), rnd(ni, rR), rnd(rR, nb)
    Abb = rnd(nb, nb) + 6.0 * np.eye(nb)
    A = np.block([[D, CR @ ZR], [CL @ ZL, Abb]])
    W = np.linalg.solve(D, CR)
    S = Abb - CL @ ZL @ W @ ZR  # what the parent sees
    for trans in (0, 1, 2):
        opm = (lambda a: a) if trans == 0 else ((lambda a: a.T) if trans == 1 else (lambda a: a.conj().T))
        if block2x2 and trans:
            A11, S22 = D[:n1, :n1], D[n1:, n1:] - D[n1:, :n1] @ np.linalg.solve(D[:n1, :n1], D[:n1, n1:])
            dt = M.block_dsolve_t(trans, lambda b: np.linalg.solve(opm(A11), b), lambda b: np.linalg.solve(opm(S22), b), np.linalg.solve(A11, C12), Z12, C21, Z21, n1)
            dsolve = lambda b, t: dt(b)
        else:
            dsolve = lambda b, t: np.linalg.solve(opm(D), b)
        B = rnd(ni + nb, q)
        ti, bb = M.front_forward(trans, dsolve, W, ZR, CL, ZL, B[:ni], B[ni:])
        xb = np.linalg.solve(opm(S), bb)
        xi = M.front_backward(trans, dsolve, W, ZR, CL, ZL, ti, xb)
        e = relerr(np.vstack([xi, xb]), np.linalg.solve(opm(A), B))
        print(f"complex={complex_} 2x2={block2x2} trans={trans}: {e:.1e}")
        assert e < TOL


def test_new_entry_points_are_declared_exported_and_bound(hs):
    stxt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    htxt = open(os.path.join(ROOT, "include", "hs_hss.h")).read()
    ktxt = open(os.path.join(ROOT, "include", "hs_kernels.h")).read()
    lib = hs._lib.lib()
    for txt, names in ((stxt, ("hs_ldiv_ulv_d", "hs_ldiv_ulv_z", "hs_ldiv_ulv_dev_d", "hs_ldiv_ulv_dev_z")), (htxt, ("hs_hss_ldiv_t",)),
                       (ktxt, ("hsk_ulv_t_group_d", "hsk_ulv_t_group_z"))):
        for name in names:
            assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
            assert name in hs._lib.EXPORTS and hasattr(lib, name), name
    assert callable(hs.ldiv_ulv)
    import inspect

    assert "trans" in inspect.signature(hs.hss.HssMatrix.ldiv).parameters


def test_argument_checks_need_no_device(hs):
    lib = hs._lib.lib()
    E = hs._lib
    b = np.full(4, 42.0)
    pb = b.ctypes.data_as(E.p_f64)
    for trans in (0, 1, 2, 3, -1):
        for fn in (lib.hs_ldiv_ulv_d, lib.hs_ldiv_ulv_z):
            assert fn(None, trans, pb, 2, pb, 2, 2, 1) == E.HS_ERR_ARGUMENT
        for fn in (lib.hs_ldiv_ulv_dev_d, lib.hs_ldiv_ulv_dev_z):
            assert fn(None, trans, None, 2, None, 2, 2, 1, None) == E.HS_ERR_ARGUMENT
        assert lib.hs_hss_ldiv_t(None, trans, b.ctypes.data_as(C.c_void_p), 2, 1, 0) == E.HS_ERR_ARGUMENT
    # the hook refuses bad job lists before it looks for a device
    d = (C.c_int64 * 10)(2, 2, 2, 1, 2, 2, 0, 0, 0, 0)  # lda < K
    for fn in (lib.hsk_ulv_t_group_d, lib.hsk_ulv_t_group_z):
        assert fn(1, d, pb, 4, pb, 4, pb, 4, 0) == E.HS_ERR_ARGUMENT
        assert fn(0, d, pb, 4, pb, 4, pb, 4, 0) == E.HS_ERR_ARGUMENT
    assert np.all(b == 42.0)
    # a host-side plan (no device behind it): trans outside 0..2 is an argument error, the output untouched
    P = prepare(hs, (12, 12), kind="convdiff", nmax=20, rhs="randn")
    n = P["A"].shape[0]
    Bm = np.zeros((n, 2), order="F")
    Cm = np.full((n, 2), 42.0, order="F")
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"])
    try:
        for bad in (3, -1):
            assert lib.hs_ldiv_ulv_d(h, bad, Cm.ctypes.data_as(E.p_f64), n, Bm.ctypes.data_as(E.p_f64), n, n, 2) == E.HS_ERR_ARGUMENT
        assert np.all(Cm == 42.0)
    finally:
        lib.hs_free(h)


def test_a_plan_over_several_ranks_is_refused(hs):
    lib = hs._lib.lib()
    E = hs._lib
    P = prepare(hs, (12, 12), kind="convdiff", nmax=20, rhs="randn")
    n = P["A"].shape[0]
    Bm = np.zeros((n, 2), order="F")
    Cm = np.full((n, 2), 42.0, order="F")
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=2)
    try:
        for trans in (0, 1, 2):
            assert lib.hs_ldiv_ulv_d(h, trans, Cm.ctypes.data_as(E.p_f64), n, Bm.ctypes.data_as(E.p_f64), n, n, 2) == E.HS_ERR_UNSUPPORTED
            assert "2 ranks" in lib.hs_last_error().decode()
            assert lib.hs_ldiv_ulv_dev_d(h, trans, None, n, None, n, n, 2, None) == E.HS_ERR_UNSUPPORTED
        assert np.all(Cm == 42.0)
    finally:
        lib.hs_free(h)
