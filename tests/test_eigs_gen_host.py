"""Generalized shift-invert eigenpairs A x = lambda M x (hs.eigs(..., M=), hs_eigs_gen_*) on the CPU: the NumPy statement of the driver
(tests/eigs_gen_mirror.py on the loop of tests/eigs_mirror.py, SuperLU as the solve) on the five test pencils, the new entry points of the C
ABI, the Python argument checks and the checks of M on host-side plans.  The device implementation is checked in tests/test_eigs_gen_gpu.py.

Bounds, with r_c = ||op(A_s) x_c - mu_c op(M) x_c||_2 computed here from the mirror's vectors:
  Hermitian A, Hermitian positive definite M:  min_i |lambda_i - lambda| <= ||r||_{M^-1} / ||x||_M <= r / (sqrt(lambda_min(M)) ||x||_M), which
    is r / lambda_min(M) for ||x||_2 = 1 and r / sqrt(lambda_min(M)) for ||x||_M = 1.
  N: M = I + Pc/4 shares the eigenvectors X of Pc, X^-1 M^-1 = (I + Lambda/4)^-1 X^-1 with |1 + ac/4| >= 1, so Bauer-Fike gives
    |mu - mu_i| <= cond(X) r, cond(X) <= KAPPA.
  Z: A = P positive definite, M semi-definite: for the reversed pencil M x = theta A x, |theta - theta_i| <= theta r / a_min, hence
    |lambda - lambda_i| <= |lambda_i| r / a_min.
  H: M = diag(rho), rho >= 1, so ||M^-1|| <= 1 and |lambda - lambda_i| <= cond(X) r with X the eigenvectors of M^-1 A."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import eigs_gen_mirror as GM
from eigs_mirror import match, nearest, poisson_spectrum
from helpers import prepare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
SHAPE = (12, 11, 10)
KAPPA = 17.0  # tests/test_eigs_gpu.py: the eigenvector condition number of the convection x-factor


def run(A, M, sigma, nev, dtype=float, trans="N", inner="euclid"):
    """(lambda, X, r, log) of the mirror on the pencil (op(A), op(M)), F = SuperLU of A - sigma M"""
    n = A.shape[0]
    As = (A - sigma * M).tocsc().astype(dtype)
    lu = spla.splu(As)
    op = {"N": lambda B: B, "T": lambda B: B.T, "H": lambda B: B.conj().T}[trans]
    opM, opAs = op(M).tocsr().astype(dtype), op(As).tocsr()
    theta, X, log = GM.eigs_gen_mirror(lambda B: lu.solve(np.ascontiguousarray(B), trans=trans), opM, n, dtype, inner=inner, nev=nev, ncv=48, block=8, tol=TOL, maxrestart=30)
    mu = 1.0 / theta
    r = GM.m_residual(opAs, opM, X, mu)
    print(f"restarts {log['restarts']} solves {log['nsolves']} M products {log['nmprod']} replaced {log['replaced']} est {log['est'].max():.1e} resid {r.max():.1e}")
    assert log["nconv"] == len(theta) and log["restarts"] <= 9 and log["nmprod"] == log["nsolves"]
    if inner == "M":
        assert np.abs(X.conj().T @ (opM @ X) - np.eye(X.shape[1])).max() <= 1e-12
    else:
        assert np.allclose(np.linalg.norm(X, axis=0), 1.0, rtol=0, atol=1e-14)
    return (np.conj(sigma) if trans == "H" else sigma) + mu, X, r, log


@pytest.mark.parametrize("inner", ["euclid", "M"])
@pytest.mark.parametrize("sigma", [0.0, 0.9])
def test_mirror_S(sigma, inner):
    A, M, spec = GM.pencil_S(SHAPE)
    ref = np.sort(nearest(spec, sigma, 6))
    lam, X, r, _ = run(A, M, sigma, 6, inner=inner)
    assert np.abs(lam.imag).max() == 0.0
    o = np.argsort(lam.real)
    err = np.abs(lam.real[o] - ref)
    print("errors", err, "bound", r[o])
    assert np.all(err <= r[o] + 1e-12 * spla.norm(A, 1))  # lambda_min(M) >= 1 in both normalisations


def test_mirror_W():
    A, M, spec = GM.pencil_W(SHAPE)
    assert M.nnz > A.nnz
    ref = np.sort(nearest(spec, 0.0, 6))
    lam, X, r, _ = run(A, M, 0.0, 6)
    o = np.argsort(lam.real)
    assert np.all(np.abs(lam.real[o] - ref) <= r[o] + 1e-12 * spla.norm(A, 1))


@pytest.mark.parametrize("trans", ["N", "T"])
def test_mirror_N(trans):
    A, M, spec = GM.pencil_N(SHAPE)
    ref = nearest(spec, 0.7, 6)
    lam, X, r, _ = run(A, M, 0.7, 6, trans=trans)
    assert len(lam) == 6 and np.all(lam[0::2].imag > 0) and np.array_equal(lam[0::2], np.conj(lam[1::2]))
    assert match(lam, ref) <= KAPPA * r.max() + 1e-11
    lam5, _, r5, _ = run(A, M, 0.7, 5, trans=trans)
    assert len(lam5) == 6 and match(lam5, ref) <= KAPPA * r5.max() + 1e-11  # a pair is not split


def test_mirror_Z_singular_M():
    A, M, ref = GM.pencil_Z(SHAPE)
    assert np.sum(M.diagonal() == 0.0) == -(-A.shape[0] // 7)
    lam, X, r, log = run(A, M, 0.0, 6)
    a0 = poisson_spectrum(SHAPE)[0]
    o = np.argsort(lam.real)
    assert np.all(np.isfinite(lam)) and np.abs(lam.imag).max() == 0.0
    assert np.all(np.abs(lam.real[o] - ref) <= np.abs(ref) * r[o] / a0 + 1e-12)


@pytest.mark.parametrize("trans", ["N", "H"])
def test_mirror_H_complex(trans):
    A, M, ref, condX = GM.pencil_H()
    lam, X, r, _ = run(A, M, 0.0, 6, dtype=complex, trans=trans)
    lamA = np.conj(lam) if trans == "H" else lam  # the adjoint returns the eigenvalues of the pencil (A^H, M^H)
    print("cond(X)", condX, "match", match(lamA, ref))
    assert match(lamA, ref) <= condX * r.max() + 1e-11 * spla.norm(A, 1)


def test_mirror_identity_and_indefinite_M():
    A, M, spec = GM.pencil_S(SHAPE)
    n = A.shape[0]
    lu = spla.splu(A.tocsc())
    kw = dict(nev=6, ncv=48, block=8, tol=TOL, maxrestart=30)
    t0, X0, _ = GM.eigs_gen_mirror(lu.solve, None, n, float, **kw)
    for inner in ("euclid", "M"):  # M = I: the same steps on the same numbers
        t1, X1, _ = GM.eigs_gen_mirror(lu.solve, sp.identity(n, format="csr"), n, float, inner=inner, **kw)
        sgn = np.sign(np.sum(X0 * X1, axis=0))  # numpy's eig fixes no sign
        assert np.allclose(t0, t1, rtol=1e-13, atol=0) and np.allclose(X0, X1 * sgn, rtol=0, atol=1e-9)
    d = np.ones(n)
    d[5] = -1.0
    v0 = np.random.default_rng(0).standard_normal((n, 8))
    v0[:, 0] = 0.0
    v0[5, 0] = 1.0
    with pytest.raises(ValueError, match="positive definite"):
        GM.eigs_gen_mirror(lu.solve, sp.diags(d, format="csr"), n, float, inner="M", v0=v0, **kw)


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------
NEW = ["hs_eigs_gen_d", "hs_eigs_gen_z", "hs_eigs_gen_info"]
HOOKS = ["hsk_eigs_coldot_d", "hsk_eigs_coldot_z"]


def test_new_entry_points_are_declared_exported_and_bound(hs):
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    ktxt = open(os.path.join(ROOT, "include", "hs_kernels.h")).read()
    lib = hs._lib.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    for name in HOOKS:
        assert re.search(r"\bint\s+%s\s*\(" % name, ktxt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    assert list(lib.hs_eigs_gen_d.argtypes) == list(lib.hs_eigs_gen_z.argtypes) and len(lib.hs_eigs_gen_d.argtypes) == len(lib.hs_eigs_d.argtypes) + 4
    assert list(lib.hs_eigs_gen_d.argtypes[7:]) == list(lib.hs_eigs_d.argtypes[3:])  # M and inner sit between n and nev
    assert set(hs.eigs_gen_info()) == {"m_products", "m_columns", "m_bytes", "inner"}
    assert lib.hs_eigs_gen_info(None) == hs._lib.HS_ERR_ARGUMENT
    assert "hsk_eigs_gen_mprod_seconds" in hs._lib.EXPORTS and re.search(r"\bdouble\s+hsk_eigs_gen_mprod_seconds\s*\(", ktxt)
    assert lib.hsk_eigs_gen_mprod_seconds() >= 0.0
    assert set(hs.eigs_info()) == {"seconds", "block_solves", "column_applications", "restarts", "orth_passes", "replaced", "workspace_bytes", "ncv"}
    z = np.zeros(4)
    vp = z.ctypes.data_as(C.c_void_p)
    pf = z.ctypes.data_as(C.POINTER(C.c_double))
    bad_pair = (C.c_int * 2)(1, 0)  # half a pair
    for sfx in ("_d", "_z"):
        fn = getattr(lib, "hsk_eigs_coldot" + sfx)
        assert fn(0, 1, vp, 1, vp, 1, None, pf) == hs._lib.HS_ERR_ARGUMENT
        assert fn(2, 300, vp, 2, vp, 2, None, pf) == hs._lib.HS_ERR_ARGUMENT
        assert fn(2, 1, vp, 1, vp, 2, None, pf) == hs._lib.HS_ERR_ARGUMENT
        assert fn(2, 2, vp, 2, vp, 2, bad_pair, pf) == hs._lib.HS_ERR_ARGUMENT
    assert not z.any()


def test_python_argument_checks_need_no_device(hs):
    n = 400
    F = hs.FactorNode(None, np.float64, n, None)  # no handle: every check below comes before the library is called
    I = sp.identity(n, format="csc")
    with pytest.raises(ValueError, match="inner"):
        hs.eigs(F, M=I, inner="A")
    with pytest.raises(ValueError, match="inner"):
        hs.eigs(F, inner=1)
    with pytest.raises(TypeError, match="scipy.sparse"):
        hs.eigs(F, M=np.eye(n))
    with pytest.raises(hs.DimensionMismatch):
        hs.eigs(F, M=sp.identity(n + 1, format="csc"))
    with pytest.raises(hs.DimensionMismatch):
        hs.eigs(F, M=sp.csc_matrix((n, n + 1)))
    with pytest.raises(TypeError, match="ComplexF64 M"):
        hs.eigs(F, M=(1j * I).tocsc())
    with pytest.raises(TypeError, match="ComplexF64 M"):
        hs.eigs(hs.transpose(F), M=(1j * I).tocsc(), inner="M")
    with pytest.raises(ValueError, match="nev"):  # the checks of the standard call are still made
        hs.eigs(F, M=I, nev=0)


def _call(lib, h, n, colptr, rowval, nzval, inner=0, sfx="_d", nev=2, ncv=8, block=2):
    lam, res, est = np.full(2 * (nev + 1), 42.0), np.full(nev + 1, 42.0), np.full(nev + 1, 42.0)
    X = np.full((n, nev + 1), 42.0, order="F")
    nout, nconv = C.c_int64(-7), C.c_int64(-7)
    pf = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None  # noqa: E731
    st = getattr(lib, "hs_eigs_gen" + sfx)(h, 0, n, pi(colptr), pi(rowval), nzval.ctypes.data_as(C.c_void_p) if nzval is not None else None, inner, nev, ncv, block, 0.0, 0.0,
                                           1e-10, 5, None, n, 0, 0, pf(lam), X.ctypes.data_as(C.c_void_p), n, pf(res), pf(est), C.byref(nout), C.byref(nconv), None)
    assert nout.value == -7 and nconv.value == -7 and np.all(lam == 42.0) and np.all(res == 42.0) and np.all(est == 42.0) and np.all(X == 42.0)
    return st


def test_malformed_M_is_refused_before_the_handle_is(hs):
    E = hs._lib
    lib = E.lib()
    P = prepare(hs, (20, 12), kind="convdiff", nmax=10)
    n = P["A"].shape[0]
    M = (sp.identity(n) + P["A"] / 4).tocsc()
    M.sort_indices()
    cp, rv, nz = M.indptr.astype(np.int64) + 1, M.indices.astype(np.int64) + 1, M.data.astype(np.float64)
    rv_bad = rv.copy()
    rv_bad[len(rv) // 2] = n + 1
    cp_bad = cp.copy()
    cp_bad[3] = cp_bad[2] - 1
    for nranks, own in ((2, E.HS_ERR_UNSUPPORTED), (1, E.HS_ERR_ARGUMENT)):  # two ranks; one rank, but a plan holds no factorization
        h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=nranks) if nranks > 1 else hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"])
        try:
            assert _call(lib, h, n, cp, rv, nz) == own  # a well-formed M: the handle's own refusal, as hs_eigs_d
            if nranks > 1:
                assert "2 ranks" in lib.hs_last_error().decode()
            assert _call(lib, h, n, None, None, None, inner=1) == own  # M = NULL with inner = 1 is the standard call
            for args, word in (((cp - 1, rv, nz), "1-based"), ((cp, rv_bad, nz), "mrowval"), ((cp_bad, rv, nz), "mcolptr"), ((cp, rv, None), "all be given"),
                               ((cp, None, None), "all be given"), ((None, rv, nz), "all be given")):
                assert _call(lib, h, n, *args) == E.HS_ERR_ARGUMENT
                assert word in lib.hs_last_error().decode(), lib.hs_last_error().decode()
            for inner in (2, -1):
                assert _call(lib, h, n, cp, rv, nz, inner=inner) == E.HS_ERR_ARGUMENT
                assert "inner" in lib.hs_last_error().decode()
            assert _call(lib, h, n, cp, rv, nz, nev=0) == E.HS_ERR_ARGUMENT  # the checks of hs_eigs_* are all still there
            assert _call(lib, h, n + 1, cp, rv, nz) == E.HS_ERR_DIMENSION
            assert _call(lib, h, n, cp, rv, nz, sfx="_z") == E.HS_ERR_DIMENSION
        finally:
            lib.hs_free(h)
    assert _call(lib, None, n, cp, rv, nz) == E.HS_ERR_ARGUMENT
