"""Shift-invert eigenpairs from stored factors, on the CPU: the NumPy statement of the driver's loop (tests/eigs_mirror.py, SuperLU as the
solve) against analytic spectra and numpy.linalg.eigvals, the hand-written dense eigen-solver of the host part (csrc/hs_small_eig.h through
hsk_small_eig_z), the new entry points of the C ABI, the Python argument checks and the refusal of a plan over several ranks.  The device
implementation (csrc/hs_eigs.hip, csrc/kernels_eigs.hip) is checked in tests/test_eigs_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import eigs_mirror as EM
from eigs_mirror import convection, convection_spectrum, match, nearest, poisson, poisson_spectrum
from helpers import prepare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def run_mirror(A, sigma, nev, dtype=float, trans="N", **kw):
    n = A.shape[0]
    lu = spla.splu((A - sigma * sp.identity(n)).tocsc().astype(dtype))
    kw.setdefault("ncv", 48)
    kw.setdefault("block", 8)
    theta, X, log = EM.eigs_mirror(lambda B: lu.solve(np.ascontiguousarray(B), trans=trans), n, dtype, nev=nev, tol=TOL, maxrestart=30, **kw)
    lam = sigma + 1.0 / theta
    print(f"restarts {log['restarts']} solves {log['nsolves']} replaced {log['replaced']} est {log['est'].max():.1e}")
    assert log["nconv"] == len(lam) and log["restarts"] <= 10
    return lam, X, log


SHAPE = (12, 11, 10)


def test_mirror_poisson_and_shift():
    A, spec = poisson(SHAPE), poisson_spectrum(SHAPE)
    lam, X, _ = run_mirror(A, 0.0, 6)
    assert match(lam, spec[:6]) <= 1e-11 and np.abs(lam.imag).max() == 0.0
    assert np.linalg.norm(A @ X - X * lam, axis=0).max() <= 2 * TOL * np.sqrt(spla.norm(A, 1) * spla.norm(A, np.inf))
    lam, X, _ = run_mirror(A, 3.1, 6)
    assert match(lam, nearest(spec, 3.1, 6)) <= 1e-11
    lam, _, _ = run_mirror(A, 0.0, 10, ncv=64, block=16)
    assert match(lam, spec[:10]) <= 1e-11


def test_mirror_cube_multiplicities():
    A, spec = poisson((10, 10, 10)), poisson_spectrum((10, 10, 10))
    lam, X, _ = run_mirror(A, 0.0, 7)  # multiplicities 1 + 3 + 3
    assert np.abs(np.sort(lam.real) - spec[:7]).max() <= 1e-11
    assert np.linalg.matrix_rank(X, 1e-8) == 7


@pytest.mark.parametrize("trans", ["N", "T"])
def test_mirror_real_nonsymmetric_pairs(trans):
    A, spec = convection(SHAPE, 8.0), convection_spectrum(SHAPE, 8.0)
    ref = nearest(spec, 2.0, 6)
    lam, X, _ = run_mirror(A, 2.0, 6, trans=trans)
    assert len(lam) == 6 and match(lam, ref) <= 1e-9
    assert np.all(lam[0::2].imag > 0) and np.array_equal(lam[0::2], np.conj(lam[1::2]))  # pairs, the positive imaginary part first
    lam5, _, _ = run_mirror(A, 2.0, 5, trans=trans)
    assert len(lam5) == 6 and match(lam5, ref) <= 1e-9  # a pair is not split
    op = A if trans == "N" else A.T
    assert np.linalg.norm(op @ X - X * lam, axis=0).max() <= 1e-8


@pytest.mark.parametrize("trans", ["N", "T", "H"])
def test_mirror_complex(trans, hs):
    A = hs.problems.grid_matrix((10, 9, 8), "helmholtz")
    w = np.linalg.eigvals(A.toarray())
    ref = nearest(w, 0.0, 6)
    lam, X, _ = run_mirror(A, 0.0, 6, dtype=complex, trans=trans)
    assert match(np.conj(lam) if trans == "H" else lam, ref) <= 1e-10


def test_mirror_deflation_replaces_columns():
    A, spec = poisson(SHAPE), poisson_spectrum(SHAPE)
    nx, ny, nz = SHAPE

    def sine(kx, ky, kz):
        v = np.kron(np.kron(np.sin(kz * np.pi * np.arange(1, nz + 1) / (nz + 1)), np.sin(ky * np.pi * np.arange(1, ny + 1) / (ny + 1))),
                    np.sin(kx * np.pi * np.arange(1, nx + 1) / (nx + 1)))
        return v / np.linalg.norm(v)

    v0 = np.random.default_rng(5).standard_normal((A.shape[0], 4))
    v0[:, 0], v0[:, 1] = sine(1, 1, 1), sine(2, 1, 1)
    lam, _, log = run_mirror(A, 0.0, 6, ncv=48, block=4, v0=v0)
    assert match(lam, spec[:6]) <= 1e-11 and log["replaced"] >= 1


def test_mirror_chol_inv():
    rng = np.random.default_rng(2)
    W = rng.standard_normal((50, 9)) + 1j * rng.standard_normal((50, 9))
    G = W.conj().T @ W
    R, Ri, bad = EM.chol_inv(G)
    assert bad == -1 and np.allclose(R.conj().T @ R, G, rtol=0, atol=1e-12 * np.abs(G).max()) and np.allclose(R @ Ri, np.eye(9), atol=1e-12)
    W[:, 3] = 0.0
    assert EM.chol_inv(W.conj().T @ W)[2] == 3


# ---- the dense eigen-solver of the host part -------------------------------------------------------------------------------------------
def small_eig(hs, H):
    m = H.shape[0]
    Hf = np.asfortranarray(H, dtype=np.complex128)
    H0 = Hf.copy()
    w = np.zeros(m, dtype=np.complex128)
    Y = np.zeros((m, m), dtype=np.complex128, order="F")
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    hs._lib.check(hs._lib.lib().hsk_small_eig_z(m, vp(Hf), m, vp(w), vp(Y), m))
    assert np.array_equal(Hf, H0)
    return w, Y


def check_small_eig(hs, H):
    w, Y = small_eig(hs, H)
    nh = np.linalg.norm(H)
    res = np.linalg.norm(H @ Y - Y * w)
    print(f"m = {H.shape[0]}: residual {res:.2e}, bound {1e-12 * nh * np.linalg.norm(Y):.2e}")
    assert res <= 1e-12 * nh * np.linalg.norm(Y)
    assert np.allclose(np.linalg.norm(Y, axis=0), 1.0, atol=1e-12)
    ref = np.linalg.eigvals(H)
    return w, Y, ref


@pytest.mark.parametrize("m", [1, 2, 7, 48, 200])
def test_small_eig_random_complex(hs, m):
    rng = np.random.default_rng(m)
    H = rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))
    w, Y, ref = check_small_eig(hs, H)
    assert match(w, ref) <= 1e-10 * np.linalg.norm(H)  # random matrices: well-conditioned eigenvalues
    assert np.linalg.cond(Y) < 1e8


@pytest.mark.parametrize("m", [2, 7, 48, 200])
def test_small_eig_real_with_conjugate_pairs(hs, m):
    rng = np.random.default_rng(100 + m)
    H = rng.standard_normal((m, m)) if m > 2 else np.array([[1.0, -2.0], [3.0, 1.0]])  # 1 +- i sqrt(6)
    w, Y, ref = check_small_eig(hs, H)
    assert match(w, ref) <= 1e-10 * np.linalg.norm(H)
    cp = w[np.abs(w.imag) > 1e-8]
    assert len(cp) >= 2 and match(cp, np.conj(cp)) <= 1e-10 * np.linalg.norm(H)  # the pairs come out as pairs


def test_small_eig_triple_eigenvalue_and_triangular(hs):
    rng = np.random.default_rng(9)
    Q = np.linalg.qr(rng.standard_normal((7, 7)) + 1j * rng.standard_normal((7, 7)))[0]
    d = np.array([2.0, 2.0, 2.0, -1.0, 0.5j, 3.0, 1.0 + 1.0j])
    H = Q @ np.diag(d) @ Q.conj().T  # a semisimple triple eigenvalue
    w, Y, _ = check_small_eig(hs, H)
    assert match(w, d) <= 1e-12 and np.sum(np.abs(w - 2.0) < 1e-12) == 3
    J = np.diag(d) + np.diag([1.0, 1.0, 0, 0, 0, 0], 1)  # the same triple eigenvalue in one Jordan block: defective
    check_small_eig(hs, Q @ J @ Q.conj().T)
    T = np.triu(rng.standard_normal((48, 48)) + 1j * rng.standard_normal((48, 48)))  # already triangular: no sweep changes it
    w, Y, _ = check_small_eig(hs, T)
    assert np.array_equal(w, np.diag(T))
    check_small_eig(hs, np.zeros((5, 5)))
    check_small_eig(hs, np.eye(6))


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------
NEW = ["hs_eigs_d", "hs_eigs_z", "hs_eigs_info"]
HOOKS = ["hsk_eigs_rotate_d", "hsk_eigs_rotate_z", "hsk_eigs_chol_inv_d", "hsk_eigs_chol_inv_z", "hsk_small_eig_z"]


def _call(lib, sfx, h, n, nev=2, ncv=8, block=2, lam=None, X=None, sigma_im=0.0, outs=True):
    res, est = np.zeros(nev + 1), np.zeros(nev + 1)
    nout, nconv = C.c_int64(-7), C.c_int64(-7)
    pf = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    st = getattr(lib, "hs_eigs" + sfx)(h, 0, n, nev, ncv, block, 0.0, sigma_im, 1e-10, 5, None, n, 0, 0, pf(lam) if lam is not None else None,
                                        X.ctypes.data_as(C.c_void_p) if X is not None else None, n, pf(res) if outs else None, pf(est), C.byref(nout), C.byref(nconv), None)
    assert nout.value == -7 and nconv.value == -7 and not res.any() and not est.any()
    return st


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
    assert list(lib.hs_eigs_d.argtypes) == list(lib.hs_eigs_z.argtypes) and lib.hs_eigs_d.argtypes[1] is C.c_int
    assert callable(hs.eigs) and callable(hs.eigs_info) and issubclass(hs.NoConvergence, ArithmeticError)
    assert set(hs.eigs_info()) == {"seconds", "block_solves", "column_applications", "restarts", "orth_passes", "replaced", "workspace_bytes", "ncv"}
    assert lib.hs_eigs_info(None) == hs._lib.HS_ERR_ARGUMENT
    # a null handle is refused without a device, nothing written
    lam = np.full(6, 42.0)
    for sfx in ("_d", "_z"):
        assert _call(lib, sfx, None, 20, lam=lam) == hs._lib.HS_ERR_ARGUMENT
    assert np.all(lam == 42.0)
    z = np.zeros(4)
    vp = z.ctypes.data_as(C.c_void_p)
    info = C.c_int(5)
    for sfx in ("_d", "_z"):
        assert getattr(lib, "hsk_eigs_rotate" + sfx)(2, 300, 1, vp, 2, vp, 300, 0, vp, 2) == hs._lib.HS_ERR_ARGUMENT
        assert getattr(lib, "hsk_eigs_rotate" + sfx)(2, 1, 2, vp, 2, vp, 1, 0, vp, 2) == hs._lib.HS_ERR_ARGUMENT
        assert getattr(lib, "hsk_eigs_chol_inv" + sfx)(65, vp, 65, vp, vp, C.byref(info)) == hs._lib.HS_ERR_ARGUMENT
    assert lib.hsk_small_eig_z(257, vp, 257, vp, vp, 257) == hs._lib.HS_ERR_ARGUMENT
    assert not z.any() and info.value == 5


def test_python_argument_checks_need_no_device(hs):
    n = 400
    F = hs.FactorNode(None, np.float64, n, None)  # no handle: every check below comes before the library is called
    Fz = hs.FactorNode(None, np.complex128, n, None)
    with pytest.raises(TypeError):
        hs.eigs(np.eye(4))
    with pytest.raises(ValueError, match="complex shift"):
        hs.eigs(F, sigma=1.0 + 2.0j)
    with pytest.raises(ValueError, match="complex shift"):
        hs.eigs(hs.transpose(F), sigma=2.0j)
    with pytest.raises(ValueError, match="nev"):
        hs.eigs(F, nev=0)
    with pytest.raises(ValueError, match="exceeds the limit of 256"):
        hs.eigs(F, ncv=250, block=8)
    with pytest.raises(ValueError, match="exceeds the limit of 256"):
        hs.eigs(Fz, ncv=250, block=8, sigma=1j)
    with pytest.raises(ValueError, match="nev \\+ block"):
        hs.eigs(F, nev=6, ncv=12, block=8)
    with pytest.raises(ValueError, match="n = 40 < ncv \\+ block"):
        hs.eigs(hs.FactorNode(None, np.float64, 40, None), nev=6, ncv=48, block=8)
    with pytest.raises(ValueError, match="block"):
        hs.eigs(F, block=65)
    with pytest.raises(hs.DimensionMismatch):
        hs.eigs(F, block=8, v0=np.zeros((n, 4)))
    with pytest.raises(hs.DimensionMismatch):
        hs.eigs(F, v0=np.zeros((n + 1, 8)))
    with pytest.raises(TypeError):
        hs.eigs(F, v0=np.zeros((n, 8), dtype=complex))
    e = hs.NoConvergence("x", partial=(1, 2))
    assert e.partial == (1, 2)


def test_refusals_from_host_side_plans(hs):
    """The argument checks of the C entry points, and what the block solve refuses, named before any device work with nothing written."""
    E = hs._lib
    lib = E.lib()
    P = prepare(hs, (20, 12), kind="convdiff", nmax=10)
    n = P["A"].shape[0]
    lam = np.full(8, 42.0)
    X = np.full((n, 3), 42.0, order="F")
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=2)
    try:
        assert _call(lib, "_d", h, n, lam=lam, X=X) == E.HS_ERR_UNSUPPORTED
        assert "2 ranks" in lib.hs_last_error().decode()
        # the argument checks come first
        assert _call(lib, "_d", h, n, nev=0, lam=lam, X=X) == E.HS_ERR_ARGUMENT
        assert _call(lib, "_d", h, n, ncv=250, block=8, lam=lam, X=X) == E.HS_ERR_ARGUMENT
        assert _call(lib, "_d", h, n, ncv=40, block=65, lam=lam, X=X) == E.HS_ERR_ARGUMENT
        assert _call(lib, "_d", h, n, nev=7, ncv=8, block=2, lam=lam, X=X) == E.HS_ERR_ARGUMENT
        assert _call(lib, "_d", h, n, ncv=200, block=50, lam=lam, X=X) == E.HS_ERR_ARGUMENT  # n = 240 < 250
        assert _call(lib, "_d", h, n, lam=None, X=X) == E.HS_ERR_ARGUMENT
        assert _call(lib, "_d", h, n, lam=lam, X=X, outs=False) == E.HS_ERR_ARGUMENT
        assert _call(lib, "_d", h, n, lam=lam, X=X, sigma_im=1.0) == E.HS_ERR_ARGUMENT
        assert _call(lib, "_d", h, n + 1, lam=lam, X=X) == E.HS_ERR_DIMENSION
        assert _call(lib, "_z", h, n, lam=lam, X=X) == E.HS_ERR_DIMENSION
    finally:
        lib.hs_free(h)
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"])  # one rank, but a plan holds no factorization
    try:
        assert _call(lib, "_d", h, n, lam=lam, X=X) == E.HS_ERR_ARGUMENT
    finally:
        lib.hs_free(h)
    assert np.all(lam == 42.0) and np.all(X == 42.0)
