"""Generalized shift-invert eigenpairs A x = lambda M x from the stored factors of A - sigma M (hs.eigs(..., M=, inner=), hs_eigs_gen_*,
csrc/hs_eigs.hip) on the MI355X: the column-dot kernel alone, then the driver on the pencils of tests/eigs_gen_mirror.py.  Every driver case
uses tol = 1e-10, block = 8, ncv = 48, maxrestart = 30 and asserts restarts <= 30 (the NumPy mirror of tests/test_eigs_gen_host.py needs at
most 9).  Matrices are built in the grid's own ordering and permuted with the nested-dissection permutation of helpers.prepare; M is passed
in that factored ordering.

Residual bound: resid_c = ||op(A_s) x - mu op(M) x||_2 <= 2 tol sqrt(||A_s||_1 ||A_s||_inf) for ||x||_2 = 1, from
A_s x - mu M x = -mu A_s (C x - theta x), C = F^-1 M, |mu| ||C x - theta x||_2 = est <= tol; with inner = "M" est is an M-norm, and
||v||_2 <= ||v||_M / sqrt(lambda_min(M)).  The eigenvalue bounds are derived in the docstring of tests/test_eigs_gen_host.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import eigs_gen_mirror as GM
from eigs_mirror import match, nearest, poisson, poisson_spectrum
from helpers import prepare

pytestmark = pytest.mark.gpu

TOL = 1e-10
KW = dict(tol=TOL, block=8, ncv=48, maxrestart=30)
SHAPE = (12, 11, 10)
KAPPA = 17.0  # tests/test_eigs_gpu.py: the eigenvector condition number of the convection x-factor
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for v in _CACHE.values():
        v["F"].free()
    _CACHE.clear()


def _pencil(hs, key, shape, build, sigma=0.0, nmax=100, **opts):
    """A, M (factored ordering), A_s = A - sigma M, its factorization F, perm and whatever else build(shape) returns after (A, M)"""
    if key not in _CACHE:
        P = prepare(hs, shape, nmax=nmax)
        perm = P["perm"]
        A, M, *rest = build(shape)
        A, M = A[perm - 1][:, perm - 1].tocsc(), M[perm - 1][:, perm - 1].tocsc()
        As = (A - sigma * M).tocsc()
        As.sort_indices()
        _CACHE[key] = dict(A=A, M=M, As=As, F=hs.factor(As, P["nd"], P["nd_loc"], **(opts or dict(swlevel=0))), perm=perm, rest=rest)
    return _CACHE[key]


def _resid_bound(As):
    return 2.0 * TOL * np.sqrt(spla.norm(As, 1) * spla.norm(As, np.inf))


def _run(hs, F, M, inner="euclid", **kw):
    lam, X, log = hs.eigs(F, log=True, M=M, inner=inner, **{**KW, **kw})
    print(f"{inner}: restarts {log['restarts']} solves {log['nsolves']} M products {log['nmprod']} replaced {log['replaced']} resid {log['resid'].max():.2e} "
          f"est {log['est'].max():.2e} {log['seconds'] * 1e3:.1f} ms")
    assert log["restarts"] <= 30 and log["nconv"] == len(lam)
    return lam, X, log


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- 1. the column-dot kernel ----------------------------------------------------------------------------------------------------------------
def _coldot(hs, X, Y, pair=None):
    cplx = np.iscomplexobj(X)
    n, nc = X.shape
    Xf, Yf = np.asfortranarray(X), np.asfortranarray(Y, dtype=X.dtype)
    d = np.full(nc, np.nan)
    pr = (C.c_int * nc)(*pair) if pair is not None else None
    hs._lib.check(getattr(hs._lib.lib(), "hsk_eigs_coldot" + ("_z" if cplx else "_d"))(n, nc, _vp(Xf), n, _vp(Yf), n, pr, d.ctypes.data_as(hs._lib.p_f64)))
    return d


def _coldot_ref(X, Y, pair):
    d = np.real(np.sum(X.conj() * Y, axis=0))
    for c, pc in enumerate(pair or []):
        if pc == 1:
            d[c] = d[c + 1] = d[c] + d[c + 1]
    return d


def _ints(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, shape).astype(float)
    return X + 1j * rng.integers(-3, 4, shape) if cplx else X


PAIRS = {1: [0], 3: [1, -1, 0], 7: [0, 1, -1, 0, 0, 1, -1]}


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n", [1, 63, 2049, 4097])
def test_coldot_is_exact_on_integers(hs, n, cplx):
    for nc in (1, 3, 7):
        X, Y = _ints((n, nc), cplx, 3 * n + nc), _ints((n, nc), cplx, 5 * n + nc)
        assert np.array_equal(_coldot(hs, X, Y), _coldot_ref(X, Y, None)), (n, nc)
        if not cplx:  # the pair layout: a Float64 pair shares the sum over both columns
            assert np.array_equal(_coldot(hs, X, Y, PAIRS[nc]), _coldot_ref(X, Y, PAIRS[nc])), (n, nc, "pairs")
        assert np.array_equal(_coldot(hs, X, X), np.real(np.sum(X.conj() * X, axis=0)))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_coldot_slab_bits_do_not_depend_on_the_rows_behind(hs, cplx):
    """rows past a slab boundary set to zero add exact zeros in slab order: the figure must be that of the row prefix alone, bit for bit"""
    rng = np.random.default_rng(8)
    X = rng.standard_normal((4097, 3)) + (1j * rng.standard_normal((4097, 3)) if cplx else 0.0)
    Y = rng.standard_normal((4097, 3)) + (1j * rng.standard_normal((4097, 3)) if cplx else 0.0)
    full = _coldot(hs, X, Y)
    ref = np.real(np.sum(X.conj() * Y, axis=0))
    assert np.allclose(full, ref, rtol=0, atol=4097 * 2.0 ** -52 * np.sum(np.abs(X) * np.abs(Y), axis=0).max())
    for rows in (2048, 4096):
        Xz = X.copy()
        Xz[rows:] = 0.0
        assert np.array_equal(_coldot(hs, Xz, Y), _coldot(hs, X[:rows], Y[:rows])), rows
    assert np.array_equal(_coldot(hs, X, Y), full)


# ---- 2. M = I is the standard call, bit for bit ------------------------------------------------------------------------------------------------
def test_identity_M_reproduces_the_standard_call_bitwise(hs):
    """T = 1.0 * V from a zero accumulator is V, MW = W, and x^H (I x) is summed as ||x||^2 is: both modes must return the standard bits"""
    P = _pencil(hs, "poisson3.1", SHAPE, lambda s: (poisson(s), sp.identity(int(np.prod(s)), format="csc")), sigma=3.1)
    n = P["A"].shape[0]
    lam0, X0, log0 = hs.eigs(P["F"], nev=6, sigma=3.1, log=True, **KW)
    assert log0["nmprod"] == 0
    for inner in ("euclid", "M"):
        lam, X, log = _run(hs, P["F"], sp.identity(n), inner, nev=6, sigma=3.1)
        assert np.array_equal(lam, lam0) and np.array_equal(X, X0) and np.array_equal(log["resid"], log0["resid"]) and np.array_equal(log["est"], log0["est"]), inner
        assert log["restarts"] == log0["restarts"] and log["nsolves"] == log0["nsolves"] and hs.eigs_gen_info()["inner"] == inner


# ---- 3, 5. Hermitian definite pencils ---------------------------------------------------------------------------------------------------------
def _check_hermitian(hs, P, sigma, inner, ref):
    A, M, As, F = P["A"], P["M"], P["As"], P["F"]
    lam, X, log = _run(hs, F, M, inner, nev=6, sigma=sigma)
    assert lam.dtype == np.float64 and X.dtype == np.float64 and lam.shape == (6,) and X.shape == (A.shape[0], 6)
    assert np.array_equal(np.argsort(np.abs(lam - sigma), kind="stable"), np.arange(6))  # nearest first
    o = np.argsort(lam)
    err, res = np.abs(lam[o] - ref), log["resid"][o]
    print("errors", err, "resid", res, "bound", _resid_bound(As))
    assert np.all(err <= res + 1e-12 * spla.norm(A, 1))  # res / lambda_min(M) and res / sqrt(lambda_min(M)) with lambda_min(M) = 1
    assert np.all(res <= _resid_bound(As))
    assert np.allclose(GM.m_residual(As, M, X, lam - sigma), log["resid"], rtol=0, atol=1e-13 * spla.norm(A, 1))  # the reported residuals are the true ones
    if inner == "M":
        assert np.abs(X.T @ (M @ X) - np.eye(6)).max() <= 1e-10
    else:
        assert np.allclose(np.linalg.norm(X, axis=0), 1.0, rtol=0, atol=1e-12)
    lam2, X2, log2 = _run(hs, F, M, inner, nev=6, sigma=sigma)
    assert np.array_equal(lam, lam2) and np.array_equal(X, X2) and np.array_equal(log["resid"], log2["resid"]) and np.array_equal(log["est"], log2["est"])


@pytest.mark.parametrize("inner", ["euclid", "M"])
@pytest.mark.parametrize("sigma", [0.0, 0.9])
def test_S_hermitian_definite_pencil(hs, sigma, inner):
    P = _pencil(hs, ("S", sigma), SHAPE, GM.pencil_S, sigma=sigma)
    _check_hermitian(hs, P, sigma, inner, np.sort(nearest(P["rest"][0], sigma, 6)))


def test_W_M_wider_than_the_pattern_of_A(hs):
    P = _pencil(hs, "W", SHAPE, GM.pencil_W)
    assert P["M"].nnz > P["A"].nnz
    _check_hermitian(hs, P, 0.0, "euclid", np.sort(nearest(P["rest"][0], 0.0, 6)))


# ---- 4. multiple eigenvalues ---------------------------------------------------------------------------------------------------------------
def test_cube_multiplicities_in_the_M_inner_product(hs):
    shape = (10, 10, 10)
    P = _pencil(hs, "cube", shape, GM.pencil_S)
    lam, X, log = _run(hs, P["F"], P["M"], "M", nev=7)  # multiplicities 1 + 3 + 3
    ref = P["rest"][0][:7]
    assert np.all(np.abs(np.sort(lam) - ref) <= log["resid"].max() + 1e-12 * spla.norm(P["A"], 1))
    assert np.all(log["resid"] <= _resid_bound(P["As"]))
    assert np.linalg.matrix_rank(X, 1e-8) == 7
    # x^T M x = 1 for every vector; inside a multiple eigenvalue the vectors span the eigenspace and need not be M-orthogonal to each other
    assert np.abs(np.sum(X * (P["M"] @ X), axis=0) - 1.0).max() <= 1e-10


# ---- 6. real non-symmetric, right and left -----------------------------------------------------------------------------------------------------
def _pairs_ok(lam):
    return np.all(lam[0::2].imag > 0) and np.array_equal(lam[0::2], np.conj(lam[1::2]))


def test_N_real_nonsymmetric_pairs_right_and_left(hs):
    sigma = 0.7
    P = _pencil(hs, "N", SHAPE, GM.pencil_N, sigma=sigma)
    A, M, As, F = P["A"], P["M"], P["As"], P["F"]
    ref = nearest(P["rest"][0], sigma, 6)
    lam, X, log = _run(hs, F, M, nev=6, sigma=sigma)
    assert lam.dtype == np.complex128 and X.dtype == np.complex128 and len(lam) == 6 and _pairs_ok(lam)
    d = np.abs(lam[:, None] - ref[None, :])
    print("errors", d.min(axis=1), "resid", log["resid"])
    assert np.all(d.min(axis=1) <= KAPPA * log["resid"] + 1e-11) and match(lam, ref) <= KAPPA * log["resid"].max() + 1e-11
    assert np.all(log["resid"] <= _resid_bound(As)) and np.array_equal(log["resid"][0::2], log["resid"][1::2])
    assert np.allclose(np.linalg.norm(X, axis=0), 1.0, rtol=0, atol=1e-12)
    assert np.allclose(GM.m_residual(As, M, X, lam - sigma), log["resid"], rtol=0, atol=1e-13 * spla.norm(A, 1))
    lam5, X5, log5 = _run(hs, F, M, nev=5, sigma=sigma)  # a pair is not split
    assert len(lam5) == 6 and X5.shape[1] == 6 and _pairs_ok(lam5)
    assert match(lam5, ref) <= KAPPA * log5["resid"].max() + 1e-11
    lamT, Y, logT = _run(hs, hs.transpose(F), M, nev=6, sigma=sigma)  # the pencil (A^T, M^T): y^T A = lambda y^T M
    assert len(lamT) == 6 and _pairs_ok(lamT)
    assert match(lamT, ref) <= KAPPA * logT["resid"].max() + 1e-11 and match(lamT, lam) <= KAPPA * (logT["resid"].max() + log["resid"].max()) + 2e-11
    assert np.all(logT["resid"] <= _resid_bound(As))
    rT = GM.m_residual(As.T.tocsr(), M.T.tocsr(), Y, lamT - sigma)  # y^T A_s = mu y^T M
    assert np.all(rT <= _resid_bound(As)) and np.allclose(rT, logT["resid"], rtol=0, atol=1e-13 * spla.norm(A, 1))


# ---- 7. a singular M ---------------------------------------------------------------------------------------------------------------------------
def test_Z_singular_M_returns_finite_eigenvalues_only(hs):
    P = _pencil(hs, "Z", SHAPE, GM.pencil_Z)
    A, M, As, F = P["A"], P["M"], P["As"], P["F"]
    ref = P["rest"][0]
    assert np.sum(M.diagonal() == 0.0) >= A.shape[0] // 7
    lam, X, log = _run(hs, F, M, nev=6)
    print("replaced", log["replaced"])
    a0 = poisson_spectrum(SHAPE)[0]
    o = np.argsort(lam)
    err = np.abs(lam[o] - ref)
    print("errors", err, "bound", np.abs(ref) * log["resid"][o] / a0)
    assert lam.dtype == np.float64 and np.all(np.isfinite(lam)) and np.all(np.isfinite(X))
    assert np.all(err <= np.abs(ref) * log["resid"][o] / a0 + 1e-12)
    assert np.all(log["resid"] <= _resid_bound(As))
    assert np.allclose(GM.m_residual(As, M, X, lam), log["resid"], rtol=0, atol=1e-13 * spla.norm(A, 1))


# ---- 8. ComplexF64, right and adjoint ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["plain", "adjoint"])
def test_H_complex_pencil(hs, which):
    P = _pencil(hs, "H", (10, 9, 8), lambda s: GM.pencil_H(s))
    A, M, As, F = P["A"], P["M"], P["As"], P["F"]
    ref, condX = P["rest"]
    lam, X, log = _run(hs, F if which == "plain" else hs.adjoint(F), M, nev=6)
    assert lam.dtype == np.complex128 and X.dtype == np.complex128
    lamA = np.conj(lam) if which == "adjoint" else lam  # the adjoint returns the eigenvalues of the pencil (A^H, M^H)
    print("match", match(lamA, ref), "resid", log["resid"], "cond(X_ref)", condX)
    assert match(lamA, ref) <= condX * log["resid"].max() + 1e-11 * spla.norm(A, 1)
    assert np.all(log["resid"] <= _resid_bound(As))
    opA, opM = (As.conj().T.tocsr(), M.conj().T.tocsr()) if which == "adjoint" else (As, M)
    assert np.allclose(GM.m_residual(opA, opM, X, lam), log["resid"], rtol=0, atol=1e-13 * spla.norm(A, 1))
    assert np.allclose(np.linalg.norm(X, axis=0), 1.0, rtol=0, atol=1e-12)


# ---- 9. a compressed handle ---------------------------------------------------------------------------------------------------------------
def _sine(shape, k, perm):
    f = [np.sin(kk * np.pi * np.arange(1, m + 1) / (m + 1)) for kk, m in zip(k, shape)]
    v = np.kron(np.kron(f[2], f[1]), f[0])
    return (v / np.linalg.norm(v))[perm - 1]


def test_compressed_handle_within_its_own_accuracy(hs):
    """d = max_c ||z_c - F^-1 (A_s z_c)||_2 over the analytic unit eigenvectors of the wanted pairs (those of P, shared by M = I + P/4) is what
    the compressed factors are off by; to first order theta = 1 / lambda moves by d theta, so |lam_c - ref_c| <= d |ref_c| (+ second order:
    the factor 10), as in tests/test_eigs_gpu.py."""
    shape = (24, 22, 20)
    P = _pencil(hs, "compressed", shape, GM.pencil_S, nmax=300, swlevel=2, swsize=8, atol=1e-6, rtol=1e-6)
    A, M, F, perm = P["A"], P["M"], P["F"], P["perm"]
    assert hs.maxrank(F) > 0
    idx = [(kx, ky, kz) for kz in range(1, 4) for ky in range(1, 4) for kx in range(1, 4)]
    val = lambda k: sum(2 - 2 * np.cos(kk * np.pi / (m + 1)) for kk, m in zip(k, shape))  # noqa: E731
    idx.sort(key=val)
    a = np.array([val(k) for k in idx[:6]])
    ref = a / (1 + a / 4)
    assert np.allclose(ref, P["rest"][0][:6], rtol=0, atol=1e-13)
    Z = np.stack([_sine(shape, k, perm) for k in idx[:6]], axis=1)
    d = np.linalg.norm(Z - hs.ldiv_block(F, A @ Z), axis=0).max()
    lam, X, log = _run(hs, F, M, nev=6)
    err = np.abs(np.sort(lam) - ref)
    print(f"maxrank {hs.maxrank(F)}  d = {d:.3e}  errors {err}  resid {log['resid']}")
    assert np.all(err <= 10.0 * d * np.abs(ref) + 1e-12)


def test_phase_timing_times_the_products_with_M_and_changes_no_bits(hs):
    P = _pencil(hs, ("S", 0.0), SHAPE, GM.pencil_S)
    L = hs._lib.lib()
    lam, X, log = _run(hs, P["F"], P["M"], "M", nev=6)
    assert L.hsk_eigs_gen_mprod_seconds() == 0.0  # taken only while the phase timing is on
    was = L.hsk_eigs_phase_timing(1)
    try:
        lam2, X2, log2 = _run(hs, P["F"], P["M"], "M", nev=6)
        t = L.hsk_eigs_gen_mprod_seconds()
    finally:
        L.hsk_eigs_phase_timing(was)
    print(f"products with M: {t * 1e3:.2f} ms of {log2['seconds'] * 1e3:.1f} ms")
    assert 0.0 < t < log2["seconds"] + 1.0
    assert np.array_equal(lam, lam2) and np.array_equal(X, X2) and np.array_equal(log["resid"], log2["resid"]) and log["nmprod"] == log2["nmprod"]


# ---- 10. errors and guards -------------------------------------------------------------------------------------------------------------------
def _raw(hs, F, n, M, inner, V0=None, nev=2, ncv=16, block=8):
    lib = hs._lib.lib()
    Mc = sp.csc_matrix(M)
    Mc.sort_indices()
    cp, rv, nz = Mc.indptr.astype(np.int64) + 1, Mc.indices.astype(np.int64) + 1, Mc.data.astype(np.float64)
    lam, res, est = np.full(2 * (nev + 1), 42.0), np.full(nev + 1, 42.0), np.full(nev + 1, 42.0)
    X = np.full((n, nev + 1), 42.0, order="F")
    nout, nconv = C.c_int64(-7), C.c_int64(-7)
    pf = lambda a: a.ctypes.data_as(hs._lib.p_f64)  # noqa: E731
    pi = lambda a: a.ctypes.data_as(hs._lib.p_i64)  # noqa: E731
    st = lib.hs_eigs_gen_d(F._h, 0, n, pi(cp), pi(rv), _vp(nz), inner, nev, ncv, block, 0.0, 0.0, TOL, 5, _vp(V0) if V0 is not None else None, n, 0, 0, pf(lam), _vp(X), n,
                           pf(res), pf(est), C.byref(nout), C.byref(nconv), None)
    assert nout.value == -7 and nconv.value == -7 and np.all(lam == 42.0) and np.all(res == 42.0) and np.all(est == 42.0) and np.all(X == 42.0)
    return st


def test_errors_and_guards(hs):
    P = _pencil(hs, ("S", 0.0), SHAPE, GM.pencil_S)
    A, M, F = P["A"], P["M"], P["F"]
    n = A.shape[0]
    E = hs._lib
    # an indefinite M: e_6 is a column of the start block and M[6, 6] < 0
    dneg = np.ones(n)
    dneg[5] = -1.0
    Mneg = sp.diags(dneg, format="csc")
    V0 = np.asfortranarray(np.random.default_rng(2).standard_normal((n, 8)))
    V0[:, 0] = 0.0
    V0[5, 0] = 1.0
    assert _raw(hs, F, n, Mneg, 1, V0=V0) == E.HS_ERR_ARGUMENT
    assert "positive definite" in E.lib().hs_last_error().decode()
    with pytest.raises(ValueError, match="positive definite"):
        hs.eigs(F, M=Mneg, inner="M", v0=V0, **KW)
    assert _raw(hs, F, n, Mneg, 2) == E.HS_ERR_ARGUMENT  # inner outside 0..1
    assert _raw(hs, F, n + 1, M, 0) == E.HS_ERR_DIMENSION
    assert _raw(hs, F, n, M, 0, nev=0) == E.HS_ERR_ARGUMENT
    # the counters: one product with M per block solve and the residual's, in the Euclidean mode
    lam, X, log = _run(hs, F, M, nev=6)
    info = hs.eigs_gen_info()
    nnz = M.nnz
    assert log["nmprod"] == log["nsolves"] + 1 == info["m_products"] and info["m_columns"] == 8 * log["nsolves"] + 6 and info["inner"] == "euclid"
    assert info["m_bytes"] == 8 * (n + 1) + 4 * nnz + 8 * nnz
    w0 = hs.eigs_info()["workspace_bytes"]
    lam, X, log = _run(hs, F, M, "M", nev=6)
    info = hs.eigs_gen_info()
    assert info["inner"] == "M" and info["m_products"] > log["nsolves"] + 2 and hs.eigs_info()["workspace_bytes"] == w0 + 8 * 8 * n
    # a handle the block solve does not serve: an HSS interior block (mf = 2)
    P2 = prepare(hs, (24, 24, 24), kind="convdiff", nmax=300, rhs="randn")
    F2 = hs.factor(P2["A"], P2["nd"], P2["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    try:
        n2 = P2["A"].shape[0]
        with pytest.raises(hs.UnsupportedError, match="block solve"):
            hs.eigs(F2, nev=4, M=sp.identity(n2, format="csc"), **KW)
        assert _raw(hs, F2, n2, sp.identity(n2, format="csc"), 0) == E.HS_ERR_UNSUPPORTED
    finally:
        F2.free()
