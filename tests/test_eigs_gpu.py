"""Shift-invert eigenpairs from the stored factors (hs.eigs, csrc/hs_eigs.hip + kernels_eigs.hip) on the MI355X: the rotation and Cholesky
kernels alone, then the driver on matrices with known spectra.  Every driver case uses tol = 1e-10, block = 8, ncv = 48, maxrestart = 30 and
asserts restarts <= 30 (the NumPy mirror of tests/test_eigs_host.py needs at most 7).  Matrices are built in the grid's own ordering and
permuted with the nested-dissection permutation of helpers.prepare.

Residual bound (||x|| = 1):  resid_c <= 2 tol sqrt(||A_s||_1 ||A_s||_inf), from  A_s x - mu x = -mu A_s (F^-1 x - theta x)  with
|mu| ||F^-1 x - theta x|| = est <= tol and ||A_s||_2 <= sqrt(||A_s||_1 ||A_s||_inf); the factor 2 covers rounding."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from helpers import prepare
from eigs_mirror import convection, convection_spectrum, match, nearest, poisson, poisson_spectrum

pytestmark = pytest.mark.gpu

TOL = 1e-10
KW = dict(tol=TOL, block=8, ncv=48, maxrestart=30)
SHAPE = (12, 11, 10)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for v in _CACHE.values():
        v[1].free()
    _CACHE.clear()


def _factored(hs, key, shape, build, sigma=0.0, nmax=100, **opts):
    """(A in the factored ordering, F of A - sigma I, perm) for A = build(shape) in the grid ordering"""
    if key not in _CACHE:
        P = prepare(hs, shape, nmax=nmax)
        perm = P["perm"]
        A = build(shape)
        A = A[perm - 1][:, perm - 1].tocsc()
        As = (A - sigma * sp.identity(A.shape[0], dtype=A.dtype)).tocsc()
        As.sort_indices()
        _CACHE[key] = (A, hs.factor(As, P["nd"], P["nd_loc"], **(opts or dict(swlevel=0))), perm, As)
    return _CACHE[key]


def _resid_bound(As):
    return 2.0 * TOL * np.sqrt(spla.norm(As, 1) * spla.norm(As, np.inf))


def _run(hs, F, **kw):
    lam, X, log = hs.eigs(F, log=True, **{**KW, **kw})
    print(f"restarts {log['restarts']} solves {log['nsolves']} replaced {log['replaced']} resid {log['resid'].max():.2e} est {log['est'].max():.2e} "
          f"{log['seconds'] * 1e3:.1f} ms")
    assert log["restarts"] <= 30 and log["nconv"] == len(lam)
    assert np.allclose(np.linalg.norm(X, axis=0), 1.0, rtol=0, atol=1e-12)
    return lam, X, log


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _ints(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, shape).astype(float)
    return X + 1j * rng.integers(-3, 4, shape) if cplx else X


def _rotate(hs, V, Q, inplace):
    cplx = np.iscomplexobj(V)
    n, K = V.shape
    N = Q.shape[1]
    Vf, Qf = np.asfortranarray(V), np.asfortranarray(Q)
    V0 = Vf.copy()
    Out = np.full((n, N), np.nan, dtype=Vf.dtype, order="F")
    fn = getattr(hs._lib.lib(), "hsk_eigs_rotate" + ("_z" if cplx else "_d"))
    hs._lib.check(fn(n, K, N, _vp(Vf), n, _vp(Qf), K, int(inplace), _vp(Out), n))
    assert np.array_equal(Vf, V0)
    return Out


# ---- 1. the rotation kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n", [1, 63, 65, 2049])
def test_rotate_is_exact_on_integers_in_and_out_of_place(hs, n, cplx):
    for K in (1, 3, 5, 17, 64, 256):
        V = _ints((n, K), cplx, 7 * K + n)
        for N in sorted({1, max(K // 2, 1), K}):
            Q = _ints((K, N), cplx, 11 * K + N)
            ref = V @ Q
            assert np.array_equal(_rotate(hs, V, Q, False), ref), (n, K, N, "out of place")
            assert np.array_equal(_rotate(hs, V, Q, True), ref), (n, K, N, "in place")


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_rotate_row_bits_do_not_depend_on_the_block(hs, cplx):
    rng = np.random.default_rng(4)
    V = rng.standard_normal((2049, 50)) + (1j * rng.standard_normal((2049, 50)) if cplx else 0.0)
    Q = rng.standard_normal((50, 23)) + (1j * rng.standard_normal((50, 23)) if cplx else 0.0)
    full = _rotate(hs, V, Q, True)
    assert np.allclose(full, V @ Q, rtol=0, atol=1e-12 * 50)
    for rows in (1, 65, 1000):
        assert np.array_equal(_rotate(hs, V[:rows], Q, False), full[:rows])


# ---- 2. Cholesky and inverse ---------------------------------------------------------------------------------------------------------------
def _chol_inv(hs, G):
    cplx = np.iscomplexobj(G)
    p = G.shape[0]
    Gf = np.asfortranarray(G)
    R = np.full((p, p), np.nan, dtype=Gf.dtype, order="F")
    Ri = np.full((p, p), np.nan, dtype=Gf.dtype, order="F")
    info = C.c_int(99)
    hs._lib.check(getattr(hs._lib.lib(), "hsk_eigs_chol_inv" + ("_z" if cplx else "_d"))(p, _vp(Gf), p, _vp(R), _vp(Ri), C.byref(info)))
    return R, Ri, info.value


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("p", [1, 2, 17, 32, 64])
def test_chol_inv_against_numpy(hs, p, cplx):
    rng = np.random.default_rng(p)
    W = rng.standard_normal((3 * p + 5, p)) + (1j * rng.standard_normal((3 * p + 5, p)) if cplx else 0.0)
    G = W.conj().T @ W
    R, Ri, info = _chol_inv(hs, G)
    assert info == -1
    ref = np.linalg.cholesky(G).conj().T
    tol = 1e-13 * np.linalg.cond(G)
    print(f"p = {p}: |R - ref| {np.abs(R - ref).max():.1e}, |R Ri - I| {np.abs(R @ Ri - np.eye(p)).max():.1e}, bound {tol:.1e}")
    assert np.array_equal(np.tril(R, -1), np.zeros((p, p))) and np.array_equal(np.tril(Ri, -1), np.zeros((p, p)))
    assert np.abs(R - ref).max() <= tol * np.abs(ref).max()
    assert np.abs(Ri - np.linalg.inv(ref)).max() <= tol * np.abs(np.linalg.inv(ref)).max()


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_chol_inv_names_the_dependent_column(hs, cplx):
    rng = np.random.default_rng(1)
    W = rng.standard_normal((40, 9)) + (1j * rng.standard_normal((40, 9)) if cplx else 0.0)
    W[:, 3] = 0.0
    assert _chol_inv(hs, W.conj().T @ W)[2] == 3
    W[:, 3] = W[:, :3] @ np.array([1.0, -2.0, 0.5])  # dependent on the columns before it, not zero
    assert _chol_inv(hs, W.conj().T @ W)[2] in (3, -1)  # the pivot is rounding noise of either sign: column 3 or none, never another
    assert _chol_inv(hs, np.zeros((4, 4)) + (0j if cplx else 0.0))[2] == 0


# ---- 3, 4. Poisson, unshifted and shifted --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.0, 3.1])
def test_poisson_nearest_eigenvalues(hs, sigma):
    A, F, _, As = _factored(hs, ("poisson", sigma), SHAPE, poisson, sigma=sigma)
    ref = np.sort(nearest(poisson_spectrum(SHAPE), sigma, 6))
    lam, X, log = _run(hs, F, nev=6, sigma=sigma)
    assert lam.dtype == np.float64 and X.dtype == np.float64 and lam.shape == (6,) and X.shape == (A.shape[0], 6)
    assert np.array_equal(np.argsort(np.abs(lam - sigma), kind="stable"), np.arange(6))  # nearest first
    o = np.argsort(lam)
    err, res = np.abs(lam[o] - ref), log["resid"][o]
    print("errors", err, "resid", res, "bound", _resid_bound(As))
    assert np.all(err <= res + 1e-12 * spla.norm(A, 1))  # Hermitian: an eigenvalue within the residual
    assert np.all(res <= _resid_bound(As))
    assert np.allclose(np.linalg.norm(A @ X - X * lam, axis=0), log["resid"], rtol=0, atol=1e-13 * spla.norm(A, 1))  # the reported residuals are the true ones
    lam2, X2, log2 = _run(hs, F, nev=6, sigma=sigma)
    assert np.array_equal(lam, lam2) and np.array_equal(X, X2) and np.array_equal(log["resid"], log2["resid"]) and np.array_equal(log["est"], log2["est"])


# ---- 5. multiple eigenvalues ---------------------------------------------------------------------------------------------------------------
def test_cube_multiplicities(hs):
    shape = (10, 10, 10)
    A, F, _, As = _factored(hs, "cube", shape, poisson)
    lam, X, log = _run(hs, F, nev=7)  # multiplicities 1 + 3 + 3
    ref = poisson_spectrum(shape)[:7]
    assert np.all(np.abs(np.sort(lam) - ref) <= np.sort(log["resid"])[::-1].max() + 1e-12 * spla.norm(A, 1))
    assert np.all(log["resid"] <= _resid_bound(As))
    assert np.linalg.matrix_rank(X, 1e-8) == 7


# ---- 6, 8. real nonsymmetric with complex pairs, right and left ------------------------------------------------------------------------------
PE = 8.0
KAPPA = 17.0  # >= (5/3)^5.5: the eigenvector condition number of the x-factor tridiag(-1 - pe/2, 2, -1 + pe/2), D = diag((5/3)^(j/2))


def _pairs_ok(lam):
    return np.all(lam[0::2].imag > 0) and np.array_equal(lam[0::2], np.conj(lam[1::2]))


def test_real_nonsymmetric_pairs(hs):
    A, F, _, As = _factored(hs, "conv", SHAPE, lambda s: convection(s, PE), sigma=2.0)
    ref = nearest(convection_spectrum(SHAPE, PE), 2.0, 6)
    lam, X, log = _run(hs, F, nev=6, sigma=2.0)
    assert lam.dtype == np.complex128 and X.dtype == np.complex128 and len(lam) == 6 and _pairs_ok(lam)
    d = np.abs(lam[:, None] - ref[None, :])
    print("errors", d.min(axis=1), "resid", log["resid"])
    assert np.all(d.min(axis=1) <= KAPPA * log["resid"] + 1e-11) and match(lam, ref) <= KAPPA * log["resid"].max() + 1e-11
    assert np.all(log["resid"] <= _resid_bound(As)) and np.array_equal(log["resid"][0::2], log["resid"][1::2])
    assert np.allclose(np.linalg.norm(A @ X - X * lam, axis=0), log["resid"], rtol=0, atol=1e-13 * spla.norm(A, 1))
    lam5, X5, log5 = _run(hs, F, nev=5, sigma=2.0)  # a pair is not split
    assert len(lam5) == 6 and X5.shape[1] == 6 and _pairs_ok(lam5)
    assert match(lam5, ref) <= KAPPA * log5["resid"].max() + 1e-11


@pytest.mark.parametrize("which", ["transpose", "adjoint"])
def test_left_eigenvectors_real(hs, which):
    A, F, _, As = _factored(hs, "conv", SHAPE, lambda s: convection(s, PE), sigma=2.0)
    lam0, _, log0 = _run(hs, F, nev=6, sigma=2.0)
    lam, Y, log = _run(hs, getattr(hs, which)(F), nev=6, sigma=2.0)
    assert len(lam) == 6 and _pairs_ok(lam)  # Float64: the adjoint is the transpose, conj(lambda) is the other member of the pair
    both = KAPPA * (log["resid"].max() + log0["resid"].max()) + 2e-11
    assert match(lam, lam0) <= both
    assert np.all(log["resid"] <= _resid_bound(As))
    assert np.all(np.linalg.norm(As.T @ Y - Y * (lam - 2.0), axis=0) <= _resid_bound(As))  # y^T A_s = mu y^T


# ---- 7, 8. Helmholtz, right and left -----------------------------------------------------------------------------------------------------
def _helmholtz(hs):
    if "helm" not in _CACHE:
        P = prepare(hs, (10, 9, 8), kind="helmholtz", nmax=100)
        A = P["A"]
        w, Xr = np.linalg.eig(A.toarray())
        _CACHE["helm"] = (A, hs.factor(A, P["nd"], P["nd_loc"], swlevel=0), w, np.linalg.cond(Xr))
    return _CACHE["helm"]


def test_helmholtz_against_dense_eig(hs):
    A, F, w, condX = _helmholtz(hs)
    ref = nearest(w, 0.0, 6)
    lam, X, log = _run(hs, F, nev=6)
    assert lam.dtype == np.complex128 and X.dtype == np.complex128
    d = np.abs(lam[:, None] - ref[None, :])
    print("errors", d.min(axis=1), "resid", log["resid"], "cond(X_ref)", condX)
    assert np.all(d.min(axis=1) <= condX * log["resid"] + 1e-11 * spla.norm(A, 1)) and np.all(d.min(axis=0) <= condX * log["resid"].max() + 1e-11 * spla.norm(A, 1))
    assert np.all(log["resid"] <= _resid_bound(A))
    assert np.allclose(np.linalg.norm(A @ X - X * lam, axis=0), log["resid"], rtol=0, atol=1e-13 * spla.norm(A, 1))
    lam2, X2, _ = _run(hs, F, nev=6)
    assert np.array_equal(lam, lam2) and np.array_equal(X, X2)


@pytest.mark.parametrize("which", ["transpose", "adjoint"])
def test_left_eigenvectors_complex(hs, which):
    A, F, w, condX = _helmholtz(hs)
    lam0, _, log0 = _run(hs, F, nev=6)
    lam, Y, log = _run(hs, getattr(hs, which)(F), nev=6)
    lamA = np.conj(lam) if which == "adjoint" else lam  # the adjoint returns the eigenvalues of A^H
    assert match(lamA, lam0) <= condX * (log["resid"].max() + log0["resid"].max()) + 2e-11 * spla.norm(A, 1)
    assert np.all(log["resid"] <= _resid_bound(A))
    op = A.conj().T if which == "adjoint" else A.T
    assert np.all(np.linalg.norm(op @ Y - Y * lam, axis=0) <= _resid_bound(A))  # y^H A = lambda_A y^H  <=>  A^H y = conj(lambda_A) y


def test_device_blocks_on_a_side_stream_return_the_bits_of_the_host_form(hs):
    import torch

    A, F, w, condX = _helmholtz(hs)
    n = A.shape[0]
    rng = np.random.default_rng(3)
    v0 = rng.standard_normal((n, 8)) + 1j * rng.standard_normal((n, 8))
    lam, X, log = _run(hs, F, nev=6, v0=v0)
    dev = torch.device("cuda:0")
    ld = n + 3
    Vp = np.zeros((ld, 8), dtype=np.complex128, order="F")
    Vp[:n] = v0
    dV = torch.from_numpy(Vp.T.copy()).to(dev)  # row j of the tensor = column j of the block
    dX = torch.full((7, ld), 7.0, dtype=torch.complex128, device=dev)
    lamd, res, est = np.zeros(14), np.zeros(7), np.zeros(7)
    nout, nconv = C.c_int64(), C.c_int64()
    pf = lambda a: a.ctypes.data_as(hs._lib.p_f64)  # noqa: E731
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        hs._lib.check(hs._lib.lib().hs_eigs_z(F._h, 0, n, 6, 48, 8, 0.0, 0.0, TOL, 30, C.c_void_p(dV.data_ptr()), ld, 0, 1, pf(lamd), C.c_void_p(dX.data_ptr()), ld, pf(res),
                                              pf(est), C.byref(nout), C.byref(nconv), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    Xd = dX.cpu().numpy().T
    assert nout.value == 6 and nconv.value == 6
    assert np.array_equal(lamd[0:12:2] + 1j * lamd[1:12:2], lam) and np.array_equal(res[:6], log["resid"]) and np.array_equal(est[:6], log["est"])
    assert np.array_equal(Xd[:n, :6], X) and np.all(Xd[n:] == 7.0) and np.all(Xd[:, 6] == 7.0)  # padding rows and the spare column untouched
    assert np.array_equal(dV.cpu().numpy().T, Vp)


# ---- 9. deflation ---------------------------------------------------------------------------------------------------------------------------
def _sine(shape, k, perm):
    nx, ny, nz = shape
    f = [np.sin(kk * np.pi * np.arange(1, m + 1) / (m + 1)) for kk, m in zip(k, shape)]
    v = np.kron(np.kron(f[2], f[1]), f[0])
    return (v / np.linalg.norm(v))[perm - 1]


def test_start_block_of_eigenvectors_is_deflated(hs):
    A, F, perm, As = _factored(hs, ("poisson", 0.0), SHAPE, poisson)
    n = A.shape[0]
    v0 = np.random.default_rng(5).standard_normal((n, 4))
    v0[:, 0], v0[:, 1] = _sine(SHAPE, (1, 1, 1), perm), _sine(SHAPE, (2, 1, 1), perm)
    assert np.linalg.norm(A @ v0[:, 0] - poisson_spectrum(SHAPE)[0] * v0[:, 0]) < 1e-13
    lam, X, log = _run(hs, F, nev=6, block=4, v0=v0)
    ref = poisson_spectrum(SHAPE)[:6]
    o = np.argsort(lam)
    assert np.all(np.abs(lam[o] - ref) <= log["resid"][o] + 1e-12 * spla.norm(A, 1)) and np.all(log["resid"] <= _resid_bound(As))
    assert log["replaced"] >= 1


# ---- 10. a compressed handle ---------------------------------------------------------------------------------------------------------------
def test_compressed_handle_within_its_own_accuracy(hs):
    """d = max_c ||z_c - F^-1 (A z_c)||_2 over the analytic unit eigenvectors of the wanted pairs is what the compressed factors are off by;
    first-order perturbation of a symmetric matrix then gives |lam_c - ref_c| <= d |ref_c| (+ second order: the factor 10)."""
    shape = (24, 22, 20)
    A, F, perm, As = _factored(hs, "compressed", shape, poisson, nmax=300, swlevel=2, swsize=8, atol=1e-6, rtol=1e-6)
    assert hs.maxrank(F) > 0
    nx, ny, nz = shape
    idx = [(kx, ky, kz) for kz in range(1, 4) for ky in range(1, 4) for kx in range(1, 4)]
    val = lambda k: sum(2 - 2 * np.cos(kk * np.pi / (m + 1)) for kk, m in zip(k, shape))  # noqa: E731
    idx.sort(key=val)
    ref = np.array([val(k) for k in idx[:6]])
    assert np.allclose(ref, poisson_spectrum(shape)[:6], rtol=0, atol=1e-13)
    Z = np.stack([_sine(shape, k, perm) for k in idx[:6]], axis=1)
    d = np.linalg.norm(Z - hs.ldiv_block(F, A @ Z), axis=0).max()
    lam, X, log = _run(hs, F, nev=6)
    err = np.abs(np.sort(lam) - ref)
    print(f"maxrank {hs.maxrank(F)}  d = {d:.3e}  errors {err}  resid {log['resid']}")
    assert np.all(err <= 10.0 * d * np.abs(ref) + 1e-12)


# ---- 11. refusals and errors ---------------------------------------------------------------------------------------------------------------
def _raw(hs, F, n, nev=2, ncv=8, block=2, sigma_im=0.0):
    lib = hs._lib.lib()
    lam, res, est = np.full(2 * (nev + 1), 42.0), np.full(nev + 1, 42.0), np.full(nev + 1, 42.0)
    X = np.full((n, nev + 1), 42.0, order="F")
    nout, nconv = C.c_int64(-7), C.c_int64(-7)
    pf = lambda a: a.ctypes.data_as(hs._lib.p_f64)  # noqa: E731
    st = lib.hs_eigs_d(F._h, 0, n, nev, ncv, block, 0.0, sigma_im, TOL, 5, None, n, 0, 0, pf(lam), _vp(X), n, pf(res), pf(est), C.byref(nout), C.byref(nconv), None)
    assert nout.value == -7 and nconv.value == -7 and np.all(lam == 42.0) and np.all(res == 42.0) and np.all(est == 42.0) and np.all(X == 42.0)
    return st


def test_refusals_and_errors(hs):
    A, F, _, _ = _factored(hs, ("poisson", 0.0), SHAPE, poisson)
    n = A.shape[0]
    E = hs._lib
    with pytest.raises(ValueError, match="256"):
        hs.eigs(F, ncv=250, block=8)
    Ps = prepare(hs, (13, 7), nmax=10)  # n = 91
    Fs = hs.factor(Ps["A"], Ps["nd"], Ps["nd_loc"], swlevel=0)
    try:
        with pytest.raises(ValueError, match="n = 91 < ncv \\+ block"):
            hs.eigs(Fs, nev=6, ncv=88, block=8)
        assert _raw(hs, Fs, 91, nev=6, ncv=88, block=8) == E.HS_ERR_ARGUMENT
        lam, X, log = _run(hs, Fs, nev=4, ncv=80, block=8)  # n is barely above ncv + block
        assert np.abs(np.sort(lam) - np.sort(np.linalg.eigvalsh(Ps["A"].toarray()))[:4]).max() <= log["resid"].max() + 1e-12 * spla.norm(Ps["A"], 1)
    finally:
        Fs.free()
    with pytest.raises(ValueError, match="complex shift"):
        hs.eigs(F, sigma=1.0 + 1.0j)
    # the library's own checks, with every output untouched
    assert _raw(hs, F, n, ncv=250, block=8) == E.HS_ERR_ARGUMENT
    assert _raw(hs, F, n, nev=0) == E.HS_ERR_ARGUMENT
    assert _raw(hs, F, n, nev=7, ncv=8, block=2) == E.HS_ERR_ARGUMENT
    assert _raw(hs, F, n, sigma_im=0.5) == E.HS_ERR_ARGUMENT
    assert _raw(hs, F, n + 1) == E.HS_ERR_DIMENSION
    assert E.lib().hs_eigs_z(F._h, 0, n, 2, 8, 2, 0.0, 0.0, TOL, 5, None, n, 0, 0, None, None, n, None, None, None, None, None) == E.HS_ERR_DIMENSION
    # the defaults: block = 16, ncv = the multiple of 16 at or above max(2 nev + 16, 64)
    lam, X, log = hs.eigs(F, nev=30, tol=1e-8, log=True)
    assert log["ncv"] == 80 and len(lam) == 30
    assert np.abs(np.sort(lam) - poisson_spectrum(SHAPE)[:30]).max() <= log["resid"].max() + 1e-12 * spla.norm(A, 1)
    lam, X = hs.eigs(F, nev=3, vectors=False, **KW)
    assert X is None and lam.shape == (3,)
    # maxrestart = 0: one pass over the basis does not converge six Helmholtz pairs
    Ah, Fh, _, _ = _helmholtz(hs)
    with pytest.raises(hs.NoConvergence) as ei:
        hs.eigs(Fh, nev=6, **{**KW, "maxrestart": 0})
    lam, X, log = ei.value.partial
    assert log["nconv"] < 6 and log["restarts"] == 0 and len(lam) == 6 and X.shape == (Ah.shape[0], 6)
    # a handle the block solve does not serve: an HSS interior block (mf = 2)
    P2 = prepare(hs, (24, 24, 24), kind="convdiff", nmax=300, rhs="randn")
    F2 = hs.factor(P2["A"], P2["nd"], P2["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    try:
        n2 = P2["A"].shape[0]
        with pytest.raises(hs.UnsupportedError, match="block solve"):
            hs.eigs(F2, nev=4, **KW)
        assert _raw(hs, F2, n2) == E.HS_ERR_UNSUPPORTED
    finally:
        F2.free()
