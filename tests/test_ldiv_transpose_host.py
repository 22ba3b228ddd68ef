"""ldiv!(transpose(F), B) / ldiv!(adjoint(F), B) without a GPU: the C ABI entry points, the Python wrappers, the nonsymmetric test
problems, and the refusals that the library names from a host-side plan (hs_plan) before any device work."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import prepare

NEW = ("hs_ldiv_t_d", "hs_ldiv_t_z", "hs_ldiv_dev_t_d", "hs_ldiv_dev_t_z")


def test_library_exports_the_transposed_solves(hs):
    L = hs._lib.lib()
    for name in NEW:
        assert name in hs._lib.EXPORTS
        assert getattr(L, name).restype is C.c_int
        assert getattr(L, name).argtypes[1] is C.c_int  # trans
    with open(hs._lib.os.path.join(hs._lib.os.path.dirname(hs._lib.CSRC), "..", "include", "hs_solver.h")) as f:
        hdr = f.read()
    for name in NEW:
        assert name + "(hs_handle* F, int trans," in hdr


@pytest.mark.parametrize("shape", [(9, 7), (5, 6, 4)])
def test_convdiff_is_nonsymmetric_with_the_poisson_pattern(hs, shape):
    A0 = hs.problems.grid_matrix(shape, "poisson")
    A = hs.problems.grid_matrix(shape, "convdiff")
    Z = hs.problems.grid_matrix(shape, "convdiff_helmholtz")
    assert A.dtype == np.float64 and Z.dtype == np.complex128
    for M in (A, Z):
        assert np.array_equal(M.indptr, A0.indptr) and np.array_equal(M.indices, A0.indices)
        assert np.all(M.data != 0)
    assert abs(A - A.T).max() > 0.1
    assert abs(Z - Z.T).max() > 0.1 and abs(Z - Z.conj().T).max() > 0.1
    # the Laplacian plus h * (v . grad): the symmetric part is Poisson's, the antisymmetric part the convection
    assert abs((A + A.T) / 2 - A0).max() < 1e-15
    pe = hs.problems.CONVDIFF_PECLET
    assert max(pe) < 2.0
    i = shape[0] + 1  # grid point (1, 1, ..): an interior point
    assert A[i, i + 1] == pytest.approx(-1.0 + pe[0] / 2) and A[i, i - 1] == pytest.approx(-1.0 - pe[0] / 2)
    # convdiff_helmholtz = convdiff + the Helmholtz shift of the same grid
    H = hs.problems.grid_matrix(shape, "helmholtz")
    assert abs((Z - A) - (H - A0)).max() < 1e-14
    # well conditioned: the same order of condition number as Poisson
    c0, c = np.linalg.cond(A0.toarray()), np.linalg.cond(A.toarray())
    assert c < 2 * c0


def _digest(M):
    M = sp.csc_matrix(M)
    h = hashlib.sha256()
    for a in (M.indptr, M.indices, M.data):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_existing_kinds_are_unchanged(hs):
    """Regression guard (passes before and after the convdiff kinds were added): poisson / helmholtz equal a restatement of their formula, bit
    for bit."""
    for shape in ((9, 7), (5, 6, 4)):
        d = len(shape)
        lap = None
        for ax in range(d):
            term = None
            for a in reversed(range(d)):
                n = shape[a]
                f = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr") if a == ax else sp.identity(n, format="csr")
                term = f if term is None else sp.kron(term, f, format="csr")
            lap = term if lap is None else lap + term
        P = sp.csc_matrix(lap.astype(np.float64))
        P.sort_indices()
        assert _digest(hs.problems.grid_matrix(shape, "poisson")) == _digest(P)
        kh = 2.0 * np.pi / 10.0
        faces = np.zeros(shape[::-1])
        for ax in range(d):
            lo, hi = [slice(None)] * d, [slice(None)] * d
            lo[d - 1 - ax], hi[d - 1 - ax] = 0, -1
            faces[tuple(lo)] += 1.0
            faces[tuple(hi)] += 1.0
        H = sp.csc_matrix(lap.astype(np.complex128) + sp.diags(-(kh**2) * np.ones(lap.shape[0]) - 1j * kh * faces.reshape(-1)))
        H.sort_indices()
        assert _digest(hs.problems.grid_matrix(shape, "helmholtz")) == _digest(H)


def test_wrappers(hs):
    """transpose / adjoint are light wrappers like Julia's Transpose / Adjoint; adjoint(adjoint(F)) is F."""
    F = object.__new__(hs.FactorNode)
    F._h, F.dtype, F.n, F._flat = None, np.dtype(np.complex128), 7, None
    T, A = hs.transpose(F), hs.adjoint(F)
    assert isinstance(T, hs.TransposedFactor) and T.parent is F and T.trans == 1 and T.n == 7 and T.shape == (7, 7)
    assert A.trans == 2 and repr(A) == "Adjoint{FactorNode{ComplexF64}}"
    assert hs.adjoint(A) is F and hs.transpose(T) is F
    with pytest.raises(TypeError):
        hs.transpose(A)  # conj(F): not a solve this library offers
    Fr = object.__new__(hs.FactorNode)
    Fr._h, Fr.dtype, Fr.n, Fr._flat = None, np.dtype(np.float64), 7, None
    assert hs.transpose(hs.adjoint(Fr)) is Fr  # Float64: adjoint = transpose
    with pytest.raises(TypeError):
        hs.transpose(np.eye(3))
    with pytest.raises(ValueError):
        F.solve(np.zeros(7), trans="X")
    with pytest.raises(hs.DimensionMismatch):
        hs.ldiv(T, np.zeros(6, dtype=np.complex128))
    with pytest.raises(TypeError, match="MethodError"):
        hs.ldiv(hs.transpose(Fr), np.zeros(7, dtype=np.complex128))
    F._h = Fr._h = None


def _call_t(hs, h, trans, n=1):
    L = hs._lib.lib()
    b = np.zeros(n)
    return L.hs_ldiv_t_d(h, trans, b.ctypes.data_as(hs._lib.p_f64), n, b.ctypes.data_as(hs._lib.p_f64), n, n, 1)


def _plan(hs, P, **kw):
    return hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], **kw)


def test_refusals_are_named_before_device_work(hs):
    """The limits of the transposed solve, from host-side plans: HS_ERR_UNSUPPORTED with the reason, trans outside 0..2 HS_ERR_ARGUMENT."""
    L = hs._lib.lib()
    P = prepare(hs, (20, 12), kind="convdiff", nmax=10)
    n = P["A"].shape[0]
    cases = [
        (dict(rank=0, nranks=2), "ranks"),
        (dict(rank=1, nranks=2, dist_top=True), "ranks"),
    ]
    for kw, word in cases:
        h = _plan(hs, P, **kw)
        try:
            for trans in (1, 2):
                st = _call_t(hs, h, trans, n)
                assert st == hs._lib.HS_ERR_UNSUPPORTED, (kw, st)
                assert word in L.hs_last_error().decode()
            assert _call_t(hs, h, 3, n) == hs._lib.HS_ERR_ARGUMENT
            assert _call_t(hs, h, -1, n) == hs._lib.HS_ERR_ARGUMENT
        finally:
            L.hs_free(h)
    P3 = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512)
    n3 = P3["A"].shape[0]
    for kw in (dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128), dict(swlevel=3, swsize=8, atol=1e-6, rtol=1e-6, mf=3, leafsize=128)):  # (hss_d: the GPU tests)
        h = _plan(hs, P3, **kw)
        try:
            st = _call_t(hs, h, 1, n3)
            assert st == hs._lib.HS_ERR_UNSUPPORTED, (kw, st)
            msg = L.hs_last_error().decode()
            assert "HSS" in msg and "ULV" in msg, msg
        finally:
            L.hs_free(h)
    # a single-rank plan without HSS fronts passes the refusals and stops at "not factored"
    h = _plan(hs, P)
    try:
        assert _call_t(hs, h, 1, n) == hs._lib.HS_ERR_ARGUMENT
        assert "not complete" in L.hs_last_error().decode()
    finally:
        L.hs_free(h)


def test_plan_bytes_do_not_change(hs):
    """The feature adds no factor memory and no workspace: hs_plan / hs_get_stats report the bytes recorded before the transposed solves
    existed (the plan depends on the pattern only: the same for Poisson and convdiff, x2 for ComplexF64)."""
    L = hs._lib.lib()
    for kind, want in (("convdiff", 74982400.0), ("convdiff_helmholtz", 149964800.0)):
        P = prepare(hs, (16, 14, 12), kind=kind, nmax=100)
        h = _plan(hs, P)
        try:
            st = hs._lib.hs_stats()
            assert L.hs_get_stats(h, C.byref(st)) == 0
            assert st.bytes_factors == want, (kind, st.bytes_factors)
            assert st.bytes_solve == 0.0
        finally:
            L.hs_free(h)
