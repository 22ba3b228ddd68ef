"""ldiv!(transpose(F), B) / ldiv!(adjoint(F), B) without a GPU: the C ABI entry points, the Python wrappers, the nonsymmetric test
problems, and the refusals that the library names from a host-side plan (hs_plan) before any device work."""
import ctypes as C
import hashlib
import re

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


BLOCK_ENTRIES = ("hs_ldiv_block_d", "hs_ldiv_block_t_d", "hs_ldiv_ulv_d", "hs_ldiv_sparse_d")
TRANS = (-1, 0, 1, 2, 3)


_UNFACTORED = (-1, 0, None, "not complete")


def _rows(name, t0, t12):
    """trans = -1 and 3 are refused under the entry point's name with trans as the info value; t0 / t12: what trans = 0 / trans = 1, 2 return."""
    t1, t2 = t12 if isinstance(t12, list) else (t12, t12)
    return [(-1, -1, name, "trans"), t0, t1, t2, (-1, 3, name, "trans")]


_BLOCK = _rows("hs_ldiv_block_*", _UNFACTORED, [(-8, 1, "hs_ldiv_block_*", "trans"), (-8, 2, "hs_ldiv_block_*", "trans")])
_BLOCK_T = _rows("hs_ldiv_block_t_*", _UNFACTORED, _UNFACTORED)
# recorded on the commit before the checks were folded (-1: HS_ERR_ARGUMENT, -8: HS_ERR_UNSUPPORTED)
REFUSALS = {
    ("rank0of2", "hs_ldiv_block_d"): _BLOCK,
    ("rank0of2", "hs_ldiv_block_t_d"): _BLOCK_T,
    ("rank0of2", "hs_ldiv_ulv_d"): _rows("hs_ldiv_ulv_*", (-8, 0, "hs_ldiv_ulv_*", "ranks"), (-8, 0, "hs_ldiv_ulv_*", "ranks")),
    ("rank0of2", "hs_ldiv_sparse_d"): _rows("hs_ldiv_sparse_*", (-8, 0, "hs_ldiv_sparse_*", "ranks"), (-8, 0, "hs_ldiv_sparse_*", "ranks")),
    ("rank1of2_dist_top", "hs_ldiv_block_d"): _BLOCK,
    ("rank1of2_dist_top", "hs_ldiv_block_t_d"): _BLOCK_T,
    ("rank1of2_dist_top", "hs_ldiv_ulv_d"): _rows("hs_ldiv_ulv_*", (-8, 0, "hs_ldiv_ulv_*", "ranks"), (-8, 0, "hs_ldiv_ulv_*", "ranks")),
    ("rank1of2_dist_top", "hs_ldiv_sparse_d"): _rows("hs_ldiv_sparse_*", (-8, 0, "hs_ldiv_sparse_*", "ranks"), (-8, 0, "hs_ldiv_sparse_*", "ranks")),
    ("single", "hs_ldiv_block_d"): _BLOCK,
    ("single", "hs_ldiv_block_t_d"): _BLOCK_T,
    ("single", "hs_ldiv_ulv_d"): _rows("hs_ldiv_ulv_*", _UNFACTORED, _UNFACTORED),
    ("single", "hs_ldiv_sparse_d"): _rows("hs_ldiv_sparse_*", _UNFACTORED, _UNFACTORED),
    ("mf2", "hs_ldiv_block_d"): _BLOCK,
    ("mf2", "hs_ldiv_block_t_d"): _BLOCK_T,
    ("mf2", "hs_ldiv_ulv_d"): _rows("hs_ldiv_ulv_*", _UNFACTORED, _UNFACTORED),
    ("mf2", "hs_ldiv_sparse_d"): _rows("hs_ldiv_sparse_*", (-8, 126, "hs_ldiv_sparse_*", "HSS"), (-8, 126, "hs_ldiv_sparse_*", "HSS")),
    ("mf3", "hs_ldiv_block_d"): _BLOCK,
    ("mf3", "hs_ldiv_block_t_d"): _BLOCK_T,
    ("mf3", "hs_ldiv_ulv_d"): _rows("hs_ldiv_ulv_*", _UNFACTORED, _UNFACTORED),
    ("mf3", "hs_ldiv_sparse_d"): _rows("hs_ldiv_sparse_*", (-8, 62, "hs_ldiv_sparse_*", "HSS"), (-8, 62, "hs_ldiv_sparse_*", "HSS")),
}


def _refusal(hs, h, entry, trans, n):
    """(status, hs_last_error_info(), the entry-point name the message prints, its discriminating word) of one call on a plan-only handle."""
    L = hs._lib.lib()
    pf, pi = hs._lib.p_f64, hs._lib.p_i64
    b = np.zeros(n)
    if entry == "hs_ldiv_sparse_d":
        cp, rv, val = np.array([1, 2], dtype=np.int64), np.array([1], dtype=np.int64), np.ones(1)
        st = L.hs_ldiv_sparse_d(h, trans, n, 1, cp.ctypes.data_as(pi), rv.ctypes.data_as(pi), val.ctypes.data_as(pf), None, 0, b.ctypes.data_as(pf), n)
    else:
        st = getattr(L, entry)(h, trans, b.ctypes.data_as(pf), n, b.ctypes.data_as(pf), n, n, 1)
    msg = L.hs_last_error().decode()
    name = re.search(r"hs_ldiv_\w+_\*", msg)
    word = next((w for w in ("ranks", "HSS", "not complete", "trans") if w in msg), None)  # ("transposed" in the first two: they come first)
    return (st, int(L.hs_last_error_info()), name.group(0) if name else None, word)


def _refusal_table(hs):
    P = prepare(hs, (20, 12), kind="convdiff", nmax=10)
    P3 = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512)
    handles = [
        ("rank0of2", P, dict(rank=0, nranks=2)),
        ("rank1of2_dist_top", P, dict(rank=1, nranks=2, dist_top=True)),
        ("single", P, dict()),
        ("mf2", P3, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)),
        ("mf3", P3, dict(swlevel=3, swsize=8, atol=1e-6, rtol=1e-6, mf=3, leafsize=128)),
    ]
    table = {}
    for hname, Pr, kw in handles:
        h = _plan(hs, Pr, **kw)
        try:
            for entry in BLOCK_ENTRIES:
                table[(hname, entry)] = [_refusal(hs, h, entry, t, Pr["A"].shape[0]) for t in TRANS]
        finally:
            hs._lib.lib().hs_free(h)
    return table


def test_block_refusals_keep_their_order_and_names(hs):
    """What hs_ldiv_block_d / hs_ldiv_block_t_d / hs_ldiv_ulv_d / hs_ldiv_sparse_d answer on the plan-only handles of the test above for trans = -1, 0,
    1, 2, 3: status, hs_last_error_info(), the entry point the message names and the word that tells the refusals apart.  The entry points run
    their checks in different orders (e.g. hs_ldiv_block_* names an unfactored handle before its ranks, hs_ldiv_ulv_* the other way round);
    the values are the ones recorded before the checks were folded into shared pieces."""
    got = _refusal_table(hs)
    assert sorted(got) == sorted(REFUSALS)
    for key in sorted(REFUSALS):
        for t, g, want in zip(TRANS, got[key], REFUSALS[key]):
            assert g == want, (key, t, g, want)


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
