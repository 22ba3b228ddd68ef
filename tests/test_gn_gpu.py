"""Tangent-linear solves and Gauss-Newton products (hs_tangent_*, hs_gn_hessvec_*, hs_gn_diag_*; csrc/hs_gn.hip + csrc/kernels_gn.hip) on the
MI355X: the right-hand side and row square sum kernels alone, the solves bit for bit against the block solves and against hs.sensitivity,
determinism over calls, group widths, supplied fields and sparse blocks, the identities that tie the forward mode to the reverse mode, the
conventions end to end against the NumPy mirror with SuperLU solves, the diagonal, refusals, and the device entry points on a side stream.
Problems and option sets are those of test_ldiv_block_gpu.py; one factorization per (kind, options) is shared by the tests of this file."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import gn_mirror as GM
import sens_mirror as SM
from helpers import prepare
from test_ldiv_block_gpu import COMPRESSED, EXACT, TOL, _kc, _rand
from test_ldiv_sparse_host import sources
from test_sens_gpu import _pattern70

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
KS = (1, 5, 40)
SMALL = EXACT[:2]  # 2-D 30 x 27, real and complex
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for c in _CACHE.values():
        c["F"].free()
    _CACHE.clear()


def _get(hs, kind, shape, nmax, label="exact", **kw):
    key = (kind, shape, nmax, label)
    if key not in _CACHE:
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        F = hs.factor(P["A"], P["nd"], P["nd_loc"], **(kw or dict(swlevel=0)))
        A = SM.canonical(P["A"])
        n = A.shape[0]
        rng = np.random.default_rng(17)
        inner = rng.choice(np.arange(1, n - 1), size=5, replace=False)
        rows = np.array([inner[0], n - 1, inner[1], inner[2], 0, inner[3], inner[4]])  # 7 distinct, unsorted, both ends
        _CACHE[key] = dict(P=P, F=F, A=A, n=n, rows=rows, cplx=F.dtype.kind == "c", solve=None)
    return _CACHE[key]


def _op(hs, F, trans):
    return (F, hs.transpose(F), hs.adjoint(F))[trans]


def _dir(c, pattern, seed):
    return _rand(c["A"].nnz if pattern == "A" else c["n"], 1, c["cplx"], seed)[:, 0]


def _rhs(hs, A, E, X, trans, pattern="A", ld=None, ldp=None):
    """The kernel of P = -op(E) X alone (hsk_gn_rhs_*); the padding rows of X are poisoned and those of P must come back untouched."""
    n, kc = A.shape[0], X.shape[1]
    cplx = np.iscomplexobj(X) or np.iscomplexobj(E)
    dt = np.complex128 if cplx else np.float64
    ld, ldp = ld or n, ldp or n
    Xp, Pp = np.full((ld, kc), 99, dtype=dt, order="F"), np.full((ldp, kc), 77, dtype=dt, order="F")
    Xp[:n] = X
    Ev = np.ascontiguousarray(E, dtype=dt)
    cp = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rv = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    L = hs._lib
    fn = L.lib().hsk_gn_rhs_z if cplx else L.lib().hsk_gn_rhs_d
    L.check(fn(trans, n, cp.ctypes.data_as(L.p_i64), rv.ctypes.data_as(L.p_i64), Ev.ctypes.data, 0 if pattern == "A" else 1, Xp.ctypes.data, ld, kc, Pp.ctypes.data, ldp))
    assert np.all(Pp[n:] == 77)
    return np.ascontiguousarray(Pp[:n])


def _rowsq(hs, X, acc, ld=None):
    n, kc = X.shape
    cplx = np.iscomplexobj(X)
    ld = ld or n
    Xp = np.full((ld, kc), 99, dtype=X.dtype, order="F")
    Xp[:n] = X
    out = np.ascontiguousarray(acc, dtype=np.float64).copy()
    L = hs._lib
    fn = L.lib().hsk_gn_rowsq_z if cplx else L.lib().hsk_gn_rowsq_d
    L.check(fn(n, kc, Xp.ctypes.data, ld, out.ctypes.data))
    return out


# ---- a. the right-hand side kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["Float64", "ComplexF64"])
def test_rhs_kernel_is_exact_on_small_integers(hs, cplx):
    rng = np.random.default_rng(2)

    def ints(shape):
        M = rng.integers(-3, 4, size=shape).astype(np.float64)
        return M + 1j * rng.integers(-3, 4, size=shape) if cplx else M

    A = _pattern70()  # an empty column, a column of 70 entries, a missing diagonal entry, nnz not a multiple of 64
    n = A.shape[0]
    X = ints((n, 35))
    for pattern in ("A", "diag"):
        E = ints(A.nnz if pattern == "A" else n)
        for trans in (0, 1, 2):
            M = GM.op_matrix(A, E, trans, pattern)
            for kc in (1, 9, 35):
                got = _rhs(hs, A, E, X[:, :kc], trans, pattern, ld=n + 3, ldp=n + 5)
                assert np.array_equal(got, -(M @ X[:, :kc])), (pattern, trans, kc)
    # a value at a j whose (j, j) is not stored counts as 0
    Ed = np.ones(n) + (0j if cplx else 0)
    P = _rhs(hs, A, Ed, X[:, :9], 0, "diag")
    assert not P[5].any() and not P[12].any() and np.array_equal(np.delete(P, [5, 12], axis=0), -np.delete(X[:, :9], [5, 12], axis=0))


@pytest.mark.parametrize("cplx", [False, True], ids=["Float64", "ComplexF64"])
def test_rhs_kernel_within_the_row_bound_on_random_data(hs, cplx):
    A = _pattern70()
    n = A.shape[0]
    X = _rand(n, 35, cplx, 3)
    for pattern in ("A", "diag"):
        E = _rand(A.nnz if pattern == "A" else n, 1, cplx, 4)[:, 0]
        for trans in (0, 1, 2):
            M = GM.op_matrix(A, E, trans, pattern)
            # the length of the chain: the longest row of op(E) (the dense column 9 is a row of E^T and E^H), one entry for the diagonal form
            m = 1 if pattern == "diag" else int(np.diff(M.indptr).max())
            assert m == 1 or (m == 70) == (trans != 0)
            got = _rhs(hs, A, E, X, trans, pattern, ld=n + 3)
            S = abs(M) @ np.abs(X)
            excess = np.abs(got + M @ X) - 4 * (m + 4) * EPS * S
            assert np.all(excess <= 0), (pattern, trans, float(excess.max()))
            # the sum of a (row, column) depends on the pattern alone: a narrower block gives the same columns
            assert np.array_equal(_rhs(hs, A, E, X[:, 8:17], trans, pattern), got[:, 8:17])


# ---- b. the row square sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["Float64", "ComplexF64"])
def test_rowsq_kernel_columns_fed_in_two_calls_give_the_bits_of_one(hs, cplx):
    n = 300  # more than one workgroup, not a multiple of 64
    X = _rand(n, 33, cplx, 5)
    a0 = np.abs(_rand(n, 1, False, 6)[:, 0])
    whole = _rowsq(hs, X, a0, ld=n + 3)
    part = _rowsq(hs, X[:, 20:], _rowsq(hs, X[:, :20], a0), ld=n + 3)
    assert np.array_equal(whole, part)
    assert np.array_equal(whole, GM.rowsq(X, a0))
    assert np.array_equal(_rowsq(hs, X[:1, :1], a0[:1]), GM.rowsq(X[:1, :1], a0[:1]))


# ---- c. hs.tangent -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax", SMALL)
def test_tangent_is_the_block_solve_of_the_kernel_right_hand_side(hs, kind, shape, nmax):
    c = _get(hs, kind, shape, nmax)
    F, A, n, rows = c["F"], c["A"], c["n"], c["rows"]
    for trans in (0, 1, 2):
        op = _op(hs, F, trans)
        for k in KS:
            for pattern in ("A", "diag") if k == 5 else ("A",):
                B, E = _rand(n, k, c["cplx"], 10 * trans + k), _dir(c, pattern, 30 + trans)
                dX, X = hs.tangent(op, B, E, pattern=pattern, want="X")
                assert dX.shape == (n, k) and dX.dtype == F.dtype
                assert np.array_equal(X, hs.ldiv_block_t(op, B)), (trans, k)
                P = _rhs(hs, A, E, X, trans, pattern)
                assert np.array_equal(dX, hs.ldiv_block_t(op, P)), (trans, k, pattern)
                assert hs.gn_info(F)["block_solves"] == 2 and hs.gn_info(F)["groups"] == 1
                dXr = hs.tangent(op, B, E, rows=rows, pattern=pattern)
                assert dXr.shape == (len(rows), k) and np.array_equal(dXr, dX[rows]), (trans, k, pattern)
                assert np.array_equal(hs.tangent(op, None, E, rows=rows, pattern=pattern, X=X), dXr)
                assert hs.gn_info(F)["block_solves"] == 1
    # no columns, no rows: empty results
    assert hs.tangent(F, np.zeros((n, 0)), _dir(c, "A", 1)).shape == (n, 0)
    assert hs.tangent(F, _rand(n, 2, c["cplx"], 1), _dir(c, "A", 1), rows=[]).shape == (0, 2)


# ---- d. hs.gn_hessvec ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax", SMALL)
def test_hessvec_is_the_sensitivity_of_the_scattered_tangent(hs, kind, shape, nmax):
    c = _get(hs, kind, shape, nmax)
    F, A, n, rows = c["F"], c["A"], c["n"], c["rows"]
    pos = SM.diag_positions(A)
    assert np.all(pos >= 0)
    for trans in (0, 1, 2):
        op = _op(hs, F, trans)
        for k in KS:
            B, E = _rand(n, k, c["cplx"], 50 + 10 * trans + k), _dir(c, "A", 70 + trans)
            HE, JE, X = hs.gn_hessvec(op, B, rows, E, want=("JE", "X"))
            assert HE.shape == (A.nnz,) and HE.dtype == F.dtype and JE.shape == (len(rows), k)
            assert np.array_equal(HE, hs.sensitivity(op, B, SM.scatter(rows, JE, n))), (trans, k)
            assert np.array_equal(JE, hs.tangent(op, B, E, rows=rows)), (trans, k)
            assert np.array_equal(X, hs.ldiv_block_t(op, B))
            assert np.array_equal(hs.gn_hessvec(op, B, rows, E), HE)
            Ed = _dir(c, "diag", 90 + trans)
            Hdiag = hs.gn_hessvec(op, B, rows, Ed, pattern="diag")
            assert Hdiag.shape == (n,) and np.array_equal(Hdiag, hs.gn_hessvec(op, B, rows, GM.embed(A, Ed, "diag"))[pos]), (trans, k)
    Z = hs.sensitivity_matrix(F, HE)
    assert np.array_equal(Z.indptr, A.indptr) and np.array_equal(Z.data, HE)
    H0 = hs.gn_hessvec(F, np.zeros((n, 0)), rows, E)
    assert H0.shape == HE.shape and not H0.any()
    H0, J0 = hs.gn_hessvec(F, B, [], E, want="JE")
    assert not H0.any() and J0.shape == (0, B.shape[1])


# ---- e. determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax", SMALL)
def test_same_bits_over_calls_group_widths_supplied_fields_and_sparse_blocks(hs, kind, shape, nmax, monkeypatch):
    c = _get(hs, kind, shape, nmax)
    F, A, n, rows = c["F"], c["A"], c["n"], c["rows"]
    k = 40
    Bs = sources(n, k, "anywhere", None, c["cplx"], 7, empty=11)
    for trans in (0, 1, 2):
        op = _op(hs, F, trans)
        B, E = _rand(n, k, c["cplx"], 110 + trans), _dir(c, "A", 120 + trans)
        HE, JE, X = hs.gn_hessvec(op, B, rows, E, want=("JE", "X"))
        info = hs.gn_info(F)
        assert info["groups"] == 1 and info["block_solves"] == 3 and info["workspace_bytes"] > 0
        again = hs.gn_hessvec(op, B, rows, E, want=("JE", "X"))
        assert all(np.array_equal(a, b) for a, b in zip(again, (HE, JE, X)))
        dX = hs.tangent(op, B, E)
        monkeypatch.setenv("HS_GN_GROUP", "32")
        g32 = hs.gn_hessvec(op, B, rows, E, want=("JE", "X"))
        groups = -(-k // (-(-32 // _kc()) * _kc()))
        assert groups == 2 or _kc() != 32
        info = hs.gn_info(F)
        assert info["groups"] == groups and info["block_solves"] == 3 * groups
        x32 = hs.gn_hessvec(op, None, rows, E, X=X, want="JE")
        info = hs.gn_info(F)
        assert info["groups"] == groups and info["block_solves"] == 2 * groups
        d32 = hs.tangent(op, B, E)
        monkeypatch.delenv("HS_GN_GROUP")
        assert all(np.array_equal(a, b) for a, b in zip(g32, (HE, JE, X))), trans
        assert np.array_equal(x32[0], HE) and np.array_equal(x32[1], JE) and np.array_equal(d32, dX), trans
        hx = hs.gn_hessvec(op, B, rows, E, X=X)
        assert np.array_equal(hx, HE) and hs.gn_info(F)["block_solves"] == 2
        # a sparse B gives the bits of its dense expansion
        Hs = hs.gn_hessvec(op, Bs, rows, E, want=("JE", "X"))
        Hd = hs.gn_hessvec(op, Bs.toarray(), rows, E, want=("JE", "X"))
        assert all(np.array_equal(a, b) for a, b in zip(Hs, Hd)), trans
        assert np.array_equal(hs.tangent(op, Bs, E), hs.tangent(op, Bs.toarray(), E))
        assert not Hs[2][:, 11].any() and not Hs[1][:, 11].any()


# ---- f. the identities on the device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax", SMALL)
def test_adjoint_identity_and_symmetry_on_the_device(hs, kind, shape, nmax):
    c = _get(hs, kind, shape, nmax)
    F, A, n, rows = c["F"], c["A"], c["n"], c["rows"]
    for trans in (0, 1, 2):
        op = _op(hs, F, trans)
        for k in (5, 40):
            B, W = _rand(n, k, c["cplx"], 130 + trans), _rand(n, k, c["cplx"], 140 + trans)
            E1, E2 = _dir(c, "A", 150 + trans), _dir(c, "A", 160 + trans)
            dX, X = hs.tangent(op, B, E1, want="X")
            G = hs.sensitivity(op, B, W)
            rel = abs(float(np.real(np.vdot(W, dX))) - float(np.real(np.sum(E1 * np.conj(G))))) / (np.linalg.norm(W) * np.linalg.norm(dX))
            H1, J1 = hs.gn_hessvec(op, None, rows, E1, X=X, want="JE")
            H2, J2 = hs.gn_hessvec(op, None, rows, E2, X=X, want="JE")
            jj, scale = float(np.real(np.vdot(J1, J2))), np.linalg.norm(J1) * np.linalg.norm(J2)
            r12, r21 = abs(float(np.real(np.vdot(H2, E1))) - jj) / scale, abs(float(np.real(np.vdot(H1, E2))) - jj) / scale
            print(f"{kind} trans={trans} k={k}: adjoint identity {rel:.2e}, symmetry {r12:.2e} / {r21:.2e} (bound {2 * TOL:.0e})")
            assert rel <= 2 * TOL and r12 <= 2 * TOL and r21 <= 2 * TOL


# ---- g. the conventions end to end, against the mirror with SuperLU solves -----------------------------------------------------------------
def _relerr(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("kind,shape,nmax", [EXACT[0], EXACT[1], EXACT[3]])
def test_against_the_mirror_with_superlu_solves(hs, kind, shape, nmax):
    """Bound TOL (the per-column solve tolerance of test_ldiv_block_gpu.py).  The chained composition of the entry points this replaces
    (hs.ldiv_block_t, a SciPy product, hs.ldiv_block_t) is measured beside it against the same reference: 9.2e-16 to 1.6e-15 (real 30 x 27),
    8.6e-15 to 1.0e-14 (complex 30 x 27) and 7.6e-14 to 1.2e-13 (complex 24^3) on the MI355X, below TOL on every handle, so TOL stands.  The
    device path measured the same figures for dX, and at most 2.0e-13 for HE."""
    c = _get(hs, kind, shape, nmax)
    F, A, n, rows = c["F"], c["A"], c["n"], c["rows"]
    solve = SM.superlu_solver(A)
    k = 5
    for trans in (0, 1, 2):
        op = _op(hs, F, trans)
        for pattern in ("A", "diag") if trans == 0 else ("A",):
            B, E = _rand(n, k, c["cplx"], 170 + trans), _dir(c, pattern, 180 + trans)
            HEref, JEref, Xref = GM.gn_hessvec(A, solve, B, rows, E, trans, pattern)
            dXref = GM.tangent(A, solve, B, E, trans, pattern, X=Xref)[0]
            dX = hs.tangent(op, B, E, pattern=pattern)
            HE, JE = hs.gn_hessvec(op, B, rows, E, pattern=pattern, want="JE")
            chained = -hs.ldiv_block_t(op, np.asarray(GM.op_matrix(A, E, trans, pattern) @ hs.ldiv_block_t(op, B)))
            e_dx, e_he, e_je, e_ch = _relerr(dX, dXref), _relerr(HE, HEref), _relerr(JE, JEref), _relerr(chained, dXref)
            print(f"{kind} {shape} trans={trans} pattern={pattern}: dX {e_dx:.2e}, JE {e_je:.2e}, HE {e_he:.2e}; the chained host composition {e_ch:.2e} (bound {TOL:.0e})")
            assert e_dx <= TOL and e_je <= TOL and e_he <= TOL, (trans, pattern)


def test_compressed_handle_with_refined_solves(hs):
    """The bounds of test_compressed_handles (test_sens_gpu.py): the blocks are the lockstep refinement's bit for bit, and HE is the sum over
    the returned blocks within the inner-product bound."""
    label, kind, shape, nmax, kw = COMPRESSED[0]
    c = _get(hs, kind, shape, nmax, label, **kw)
    F, A, n, rows = c["F"], c["A"], c["n"], c["rows"]
    assert hs.maxrank(F) > 0
    trans, k, itmax = 2, 5, 2
    op = _op(hs, F, trans)
    B, E = _rand(n, k, c["cplx"], 190), _dir(c, "A", 191)
    HE, JE, X = hs.gn_hessvec(op, B, rows, E, itmax=itmax, want=("JE", "X"))
    assert hs.gn_info(F)["block_solves"] == 3
    assert np.array_equal(X, hs.ldiv_refine_block(op, B, itmax=itmax, ferr=False)[0])
    dX = hs.tangent(op, B, E, itmax=itmax)
    assert np.array_equal(dX, hs.ldiv_refine_block(op, _rhs(hs, A, E, X, trans), itmax=itmax, ferr=False)[0])
    assert np.array_equal(JE, dX[rows])
    G, Xs, Lam = hs.sensitivity(op, B, SM.scatter(rows, JE, n), itmax=itmax, want=("X", "Lam"))
    assert np.array_equal(HE, G)
    ref, S = SM.reduce(A, Lam, Xs, trans), SM.bound(A, Lam, Xs, trans)
    assert np.all(np.abs(HE - ref) <= 4 * (k + 4) * EPS * S)
    Bsp = sources(n, k, "anywhere", None, c["cplx"], 9)
    assert np.array_equal(hs.gn_hessvec(op, Bsp, rows, E, itmax=itmax), hs.gn_hessvec(op, Bsp.toarray(), rows, E, itmax=itmax))


# ---- h. hs.gn_diag -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax", SMALL)
def test_diagonal_of_the_gauss_newton_product(hs, kind, shape, nmax, monkeypatch):
    c = _get(hs, kind, shape, nmax)
    F, A, n, rows = c["F"], c["A"], c["n"], c["rows"]
    pos = SM.diag_positions(A)
    nr = len(rows)
    S = sp.csc_matrix((np.ones(nr), (rows, np.arange(nr))), shape=(n, nr))
    rng = np.random.default_rng(3)
    for trans in (0, 1, 2):
        op = _op(hs, F, trans)
        for k in (5, 40):
            B = _rand(n, k, c["cplx"], 200 + trans)
            Hd, z2, x2 = hs.gn_diag(op, B, rows, factors=True)
            assert Hd.dtype == np.float64 and Hd.shape == (A.nnz,)
            info = hs.gn_info(F)
            assert info["groups"] == 2 and info["block_solves"] == 2
            X = hs.ldiv_block_t(op, B)
            Lam = hs.sensitivity(op, np.zeros((n, nr)), S, want="Lam")[1]  # the adjoint states of the unit columns
            assert np.array_equal(x2, GM.rowsq(X)) and np.array_equal(z2, GM.rowsq(Lam)), (trans, k)
            assert np.array_equal(Hd, GM.diag_from(A, z2, x2, trans)), (trans, k)
            assert np.array_equal(hs.gn_diag(op, B, rows), Hd)
            assert np.array_equal(hs.gn_diag(op, None, rows, X=X), Hd) and hs.gn_info(F)["block_solves"] == 1
            assert np.array_equal(hs.gn_diag(op, B, rows, pattern="diag"), Hd[pos])
            if k == 40:
                monkeypatch.setenv("HS_GN_GROUP", "32")
                h32 = hs.gn_diag(op, B, rows, factors=True)
                assert hs.gn_info(F)["groups"] == -(-k // (-(-32 // _kc()) * _kc())) + 1
                monkeypatch.delenv("HS_GN_GROUP")
                assert all(np.array_equal(a, b) for a, b in zip(h32, (Hd, z2, x2)))
            else:
                for p in rng.choice(A.nnz, size=4, replace=False):
                    e = np.zeros(A.nnz, dtype=F.dtype)
                    e[p] = 1
                    hp = float(np.real(hs.gn_hessvec(op, None, rows, e, X=X)[p]))
                    assert abs(hp - Hd[p]) <= 2 * TOL * Hd[p], (trans, p, hp, Hd[p])
    Hd0, z0, x0 = hs.gn_diag(F, B, [], factors=True)
    assert not Hd0.any() and not z0.any() and not x0.any()


# ---- i. refusals, the device entry points --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,nmax,kw", [((24, 24, 24), 300, dict(mf=2, leafsize=128)), ((32, 32, 32), 512, dict(hss_min=1024))], ids=["mf2", "hss_min"])
def test_handles_the_transposed_block_solve_refuses(hs, shape, nmax, kw):
    E = hs._lib
    lib = E.lib()
    P = prepare(hs, shape, kind="convdiff", nmax=nmax, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, **kw)
    n, nnz = P["A"].shape[0], SM.canonical(P["A"]).nnz
    B = np.asfortranarray(_rand(n, 3, False, 1))
    Ev = _rand(nnz, 1, False, 2)[:, 0]
    for op in (F, hs.transpose(F), hs.adjoint(F)):
        with pytest.raises(hs.UnsupportedError, match="HSS.*node|node.*HSS"):
            hs.tangent(op, B, Ev)
        with pytest.raises(hs.UnsupportedError, match="HSS.*node|node.*HSS"):
            hs.gn_hessvec(op, B, [0, 1], Ev)
        with pytest.raises(hs.UnsupportedError, match="HSS.*node|node.*HSS"):
            hs.gn_diag(op, None, [0, 1], X=B)
    bB = E.hs_block_arg(B.ctypes.data, n, None, None, None)
    out = [np.full(nnz, 42.0), np.full((n, 3), 42.0, order="F"), np.full((2, 3), 42.0, order="F"), np.full(n, 42.0)]
    HE, X, JE, z2 = (a.ctypes.data for a in out)
    pr = np.array([1, 2], dtype=np.int64).ctypes.data_as(E.p_i64)
    for trans in (0, 1, 2):
        assert lib.hs_tangent_d(F._h, trans, n, 3, C.byref(bB), None, n, Ev.ctypes.data, 0, 0, pr, 2, JE, 2, X, n) == E.HS_ERR_UNSUPPORTED
        assert lib.hs_gn_hessvec_d(F._h, trans, n, 3, C.byref(bB), None, n, Ev.ctypes.data, 0, 2, pr, 2, HE, JE, 2, X, n) == E.HS_ERR_UNSUPPORTED
        assert lib.hs_gn_diag_d(F._h, trans, n, 3, C.byref(bB), None, n, pr, 2, 0, 0, HE, z2, z2) == E.HS_ERR_UNSUPPORTED
    assert all(np.all(a == 42.0) for a in out)
    F.free()


def test_argument_and_dimension_refusals(hs):
    E = hs._lib
    lib = E.lib()
    c = _get(hs, *EXACT[0])
    F, A, n = c["F"], c["A"], c["n"]
    B = np.asfortranarray(_rand(n, 3, False, 3))
    Ev = _dir(c, "A", 4)
    with pytest.raises(ValueError, match="twice"):
        hs.gn_hessvec(F, B, [3, 8, 3], Ev)
    with pytest.raises(ValueError, match="twice"):
        hs.tangent(F, B, Ev, rows=[3, 8, 3])
    with pytest.raises(ValueError, match="twice"):
        hs.gn_diag(F, B, [3, 8, 3])
    with pytest.raises(TypeError, match="MethodError"):
        hs.tangent(F, B + 1j, Ev)
    with pytest.raises(hs.DimensionMismatch):
        hs.tangent(F, B, Ev[:-1])
    with pytest.raises(hs.DimensionMismatch):
        hs.gn_hessvec(F, B, [0, n], Ev)
    bB = E.hs_block_arg(B.ctypes.data, n, None, None, None)
    out = dict(HE=np.full(A.nnz, 42.0), JE=np.full((3, 3), 42.0, order="F"), X=np.full((n, 3), 42.0, order="F"), dX=np.full((n, 3), 42.0, order="F"))
    rows1 = np.array([5, 1, 9], dtype=np.int64)

    def hv(trans=0, n_=n, bB_=bB, Xin=None, ldxin=n, E_=Ev, pattern=0, itmax=0, rows_=rows1, nrows=3, HE=out["HE"], ldje=3, ldx=n):
        return lib.hs_gn_hessvec_d(F._h, trans, n_, 3, None if bB_ is None else C.byref(bB_), Xin, ldxin, None if E_ is None else E_.ctypes.data, pattern, itmax,
                                   None if rows_ is None else rows_.ctypes.data_as(E.p_i64), nrows, None if HE is None else HE.ctypes.data, out["JE"].ctypes.data, ldje,
                                   out["X"].ctypes.data, ldx)

    def tg(rows_=None, nrows=0, lddx=n, dX=out["dX"]):
        return lib.hs_tangent_d(F._h, 0, n, 3, C.byref(bB), None, n, Ev.ctypes.data, 0, 0, None if rows_ is None else rows_.ctypes.data_as(E.p_i64), nrows,
                                None if dX is None else dX.ctypes.data, lddx, None, n)

    A_, D_ = E.HS_ERR_ARGUMENT, E.HS_ERR_DIMENSION
    assert hv(trans=3) == A_ and hv(pattern=2) == A_ and hv(itmax=-1) == A_ and hv(HE=None) == A_ and hv(E_=None) == A_ and hv(rows_=None) == A_
    assert hv(bB_=None) == A_ and "both NULL" in lib.hs_last_error().decode()
    assert hv(rows_=np.array([5, 1, 5], dtype=np.int64)) == A_ and "twice" in lib.hs_last_error().decode()
    assert hv(bB_=E.hs_block_arg(None, 0, None, None, None)) == A_
    cp, rv, val = np.array([1, 3, 3, 3], dtype=np.int64), np.array([9, 4], dtype=np.int64), np.ones(2)
    bad = E.hs_block_arg(None, 0, cp.ctypes.data_as(E.p_i64), rv.ctypes.data_as(E.p_i64), val.ctypes.data)
    assert hv(bB_=bad) == A_  # rows of a column not strictly increasing
    assert hv(n_=n - 1) == D_ and hv(ldx=n - 1) == D_ and hv(ldje=2) == D_ and hv(nrows=-1) == D_ and hv(nrows=n + 1) == D_
    assert hv(rows_=np.array([5, 0, 9], dtype=np.int64)) == D_ and hv(rows_=np.array([5, n + 1, 9], dtype=np.int64)) == D_
    assert hv(bB_=E.hs_block_arg(B.ctypes.data, n - 1, None, None, None)) == D_ and hv(bB_=None, Xin=B.ctypes.data, ldxin=n - 1) == D_
    assert tg(dX=None) == A_ and tg(lddx=n - 1) == D_ and tg(rows_=rows1, nrows=3, lddx=2) == D_
    assert lib.hs_gn_hessvec_z(F._h, 0, n, 3, C.byref(bB), None, n, Ev.ctypes.data, 0, 0, rows1.ctypes.data_as(E.p_i64), 3, out["HE"].ctypes.data, None, 3, None,
                               n) == A_  # eltype of F and the blocks differ
    assert lib.hs_gn_diag_d(F._h, 0, n, 3, C.byref(bB), None, n, rows1.ctypes.data_as(E.p_i64), 3, 0, 0, None, None, None) == A_
    assert all(np.all(v == 42.0) for v in out.values())
    rv[:] = [4, 9]
    assert hv(bB_=bad) == E.HS_OK and not np.any(out["HE"] == 42.0)  # the same block, well formed
    assert tg(rows_=rows1, nrows=3, lddx=n) == E.HS_OK and np.all(out["dX"][3:] == 42.0) and not np.any(out["dX"][:3] == 42.0)


def test_device_entry_points_on_a_side_stream(hs):
    import torch

    c = _get(hs, *EXACT[1])
    F, A, n, rows = c["F"], c["A"], c["n"], c["rows"]
    nnz, nr = A.nnz, len(rows)
    E = hs._lib
    lib = E.lib()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    k, ld = 37, n + 3
    B, Ev = _rand(n, k, True, 11), _dir(c, "A", 12)

    def up(M, ld_):
        t = torch.zeros((M.shape[1], ld_), dtype=torch.complex128, device=dev)  # row j = column j of the column-major block
        t[:, : M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)
        return t

    def full(shape, dtype=torch.complex128):
        return torch.full(shape, 7.0, dtype=dtype, device=dev)

    dB, dE = up(B, ld), torch.from_numpy(Ev).to(dev)
    bB = E.hs_block_arg(dB.data_ptr(), ld, None, None, None)
    rows1 = np.ascontiguousarray(rows, dtype=np.int64) + 1
    pr = rows1.ctypes.data_as(E.p_i64)
    for trans in (0, 1, 2):
        op = _op(hs, F, trans)
        HE, JE, X = hs.gn_hessvec(op, B, rows, Ev, want=("JE", "X"))
        dX = hs.tangent(op, B, Ev)
        Hd, z2, x2 = hs.gn_diag(op, B, rows, factors=True)
        dHE, dJE, dXf, ddX = full((nnz,)), full((k, nr + 2)), full((k, ld)), full((k, ld))
        with torch.cuda.stream(s):
            E.check(lib.hs_gn_hessvec_dev_z(F._h, trans, n, k, C.byref(bB), None, 0, dE.data_ptr(), 0, 0, pr, nr, dHE.data_ptr(), dJE.data_ptr(), nr + 2, dXf.data_ptr(), ld,
                                            s.cuda_stream))
            E.check(lib.hs_tangent_dev_z(F._h, trans, n, k, None, dXf.data_ptr(), ld, dE.data_ptr(), 0, 0, None, 0, ddX.data_ptr(), ld, None, 0, s.cuda_stream))
        gj, gx, gd = dJE.cpu().numpy().T, dXf.cpu().numpy().T, ddX.cpu().numpy().T
        assert np.array_equal(dHE.cpu().numpy(), HE) and np.array_equal(gj[:nr], JE) and np.array_equal(gx[:n], X) and np.array_equal(gd[:n], dX), trans
        assert np.all(gj[nr:] == 7.0) and np.all(gx[n:] == 7.0) and np.all(gd[n:] == 7.0)
        dHd, dz2, dx2 = full((nnz,), torch.float64), full((n,), torch.float64), full((n,), torch.float64)
        with torch.cuda.stream(s):
            E.check(lib.hs_gn_diag_dev_z(F._h, trans, n, k, C.byref(bB), None, 0, pr, nr, 0, 0, dHd.data_ptr(), dz2.data_ptr(), dx2.data_ptr(), s.cuda_stream))
        assert np.array_equal(dHd.cpu().numpy(), Hd) and np.array_equal(dz2.cpu().numpy(), z2) and np.array_equal(dx2.cpu().numpy(), x2), trans
