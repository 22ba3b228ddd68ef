"""Adjoint-state sensitivities on A's pattern (hs_sens_*, hs_misfit_*; csrc/hs_sens.hip + csrc/kernels_sens.hip) on the MI355X: the reduction
kernel alone on exact data, the solves bit for bit against the block solves, G against the returned blocks within the inner-product bound
and against SuperLU, determinism over calls, group widths and patterns, the misfit form, compressed handles, refusals and a timing guard.
Problems and option sets are those of test_ldiv_block_gpu.py; one factorization per (kind, options) is shared by the tests of this file."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import sens_mirror as SM
from helpers import prepare
from test_ldiv_block_gpu import COMPRESSED, EXACT, _kc, _rand
from test_ldiv_sparse_host import sources, tree_closure

pytestmark = pytest.mark.gpu

TOL = 1e-10  # per column solve tolerance of test_ldiv_block_gpu.py and test_ldiv_sparse_gpu.py
EPS = float(np.finfo(np.float64).eps)
KS = (1, 5, 40, 70)
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
        owner, parent = tree_closure(P["nd"], n)
        leaves = [i for i in range(len(parent)) if i not in set(parent)]
        _CACHE[key] = dict(P=P, F=F, A=A, n=n, leaf=np.flatnonzero(owner == leaves[1]), far=np.flatnonzero(owner == leaves[-2]), runs={}, solve=None)
    return _CACHE[key]


def _op(hs, F, trans):
    return (F, hs.transpose(F), hs.adjoint(F))[trans]


def _lam_by_block_solves(hs, F, W, trans):
    """The right-hand column of the table in include/hs_solver.h through hs.ldiv_block_t."""
    if trans == 0:
        return hs.ldiv_block_t(hs.adjoint(F), W)
    if trans == 1:
        return np.conj(hs.ldiv_block_t(F, np.conj(W)))
    return hs.ldiv_block_t(F, W)


def _run(hs, c, trans, k, itmax=0):
    """One dense call with both blocks returned; computed once per (trans, k) and left unchanged."""
    key = (trans, k, itmax)
    if key not in c["runs"]:
        F, n = c["F"], c["n"]
        cplx = F.dtype.kind == "c"
        B, W = _rand(n, k, cplx, 100 * trans + k), _rand(n, k, cplx, 100 * trans + k + 1)
        G, X, Lam = hs.sensitivity(_op(hs, F, trans), B, W, itmax=itmax, want=("X", "Lam"))
        c["runs"][key] = dict(B=B, W=W, G=G, X=X, Lam=Lam, info=hs.sens_info(F))
    return c["runs"][key]


# ---- a. the kernel's lane map, exact ---------------------------------------------------------------------------------------------------
def _pattern70():
    """n = 70: column 5 empty, column 9 dense (70 entries: more than one wave), (12, 12) missing, nnz not a multiple of 64."""
    n = 70
    rng = np.random.default_rng(1)
    M = (rng.random((n, n)) < 0.08) | np.eye(n, dtype=bool)
    M[:, 5] = False
    M[:, 9] = True
    M[12, 12] = False
    if M.sum() % 64 == 0:
        M[0, 1] = not M[0, 1]
    A = sp.csc_matrix(M.astype(np.float64))
    A.sort_indices()
    assert A.nnz % 64 != 0 and A.indptr[6] == A.indptr[5] and A.indptr[10] - A.indptr[9] == 70
    return A


def _sddmm(hs, A, L, R, kc, swap=0, conjl=0, conjr=0, diag=0, form=0, G0=None, ld=None):
    n = A.shape[0]
    cplx = np.iscomplexobj(L)
    dt = np.complex128 if cplx else np.float64
    ld = ld or n
    Lp, Rp = np.full((ld, kc), 99, dtype=dt, order="F"), np.full((ld, kc), 77, dtype=dt, order="F")  # the padding rows are never read
    Lp[:n], Rp[:n] = L[:, :kc], R[:, :kc]
    cp = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rv = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    G = np.ascontiguousarray(G0, dtype=dt).copy()
    E = hs._lib
    fn = E.lib().hsk_sddmm_z if cplx else E.lib().hsk_sddmm_d
    E.check(fn(n, cp.ctypes.data_as(E.p_i64), rv.ctypes.data_as(E.p_i64), kc, Lp.ctypes.data, ld, Rp.ctypes.data, ld, swap, conjl, conjr, diag, form, G.ctypes.data, None))
    return G


def _sddmm_numpy(A, L, R, kc, swap, conjl, conjr, G0):
    i, j = SM.entry_index(A)
    a, b = (j, i) if swap else (i, j)
    l = np.conj(L[a, :kc]) if conjl else L[a, :kc]
    r = np.conj(R[b, :kc]) if conjr else R[b, :kc]
    return G0 - (l * r).sum(axis=1)


@pytest.mark.parametrize("cplx", [False, True], ids=["Float64", "ComplexF64"])
def test_kernel_lane_map_is_exact_on_small_integers(hs, cplx):
    rng = np.random.default_rng(2)

    def ints(shape):
        M = rng.integers(-3, 4, size=shape).astype(np.float64)
        return M + 1j * rng.integers(-3, 4, size=shape) if cplx else M

    A = _pattern70()
    n = A.shape[0]
    L, R = ints((n, 33)), ints((n, 33))
    G0 = ints(A.nnz)
    pos = SM.diag_positions(A)
    assert pos[5] == -1 and pos[12] == -1 and (pos >= 0).sum() == n - 2
    flags = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]
    for kc in (1, 3, 16, 33):
        for swap, cl, cr in flags:
            want = _sddmm_numpy(A, L, R, kc, swap, cl, cr, G0)
            for form in (0, 1):
                got = _sddmm(hs, A, L, R, kc, swap, cl, cr, 0, form, G0, ld=n + 3)
                assert np.array_equal(got, want), (kc, swap, cl, cr, form)
            # the diagonal mode: the chain of (j, j) from its own initial value, 0 where the entry is absent
            d0 = ints(n)
            wd = np.zeros(n, dtype=want.dtype)
            wd[pos >= 0] = (_sddmm_numpy(A, L, R, kc, swap, cl, cr, np.zeros(A.nnz)) + 0)[pos[pos >= 0]] + d0[pos >= 0]
            assert np.array_equal(_sddmm(hs, A, L, R, kc, swap, cl, cr, 1, 0, d0, ld=n + 3), wd), (kc, swap, cl, cr, "diag")
    # n = 1: one stored entry, and none
    one = sp.csc_matrix(np.ones((1, 1)))
    l1, r1 = ints((1, 33)), ints((1, 33))
    for kc in (1, 33):
        assert np.array_equal(_sddmm(hs, one, l1, r1, kc, 0, 1, 1, 0, 0, np.array([5.0])), _sddmm_numpy(one, l1, r1, kc, 0, 1, 1, np.array([5.0])))
        assert np.array_equal(_sddmm(hs, one, l1, r1, kc, 1, 0, 0, 1, 0, np.array([5.0])), _sddmm_numpy(one, l1, r1, kc, 1, 0, 0, np.array([5.0])))
    none = sp.csc_matrix((1, 1))
    assert np.array_equal(_sddmm(hs, none, l1, r1, 3, 0, 0, 0, 1, 0, np.array([5.0])), [0.0])


@pytest.mark.parametrize("cplx", [False, True], ids=["Float64", "ComplexF64"])
def test_kernel_columns_fed_in_two_calls_give_the_bits_of_one(hs, cplx):
    A = _pattern70()
    n = A.shape[0]
    L, R = _rand(n, 33, cplx, 3), _rand(n, 33, cplx, 4)  # rounding in every step: the order of the chain shows in the bits
    G0 = _rand(A.nnz, 1, cplx, 5)[:, 0]
    d0 = _rand(n, 1, cplx, 6)[:, 0]
    for form in (0, 1):
        for swap, cl, cr in ((0, 0, 1), (1, 1, 0)):
            whole = _sddmm(hs, A, L, R, 33, swap, cl, cr, 0, form, G0, ld=n + 3)
            part = _sddmm(hs, A, L, R, 20, swap, cl, cr, 0, form, G0)
            part = _sddmm(hs, A, L[:, 20:], R[:, 20:], 13, swap, cl, cr, 0, form, part, ld=n + 3)
            assert np.array_equal(whole, part), (form, swap)
            assert np.array_equal(whole, _sddmm(hs, A, L, R, 33, swap, cl, cr, 0, 0, G0))  # both forms run one chain
            assert np.allclose(whole, _sddmm_numpy(A, L, R, 33, swap, cl, cr, G0), rtol=1e-12, atol=1e-12)
    dw = _sddmm(hs, A, L, R, 33, 0, 0, 1, 1, 0, d0)
    dp = _sddmm(hs, A, L[:, 20:], R[:, 20:], 13, 0, 0, 1, 1, 0, _sddmm(hs, A, L, R, 20, 0, 0, 1, 1, 0, d0))
    assert np.array_equal(dw, dp)


# ---- b. the solves are the block solves --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_returned_blocks_carry_the_bits_of_the_block_solves(hs, kind, shape, nmax):
    c = _get(hs, kind, shape, nmax)
    F, n = c["F"], c["n"]
    cplx = F.dtype.kind == "c"
    for trans in (0, 1, 2):
        for k in KS:
            r = _run(hs, c, trans, k)
            assert r["X"].shape == (n, k) and r["G"].shape == (c["A"].nnz,) and r["G"].dtype == F.dtype
            assert np.array_equal(r["X"], hs.ldiv_block_t(_op(hs, F, trans), r["B"])), (trans, k)
            assert np.array_equal(r["Lam"], _lam_by_block_solves(hs, F, r["W"], trans)), (trans, k)
    # a sparse B or W gives the bits of its dense expansion, G included
    i = 0
    for trans in (0, 1, 2):
        for k, empty in ((5, None), (40, 7)):
            Bs = sources(n, k, "leaf", c["leaf"], cplx, 20 + i, empty)
            Ws = sources(n, k, "anywhere", c["leaf"], cplx, 40 + i, None if empty is None else 3)
            op = _op(hs, F, trans)
            Gd, Xd, Ld = hs.sensitivity(op, Bs.toarray(), Ws.toarray(), want=("X", "Lam"))
            for Bv, Wv in ((Bs, Ws), (Bs, Ws.toarray()), (Bs.toarray(), Ws)):
                G, X, Lam = hs.sensitivity(op, Bv, Wv, want=("X", "Lam"))
                assert np.array_equal(X, Xd) and np.array_equal(Lam, Ld) and np.array_equal(G, Gd), (trans, k)
            assert np.array_equal(Xd, hs.ldiv_block_t(op, Bs.toarray().astype(F.dtype)))
            i += 1
    # want selects what comes back; no columns: G = 0
    r = _run(hs, c, 0, 5)
    assert np.array_equal(hs.sensitivity(F, r["B"], r["W"]), r["G"])
    G, Lam = hs.sensitivity(F, r["B"], r["W"], want="Lam")
    assert np.array_equal(Lam, r["Lam"])
    G0 = hs.sensitivity(F, np.zeros((n, 0)), np.zeros((n, 0)))
    assert G0.shape == r["G"].shape and not G0.any()
    Z = hs.sensitivity_matrix(F, r["G"])
    assert np.array_equal(Z.indptr, c["A"].indptr) and np.array_equal(Z.indices, c["A"].indices) and np.array_equal(Z.data, r["G"])


# ---- c. G against the returned blocks ----------------------------------------------------------------------------------------------------
def _check_against_blocks(c, r, trans, k):
    ref = SM.reduce(c["A"], r["Lam"], r["X"], trans)
    S = SM.bound(c["A"], r["Lam"], r["X"], trans)
    excess = np.abs(r["G"] - ref) - 4 * (k + 4) * EPS * S
    assert np.all(excess <= 0), (trans, k, float(excess.max()))
    return float((np.abs(r["G"] - ref) / np.where(S > 0, S, 1.0)).max() / EPS)


@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_G_is_the_sum_over_the_returned_blocks(hs, kind, shape, nmax):
    c = _get(hs, kind, shape, nmax)
    for trans in (0, 1, 2):
        for k in KS:
            w = _check_against_blocks(c, _run(hs, c, trans, k), trans, k)
            print(f"{kind} {shape} trans={trans} k={k}: worst |G - G_numpy| / S = {w:.2f} eps (bound {4 * (k + 4)} eps)")


# ---- d. G against SuperLU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_G_against_superlu(hs, kind, shape, nmax):
    c = _get(hs, kind, shape, nmax)
    solve = SM.superlu_solver(c["A"])
    for trans in (0, 1, 2):
        for k in (5, 40):  # the SuperLU solves are the time of this test
            r = _run(hs, c, trans, k)
            Gref, Xref, Lref = SM.sensitivity(c["A"], solve, r["B"], r["W"], trans)
            S = SM.bound(c["A"], Lref, Xref, trans)
            err = float(np.abs(r["G"] - Gref).max())
            print(f"{kind} {shape} trans={trans} k={k}: max |G - G_ref| = {err:.3e}, bound {2 * TOL * S.max():.3e}")
            assert err <= 2 * TOL * float(S.max()), (trans, k)


# ---- e. determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_same_bits_over_calls_group_widths_and_patterns(hs, kind, shape, nmax, monkeypatch):
    c = _get(hs, kind, shape, nmax)
    F = c["F"]
    pos = SM.diag_positions(c["A"])
    assert np.all(pos >= 0)
    for trans in (0, 1, 2):
        r = _run(hs, c, trans, 70)
        op = _op(hs, F, trans)
        assert r["info"]["groups"] == 1 and r["info"]["products"] == c["A"].nnz * 70
        G, X, Lam = hs.sensitivity(op, r["B"], r["W"], want=("X", "Lam"))
        assert np.array_equal(G, r["G"]) and np.array_equal(X, r["X"]) and np.array_equal(Lam, r["Lam"])
        monkeypatch.setenv("HS_SENS_GROUP", "32")
        G32 = hs.sensitivity(op, r["B"], r["W"])
        assert hs.sens_info(F)["groups"] == -(-70 // (-(-32 // _kc()) * _kc()))
        monkeypatch.delenv("HS_SENS_GROUP")
        assert np.array_equal(G32, r["G"]), trans
        d = hs.sensitivity(op, r["B"], r["W"], pattern="diag")
        assert d.shape == (c["n"],) and np.array_equal(d, r["G"][pos]), trans
        assert hs.sens_info(F)["products"] == c["n"] * 70


# ---- f. the misfit form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_misfit_is_the_sensitivity_of_the_scattered_residual(hs, kind, shape, nmax):
    c = _get(hs, kind, shape, nmax)
    F, n = c["F"], c["n"]
    cplx = F.dtype.kind == "c"
    rng = np.random.default_rng(9)
    spread = np.concatenate([rng.choice(c["far"], 3, replace=False), rng.choice(c["leaf"], 3, replace=False), [n - 1, 0]])  # over the tree, unsorted
    spread = spread[np.sort(np.unique(spread, return_index=True)[1])]
    i = 0
    for trans in (0, 1, 2):
        for k, rows in ((5, rng.permutation(c["leaf"])[:6]), (40, spread)):
            op = _op(hs, F, trans)
            B = sources(n, k, "leaf", c["leaf"], cplx, 60 + i) if i % 2 else _rand(n, k, cplx, 60 + i)
            D = _rand(len(rows), k, cplx, 80 + i)
            J, G, R = hs.misfit(op, B, rows, D, want_residual=True)
            X = hs.ldiv_block_t(op, B.toarray().astype(F.dtype) if sp.issparse(B) else B)
            assert np.array_equal(R, X[rows] - D), (trans, k)
            Jref = 0.5 * (np.abs(R) ** 2).sum(axis=0)
            assert np.all(np.abs(J - Jref) <= (len(rows) + 4) * EPS * Jref), (trans, k)
            assert np.array_equal(G, hs.sensitivity(op, B, SM.scatter(rows, R, n))), (trans, k)
            assert np.array_equal(G, hs.sensitivity(op, B, sp.csc_matrix(SM.scatter(rows, R, n)))), (trans, k)
            J2, G2 = hs.misfit(op, B, rows, D)
            assert np.array_equal(J2, J) and np.array_equal(G2, G)
            Jd, Gd = hs.misfit(op, B, rows, D, pattern="diag")
            assert np.array_equal(Gd, G[SM.diag_positions(c["A"])])
            i += 1
    with pytest.raises(ValueError, match="twice"):
        hs.misfit(F, _rand(n, 2, cplx, 1), [3, 8, 3], np.zeros((3, 2)))


# ---- g. compressed handles ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,kind,shape,nmax,kw", COMPRESSED, ids=[x[0] for x in COMPRESSED])
def test_compressed_handles(hs, label, kind, shape, nmax, kw):
    c = _get(hs, kind, shape, nmax, label, **kw)
    F, n = c["F"], c["n"]
    assert hs.maxrank(F) > 0  # low-rank Gauss transforms are in the solves
    trans = [x[0] for x in COMPRESSED].index(label) % 3
    op = _op(hs, F, trans)
    for k in (5, 40):
        r = _run(hs, c, trans, k)
        assert np.array_equal(r["X"], hs.ldiv_block_t(op, r["B"])) and np.array_equal(r["Lam"], _lam_by_block_solves(hs, F, r["W"], trans))
        _check_against_blocks(c, r, trans, k)
    # refined solves: the forward block is the lockstep refinement's, G is the sum over the returned blocks
    r = _run(hs, c, trans, 40, itmax=5)
    assert np.array_equal(r["X"], hs.ldiv_refine_block(op, r["B"], itmax=5, ferr=False)[0])
    _check_against_blocks(c, r, trans, 40)
    cplx = F.dtype.kind == "c"
    Bs, Ws = sources(n, 7, "leaf", c["leaf"], cplx, 3), sources(n, 7, "anywhere", c["leaf"], cplx, 4, empty=2)
    Gs, Xs, Ls = hs.sensitivity(op, Bs, Ws, itmax=5, want=("X", "Lam"))
    Gd, Xd, Ld = hs.sensitivity(op, Bs.toarray(), Ws.toarray(), itmax=5, want=("X", "Lam"))
    assert np.array_equal(Xs, Xd) and np.array_equal(Ls, Ld) and np.array_equal(Gs, Gd)  # expanded on the device: the same block
    rows = c["far"][:5]
    D = _rand(5, 7, cplx, 5)
    J, G, R = hs.misfit(op, Bs, rows, D, itmax=5, want_residual=True)
    assert np.array_equal(R, Xd[rows] - D)
    assert np.array_equal(G, hs.sensitivity(op, Bs, SM.scatter(rows, R, n), itmax=5))


# ---- h. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(hs):
    E = hs._lib
    lib = E.lib()
    P = prepare(hs, (24, 24, 24), kind="convdiff", nmax=300, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    n = P["A"].shape[0]
    nnz = SM.canonical(P["A"]).nnz
    B, W = np.asfortranarray(_rand(n, 3, False, 1)), np.asfortranarray(_rand(n, 3, False, 2))
    for op in (F, hs.transpose(F), hs.adjoint(F)):
        with pytest.raises(hs.UnsupportedError, match="HSS"):
            hs.sensitivity(op, B, W)
        with pytest.raises(hs.UnsupportedError, match="HSS"):
            hs.misfit(op, B, [0, 1], np.zeros((2, 3)))
    bB, bW = E.hs_block_arg(B.ctypes.data, n, None, None, None), E.hs_block_arg(W.ctypes.data, n, None, None, None)
    G = np.full(nnz, 42.0)
    X, Lam = np.full((n, 3), 42.0, order="F"), np.full((n, 3), 42.0, order="F")
    J, R = np.full(3, 42.0), np.full((2, 3), 42.0, order="F")
    rows1 = np.array([1, 2], dtype=np.int64)
    D = np.zeros((2, 3), order="F")
    for trans in (0, 1, 2):
        assert lib.hs_sens_d(F._h, trans, n, 3, C.byref(bB), C.byref(bW), 0, 0, G.ctypes.data, X.ctypes.data, n, Lam.ctypes.data, n) == E.HS_ERR_UNSUPPORTED
        assert lib.hs_misfit_d(F._h, trans, n, 3, C.byref(bB), rows1.ctypes.data_as(E.p_i64), 2, D.ctypes.data, 2, 5, 1, J.ctypes.data, R.ctypes.data, 2,
                               G.ctypes.data) == E.HS_ERR_UNSUPPORTED
    assert np.all(G == 42.0) and np.all(X == 42.0) and np.all(Lam == 42.0) and np.all(J == 42.0) and np.all(R == 42.0)
    F.free()
    c = _get(hs, "convdiff", (30, 27), 40)
    F, n = c["F"], c["n"]
    B, W = _rand(n, 3, False, 3), _rand(n, 3, False, 4)
    with pytest.raises(TypeError, match="MethodError"):
        hs.sensitivity(F, B + 1j, W)  # the dtype rule of ldiv_block
    with pytest.raises(TypeError, match="MethodError"):
        hs.misfit(F, B, [0], np.zeros((1, 3)) + 1j)
    with pytest.raises(hs.DimensionMismatch):
        hs.sensitivity(F, B[:-1], W[:-1])
    with pytest.raises(hs.DimensionMismatch):
        hs.sensitivity(F, B, sp.csc_matrix(W)[:-1])
    with pytest.raises(hs.DimensionMismatch):
        hs.misfit(F, B, [0, n], np.zeros((2, 3)))
    # the C ABI: sizes, flags, a malformed CSC block; every output keeps its sentinel
    Bf, Wf = np.asfortranarray(B), np.asfortranarray(W)
    bB, bW = E.hs_block_arg(Bf.ctypes.data, n, None, None, None), E.hs_block_arg(Wf.ctypes.data, n, None, None, None)
    G = np.full(c["A"].nnz, 42.0)
    X = np.full((n, 3), 42.0, order="F")

    def call(trans=0, n_=n, bB_=bB, bW_=bW, itmax=0, pattern=0, ldx=n, G_=G):
        return lib.hs_sens_d(F._h, trans, n_, 3, C.byref(bB_), C.byref(bW_), itmax, pattern, None if G_ is None else G_.ctypes.data, X.ctypes.data, ldx, None, n)

    assert call(trans=3) == E.HS_ERR_ARGUMENT and call(pattern=2) == E.HS_ERR_ARGUMENT and call(itmax=-1) == E.HS_ERR_ARGUMENT and call(G_=None) == E.HS_ERR_ARGUMENT
    assert call(n_=n - 1) == E.HS_ERR_DIMENSION and call(ldx=n - 1) == E.HS_ERR_DIMENSION
    assert call(bB_=E.hs_block_arg(Bf.ctypes.data, n - 1, None, None, None)) == E.HS_ERR_DIMENSION
    assert call(bW_=E.hs_block_arg(None, 0, None, None, None)) == E.HS_ERR_ARGUMENT
    cp, rv, val = np.array([1, 3, 3, 3], dtype=np.int64), np.array([9, 4], dtype=np.int64), np.ones(2)
    bad = E.hs_block_arg(None, 0, cp.ctypes.data_as(E.p_i64), rv.ctypes.data_as(E.p_i64), val.ctypes.data)
    assert call(bW_=bad) == E.HS_ERR_ARGUMENT  # rows of a column not strictly increasing
    rv[:] = [4, n + 1]
    assert call(bB_=bad) == E.HS_ERR_DIMENSION
    rv[:] = [4, 9]
    assert call(bB_=E.hs_block_arg(None, 0, cp.ctypes.data_as(E.p_i64), rv.ctypes.data_as(E.p_i64), None)) == E.HS_ERR_ARGUMENT
    assert lib.hs_sens_z(F._h, 0, n, 3, C.byref(bB), C.byref(bW), 0, 0, G.ctypes.data, None, n, None, n) == E.HS_ERR_ARGUMENT  # eltype of F and the blocks differ
    assert np.all(G == 42.0) and np.all(X == 42.0)
    assert call(bW_=bad) == E.HS_OK and not np.any(G == 42.0)  # the same block, well formed


def test_device_entry_points_on_a_side_stream(hs):
    import torch

    c = _get(hs, "convdiff_helmholtz", (30, 27), 40)
    F, n, nnz = c["F"], c["n"], c["A"].nnz
    E = hs._lib
    lib = E.lib()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    k, ld = 37, n + 3
    B, W = _rand(n, k, True, 11), _rand(n, k, True, 12)
    rows = np.concatenate([c["far"][:3], c["leaf"][:2]])
    D = _rand(5, k, True, 13)

    def up(M, ld_):
        t = torch.zeros((M.shape[1], ld_), dtype=torch.complex128, device=dev)  # row j = column j of the column-major block
        t[:, : M.shape[0]] = torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)
        return t

    dB, dW, dD = up(B, ld), up(W, ld), up(D, 5)
    for trans in (0, 1, 2):
        op = _op(hs, F, trans)
        G, X, Lam = hs.sensitivity(op, B, W, want=("X", "Lam"))
        J, Gm, R = hs.misfit(op, B, rows, D, want_residual=True)
        dG = torch.full((nnz,), 7.0, dtype=torch.complex128, device=dev)
        dX = torch.full((k, ld), 7.0, dtype=torch.complex128, device=dev)
        dL = torch.full((k, ld), 7.0, dtype=torch.complex128, device=dev)
        bB, bW = E.hs_block_arg(dB.data_ptr(), ld, None, None, None), E.hs_block_arg(dW.data_ptr(), ld, None, None, None)
        with torch.cuda.stream(s):
            E.check(lib.hs_sens_dev_z(F._h, trans, n, k, C.byref(bB), C.byref(bW), 0, 0, dG.data_ptr(), dX.data_ptr(), ld, dL.data_ptr(), ld, s.cuda_stream))
        assert hs.sens_info(F)["values_moved"] == 0
        gx, gl = dX.cpu().numpy().T, dL.cpu().numpy().T
        assert np.array_equal(dG.cpu().numpy(), G) and np.array_equal(gx[:n], X) and np.array_equal(gl[:n], Lam)
        assert np.all(gx[n:] == 7.0) and np.all(gl[n:] == 7.0)
        dJ = torch.zeros(k, dtype=torch.float64, device=dev)
        dR = torch.full((k, 6), 7.0, dtype=torch.complex128, device=dev)
        rows1 = np.ascontiguousarray(rows, dtype=np.int64) + 1
        with torch.cuda.stream(s):
            E.check(lib.hs_misfit_dev_z(F._h, trans, n, k, C.byref(bB), rows1.ctypes.data_as(E.p_i64), 5, dD.data_ptr(), 5, 0, 0, dJ.data_ptr(), dR.data_ptr(), 6,
                                        dG.data_ptr(), s.cuda_stream))
        gr = dR.cpu().numpy().T
        assert np.array_equal(dG.cpu().numpy(), Gm) and np.array_equal(dJ.cpu().numpy(), J) and np.array_equal(gr[:5], R) and np.all(gr[5:] == 7.0)


# ---- i. guard ----------------------------------------------------------------------------------------------------------------------------
def test_the_pipeline_stays_on_the_device(hs):
    """A guard, not a target: by the byte model the reduction and the staging add under 2 % to the two block solves at this shape, so a
    kernel ten times off the model still passes; a failure means the pipeline has left the device or serialised.  Device seconds of
    hs_sens_info against the sum of the device seconds hs_ldiv_block_info reports for the forward and the adjoint block solve of the same
    blocks, all timed in this process, after one warm-up, as a median of 3."""
    P = prepare(hs, (40, 40, 40), kind="poisson", rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
    n = P["A"].shape[0]
    B, W = _rand(n, 32, False, 51), _rand(n, 32, False, 52)
    ts, tf, ta, split = [], [], [], []
    for it in range(4):
        G = hs.sensitivity(F, B, W)
        info = hs.sens_info(F)
        hs.ldiv_block_t(F, B)
        t1 = hs.ldiv_block_info(F)["seconds"]
        hs.ldiv_block_t(hs.adjoint(F), W)
        t2 = hs.ldiv_block_info(F)["seconds"]
        if it > 0:
            ts.append(info["seconds"])
            tf.append(t1)
            ta.append(t2)
            split.append((info["seconds_forward"], info["seconds_adjoint"], info["seconds_reduce"]))
    t_sens, t_solves = float(np.median(ts)), float(np.median(tf)) + float(np.median(ta))
    f, a, r = (float(np.median([x[i] for x in split])) for i in range(3))
    print(f"Poisson 40^3, 32 columns: sensitivity {t_sens * 1e3:.3f} ms (forward {f * 1e3:.3f}, adjoint {a * 1e3:.3f}, reduction {r * 1e3:.3f}), "
          f"the two block solves {t_solves * 1e3:.3f} ms, ratio {t_sens / t_solves:.3f}")
    assert info["groups"] == 1 and info["values_moved"] == 2 * n * 32 + len(G)
    assert t_sens <= 1.25 * t_solves
    F.free()
