"""Solves with A1 = A + U V^H (or A + dA) from the stored factorization of A (hs_mod_*, csrc/hs_mod.hip + kernels_mod.hip) on the MI355X:
the four kernels alone with exact integer data and against the NumPy statement of the summation order (tests/mod_mirror.py), dense and
entry modifications against dense / SuperLU solves of the modified matrix, the bitwise properties, GMRES on a compressed handle
preconditioned by the modified factorization, the refusals, and a timing guard.

Error bound of the modified solves (cases b, c, d): with e0 the worst-column error of hs.ldiv_block_t on the UNMODIFIED system against
SuperLU, measured in the same test, the error must stay below 10 * cond_1(C) * max(e0, eps): the correction solves with the capacitance
matrix C, and the factor 10 covers the two extra products.  The tests build their modifications so that cond_1(C) <= 100 and assert it."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import mod_mirror as MM
from helpers import prepare, relerr

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
EXACT = [("convdiff", (30, 27), 40), ("convdiff_helmholtz", (30, 27), 40), ("convdiff", (24, 24, 24), 300), ("convdiff_helmholtz", (24, 24, 24), 300)]
COMPRESSED = [("tol1e-4", "convdiff_helmholtz", (24, 24, 24), 300, dict(swlevel=2, swsize=8, atol=1e-4, rtol=1e-4))]
USED = [EXACT[0], EXACT[1], EXACT[3]]  # n = 810 real and complex (not a multiple of 64); n = 13824 = 6.75 slabs of 2048
IDS = ["2d-real", "2d-complex", "3d-complex"]
TRANS = ("N", "T", "H")
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for v in _CACHE.values():
        v[1].free()
    _CACHE.clear()


def _problem(hs, kind, shape, nmax, want_lu=True, **kw):
    key = (kind, shape, nmax, tuple(sorted(kw.items())))
    if key not in _CACHE:
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        F = hs.factor(P["A"], P["nd"], P["nd_loc"], **(kw or dict(swlevel=0)))
        _CACHE[key] = (P, F, spla.splu(P["A"]) if want_lu else None)
    return _CACHE[key]


def _rand(n, k, cplx, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    return B + 1j * rng.standard_normal((n, k)) if cplx else B


def _ints(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, shape).astype(float)
    return X + 1j * rng.integers(-3, 4, shape) if cplx else X


def _worst_col(X, R):
    return max(relerr(X[:, j], R[:, j]) for j in range(X.shape[1]))


def _op(F, hs, t):
    return {"N": F, "T": hs.transpose(F), "H": hs.adjoint(F)}[t]


def _lu_trans(lu, B, t):
    return lu.solve(B, trans={"N": "N", "T": "T", "H": "H"}[t])


def _e0(hs, F, lu, B, t):
    """worst-column error of the block solve of the unmodified system against SuperLU"""
    return _worst_col(hs.ldiv_block_t(_op(F, hs, t), B), _lu_trans(lu, B, t))


def _bound(condC, e0):
    return 10.0 * condC * max(e0, EPS)


# ---- a. the kernels alone -----------------------------------------------------------------------------------------------------------------
def _hook(hs, name, cplx):
    return getattr(hs._lib.lib(), name + ("_z" if cplx else "_d"))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _inner(hs, P, Y, conj):
    cplx = np.iscomplexobj(P)
    n, k = P.shape
    m = Y.shape[1]
    P, Y = np.asfortranarray(P), np.asfortranarray(Y)
    T = np.full((k, m), np.nan, dtype=P.dtype, order="F")
    hs._lib.check(_hook(hs, "hsk_mod_inner", cplx)(n, k, m, _vp(P), n, _vp(Y), n, int(conj), _vp(T), k))
    return T


def _apply(hs, Y, Z, T, conj):
    cplx = np.iscomplexobj(Y)
    n, m = Y.shape
    k = Z.shape[1]
    Y, Z, T = np.array(Y, order="F"), np.asfortranarray(Z), np.asfortranarray(T)
    hs._lib.check(_hook(hs, "hsk_mod_apply", cplx)(n, k, m, _vp(Y), n, _vp(Z), n, _vp(T), k, int(conj)))
    return Y


KN, KK, KM = (1, 63, 810, 13824), (1, 5, 16, 17, 64, 130, 256), (1, 15, 17, 33, 64)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n", KN)
def test_inner_and_apply_are_exact_on_integer_data(hs, n, cplx):
    P0, Y0 = _ints((n, max(KK)), cplx, 1), _ints((n, max(KM)), cplx, 2)  # asymmetric: a transposed tile would show
    T0 = _ints((max(KK), max(KM)), cplx, 3)
    for k in KK:
        for m in KM:
            P, Y, T = P0[:, :k], Y0[:, :m], T0[:k, :m]
            for conj in (False, True):
                assert np.array_equal(_inner(hs, P, Y, conj), (P.T if conj else P.conj().T) @ Y), (n, k, m, conj, "inner")
                assert np.array_equal(_apply(hs, Y, P, T, conj), Y - (P.conj() if conj else P) @ T), (n, k, m, conj, "apply")


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_inner_on_random_data_has_the_bits_of_the_mirror(hs, cplx):
    n = 2 * MM.SLAB + 37  # three slabs, the last partial and no multiple of the step
    P, Y = _rand(n, 3, cplx, 11), _rand(n, 2, cplx, 12)
    for conj in ((False, True) if cplx else (False,)):
        T = _inner(hs, P, Y, conj)
        R = MM.inner(P, Y, conj)
        print(f"cplx={cplx} conj={conj}: max |T - mirror| = {np.abs(T - R).max():.2e}, vs numpy {np.abs(T - (P.T if conj else P.conj().T) @ Y).max():.2e}")
        assert np.array_equal(T, R)
    # the same columns inside a wider block, at other positions: the same bits
    Pw, Yw = _rand(n, 20, cplx, 13), _rand(n, 35, cplx, 14)
    Pw[:, 17], Yw[:, 33] = P[:, 1], Y[:, 0]
    assert _inner(hs, Pw, Yw, False)[17, 33] == _inner(hs, P, Y, False)[1, 0]


def test_gather(hs):
    for cplx in (False, True):
        Y = _rand(810, 33, cplx, 4)
        J = np.random.default_rng(5).permutation(810)[:40].astype(np.int64)
        T = np.zeros((40, 33), dtype=Y.dtype, order="F")
        Yf = np.asfortranarray(Y)
        hs._lib.check(_hook(hs, "hsk_mod_gather", cplx)(810, 40, 33, _vp(Yf), 810, J.ctypes.data_as(hs._lib.p_i64), _vp(T), 40))
        assert np.array_equal(T, Y[J])


def _cap(hs, Cm, T, op):
    cplx = np.iscomplexobj(Cm)
    k, m = T.shape
    Cm, T = np.asfortranarray(Cm), np.array(T, order="F")
    st = _hook(hs, "hsk_mod_cap", cplx)(k, m, _vp(Cm), k, op, _vp(T), k)
    return st, T


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("k", [1, 2, 17, 64, 256])
def test_cap_lu_and_solve(hs, k, cplx):
    rng = np.random.default_rng(k)
    Cm = _rand(k, k, cplx, k)
    Cm[np.arange(k), np.arange(k)] = 0.0
    Cm = Cm / max(np.abs(Cm).sum(axis=0).max(), 1.0) * 0.5 + np.eye(k)  # off-diagonal column sums <= 0.5: cond_1 <= 1.5 / 0.5
    cond = float(abs(np.linalg.cond(Cm, 1)))
    assert cond <= 10.0
    T = _rand(k, 19, cplx, k + 1)
    lu = sla.lu_factor(Cm)
    for op in (0, 1, 2):
        st, X = _cap(hs, Cm, T, op)
        assert st == 0
        e = relerr(X, sla.lu_solve(lu, T, trans=op))
        print(f"k={k} cplx={cplx} op={op}: {e:.2e} (cond_1 = {cond:.2f})")
        assert e <= 1e-12 * cond
    if k >= 2:
        # rows must be exchanged: the rows cyclically shifted and a zero leading entry
        Cs = np.roll(Cm, 1, axis=0)
        Cs[0, 0] = 0.0
        conds = float(abs(np.linalg.cond(Cs, 1)))
        lus = sla.lu_factor(Cs)
        for op in (0, 1, 2):
            st, X = _cap(hs, Cs, T, op)
            e = relerr(X, sla.lu_solve(lus, T, trans=op))
            print(f"  shifted rows op={op}: {e:.2e} (cond_1 = {conds:.2e})")
            assert st == 0 and e <= 1e-12 * conds
        # exactly singular: a zero column stays exactly zero under the row operations
        Z = np.array(rng.integers(-2, 3, (k, k)), dtype=Cm.dtype)
        Z[:, k // 2] = 0.0
        st, X = _cap(hs, Z, T, 0)
        assert st == hs._lib.HS_ERR_SINGULAR and np.array_equal(X, T)
    else:
        st, X = _cap(hs, np.zeros((1, 1), dtype=Cm.dtype), T, 0)
        assert st == hs._lib.HS_ERR_SINGULAR


# ---- b. dense U, V on exact handles -----------------------------------------------------------------------------------------------------
def _dense_mod(P, lu, k, cplx, seed):
    """U, V (n x k) scaled so that V^H A^-1 U has 2-norm 0.5 (cond_2(C) <= 3), cond_1(C), and Z = A^-1 U, all from SuperLU solves"""
    n = P["A"].shape[0]
    U, V = _rand(n, k, cplx, seed), _rand(n, k, cplx, seed + 1)
    Z = lu.solve(U)
    G = V.conj().T @ Z
    alpha = 0.5 / np.linalg.norm(G, 2)
    return U * alpha, V, float(abs(np.linalg.cond(np.eye(k) + alpha * G, 1))), Z * alpha


def _op_dense(A, U, V, t):
    A1 = A + U @ V.conj().T
    return {"N": A1, "T": A1.T, "H": A1.conj().T}[t]


def _smw_reference(lu, U, V, Z, Y, t, W):
    """op(A1)^-1 B by the Sherman-Morrison-Woodbury identity in NumPy on SuperLU solves: Y = op(A)^-1 B, Z = A^-1 U, W = A^-H V"""
    Cm = np.eye(U.shape[1]) + V.conj().T @ Z
    if t == "N":
        return Y - Z @ np.linalg.solve(Cm, V.conj().T @ Y)
    if t == "H":
        return Y - W @ np.linalg.solve(Cm.conj().T, U.conj().T @ Y)
    return Y - W.conj() @ np.linalg.solve(Cm.T, U.T @ Y)


def _residual(A, U, V, X, B, t):
    """worst column of ||B - op(A1) X|| / ||B||, matrix-free"""
    if t == "N":
        R = B - A @ X - U @ (V.conj().T @ X)
    elif t == "T":
        R = B - A.T @ X - V.conj() @ (U.T @ X)
    else:
        R = B - A.conj().T @ X - V @ (U.conj().T @ X)
    return max(np.linalg.norm(R[:, j]) / np.linalg.norm(B[:, j]) for j in range(B.shape[1]))


@pytest.mark.parametrize("k", [1, 5, 17, 64])
@pytest.mark.parametrize("kind,shape,nmax", USED, ids=IDS)
def test_dense_modification(hs, kind, shape, nmax, k):
    P, F, lu = _problem(hs, kind, shape, nmax)
    A = P["A"]
    n = A.shape[0]
    cplx = F.dtype.kind == "c"
    U, V, condC, Z = _dense_mod(P, lu, k, cplx, 100 + k)
    assert condC <= 100.0, condC
    M = hs.modify(F, U=U, V=V)
    info = M.info()
    assert M.k == k and M.n == n and M.dtype == F.dtype and info["k"] == k and not info["has_w"]
    assert 0.5 / condC <= M.rcond <= 2.0 / condC, (M.rcond, condC)
    small = n <= 1000
    if small:
        Ad = A.toarray()
        lus = {t: sla.lu_factor(_op_dense(Ad, U, V, t)) for t in TRANS}
    else:  # a dense A1 is out of reach: the identity itself in NumPy on SuperLU solves, independent of the device
        W = lu.solve(V, trans="H")
    B70 = _rand(n, 70, cplx, 200)
    R0 = {t: _lu_trans(lu, B70, t) for t in TRANS}  # the unmodified system by SuperLU, once for all widths
    for nrhs in (1, 17, 33, 70):
        B = B70[:, 70 - nrhs :]
        for t in TRANS:
            X = hs.ldiv_mod(M, B, trans=t)
            e0 = _worst_col(hs.ldiv_block_t(_op(F, hs, t), B), R0[t][:, 70 - nrhs :])
            err = _worst_col(X, sla.lu_solve(lus[t], B) if small else _smw_reference(lu, U, V, Z, R0[t][:, 70 - nrhs :], t, W))
            res = _residual(A, U, V, X, B, t)
            print(f"{kind} {shape} k={k} nrhs={nrhs} trans={t}: err {err:.2e}  e0 {e0:.2e}  cond_1(C) {condC:.2f}  bound {_bound(condC, e0):.2e}  ||B - op(A1) X|| / ||B|| {res:.2e}")
            assert X.shape == B.shape and err <= _bound(condC, e0)
    assert M.info()["has_w"]
    b = _rand(n, 1, cplx, 9)[:, 0]
    x = hs.ldiv_mod(M, b)
    assert x.shape == (n,) and np.array_equal(x, hs.ldiv_mod(M, b.reshape(-1, 1))[:, 0])
    M.free()


# ---- c. entry modifications ---------------------------------------------------------------------------------------------------------------
def _leaf_columns(nd, ncols):
    """`ncols` neighbouring columns (0-based) out of the interior of the largest leaf of the elimination tree, and whether they all lie in
    that leaf; a leaf smaller than `ncols` is continued over the consecutive columns that follow it (its neighbours in the postorder)"""
    leaves = []

    def walk(x):
        if x.left is None and x.right is None:
            leaves.append(x)
        for c in (x.left, x.right):
            if c is not None:
                walk(c)

    walk(nd)
    ints = np.sort(np.asarray(max(leaves, key=lambda x: len(x.int)).int)) - 1
    if len(ints) >= ncols:
        return ints[:ncols], True
    return np.arange(ints[0], ints[0] + ncols), False


def _entry_mod(P, ncols, spread, lu):
    """dA on `ncols` columns, neighbours in one leaf or spread over the tree: the diagonal entry and the first stored off-diagonal entry of
    the column change by 3 : 2 parts of a_jj, the whole scaled so that (A^-1 dA[:, J])[J, :] has 2-norm 0.5 (SuperLU solves): cond_2(C) <= 3.
    Returns dA, J and whether J lies in one leaf."""
    A = sp.csc_matrix(P["A"])
    n = A.shape[0]
    J, one_leaf = (np.unique(np.linspace(0, n - 1, ncols).astype(int)), False) if spread else _leaf_columns(P["nd"], ncols)
    rows, cols, vals = [], [], []
    for j in J:
        col = A.indices[A.indptr[j] : A.indptr[j + 1]]
        d = A[j, j]
        i = int(col[col != j][0])
        rows += [j, i]
        cols += [j, j]
        vals += [0.3 * d, 0.2 * d]
    dA = sp.csc_matrix((np.array(vals, dtype=A.dtype), (rows, cols)), shape=(n, n))
    return dA * (0.5 / np.linalg.norm(lu.solve(dA[:, J].toarray())[J], 2)), J, one_leaf


# (problem, columns, spread).  The leaves of the 2-D problems hold at most 18 interior columns, so their 40 neighbouring columns run over
# consecutive leaves; the 40 columns inside ONE leaf are those of the 24^3 problem (leaves of 64 to 150 columns)
ENTRY = [(0, 1, False), (0, 5, False), (0, 40, False), (0, 5, True), (0, 40, True), (1, 1, True), (1, 5, False), (1, 40, False), (1, 40, True), (2, 40, False), (2, 40, True)]


@pytest.mark.parametrize("which,ncols,spread", ENTRY, ids=[f"{IDS[w]}-{c}-{'spread' if s else 'neighbours'}" for w, c, s in ENTRY])
def test_entry_modification(hs, which, ncols, spread):
    kind, shape, nmax = USED[which]
    P, F, lu = _problem(hs, kind, shape, nmax)
    A = P["A"]
    n = A.shape[0]
    cplx = F.dtype.kind == "c"
    dA, J, one_leaf = _entry_mod(P, ncols, spread, lu)
    k = len(J)
    assert k == ncols and (spread or one_leaf or (which < 2 and ncols == 40))
    Ud = dA[:, J].toarray()
    Vd = np.zeros((n, k))
    Vd[J, np.arange(k)] = 1.0
    condC = float(abs(np.linalg.cond(np.eye(k) + lu.solve(Ud)[J], 1)))
    assert condC <= 100.0, condC
    M = hs.modify(F, dA=dA)
    Md = hs.modify(F, U=Ud, V=Vd)
    assert M.k == k and 0.5 / condC <= M.rcond <= 2.0 / condC
    lu1 = spla.splu(sp.csc_matrix(A + dA))
    B = _rand(n, 33, cplx, 300 + ncols)
    for t in TRANS:
        R = _lu_trans(lu1, B, t)
        X, Xd = hs.ldiv_mod(M, B, trans=t), hs.ldiv_mod(Md, B, trans=t)
        e0 = _e0(hs, F, lu, B, t)
        err, errd, diff = _worst_col(X, R), _worst_col(Xd, R), _worst_col(X, Xd)
        print(f"{IDS[which]} {ncols} cols spread={spread} one_leaf={one_leaf} trans={t}: sparse {err:.2e} dense {errd:.2e} apart {diff:.2e}  e0 {e0:.2e} cond_1(C) {condC:.2f} bound {_bound(condC, e0):.2e}")
        assert err <= _bound(condC, e0) and errd <= _bound(condC, e0) and diff <= _bound(condC, e0)
    M.free()
    Md.free()


# ---- d. bits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax", USED, ids=IDS)
def test_bits(hs, kind, shape, nmax):
    P, F, lu = _problem(hs, kind, shape, nmax)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    B = _rand(n, 70, cplx, 7)
    M0 = hs.modify(F)
    assert M0.k == 0 and M0.rcond == 1.0
    U, V, _, _ = _dense_mod(P, lu, 5, cplx, 31)
    M = hs.modify(F, U=U, V=V)
    dA, J, _ = _entry_mod(P, 5, True, lu)
    Ms = hs.modify(F, dA=dA)
    for t in TRANS:
        assert np.array_equal(hs.ldiv_mod(M0, B, trans=t), hs.ldiv_block_t(_op(F, hs, t), B))
        for Mx in (M, Ms):
            X = hs.ldiv_mod(Mx, B, trans=t)
            assert np.array_equal(X, hs.ldiv_mod(Mx, B, trans=t))
            for j in (0, 31, 32, 69):
                assert np.array_equal(hs.ldiv_mod(Mx, B[:, j], trans=t), X[:, j])
            perm = np.random.default_rng(3).permutation(70)
            assert np.array_equal(hs.ldiv_mod(Mx, B[:, perm], trans=t), X[:, perm])
            assert np.array_equal(hs.ldiv_mod(Mx, B[:, 5:38], trans=t), X[:, 5:38])
            Br = B.astype(F.dtype).copy(order="F")
            assert hs.ldiv_mod(Br, Mx, Br, trans=t) is Br and np.array_equal(Br, X)
    # C aliasing B in the C ABI, ld > n, the padding rows untouched, nrhs = 0 touching nothing
    L = hs._lib.lib()
    fn = L.hs_mod_ldiv_z if cplx else L.hs_mod_ldiv_d
    pf = hs._lib.p_f64
    ld = n + 5
    Bp = np.zeros((ld, 70), dtype=F.dtype, order="F")
    Bp[:n] = B
    hs._lib.check(fn(M._h, 0, Bp.ctypes.data_as(pf), ld, Bp.ctypes.data_as(pf), ld, n, 70))
    assert np.array_equal(Bp[:n], hs.ldiv_mod(M, B)) and np.all(Bp[n:] == 0)
    Cq = np.full((n, 2), 7.0, dtype=F.dtype, order="F")
    hs._lib.check(fn(M._h, 0, Cq.ctypes.data_as(pf), n, Bp.ctypes.data_as(pf), ld, n, 0))
    assert np.all(Cq == 7.0)
    for Mx in (M0, M, Ms):
        Mx.free()


def test_other_chunk_widths_agree(hs, tmp_path):
    """HS_LDIV_BLOCK_COLS is read once per process: 16 and 64 in child processes.  The block solve's own tests do not require its bits to
    be those of another chunk width, so neither does this one: the columns agree to the bound of the modified solves."""
    kind, shape, nmax = USED[0]
    P, F, lu = _problem(hs, kind, shape, nmax)
    n = P["A"].shape[0]
    B = _rand(n, 70, False, 7)
    U, V, condC, _ = _dense_mod(P, lu, 5, False, 31)
    M = hs.modify(F, U=U, V=V)
    np.savez(tmp_path / "in.npz", B=B, U=U, V=V)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"""
import sys, os, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, "tests")!r})
import hsamd
from helpers import prepare
hs = hsamd.load()
P = prepare(hs, {shape!r}, kind={kind!r}, nmax={nmax}, rhs="randn")
F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
d = np.load({str(tmp_path / "in.npz")!r})
M = hs.modify(F, U=d["U"], V=d["V"])
np.savez({str(tmp_path)!r} + "/out" + os.environ["HS_LDIV_BLOCK_COLS"] + ".npz", N=hs.ldiv_mod(M, d["B"]), T=hs.ldiv_mod(M, d["B"], trans="T"))
"""
    for w in ("16", "64"):
        subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, HS_LDIV_BLOCK_COLS=w), timeout=300)
    for t in ("N", "T"):
        X = hs.ldiv_mod(M, B, trans=t)
        e0 = _e0(hs, F, lu, B, t)
        for w in ("16", "64"):
            Xw = np.load(tmp_path / f"out{w}.npz")[t]
            d = _worst_col(Xw, X)
            print(f"HS_LDIV_BLOCK_COLS={w} trans={t}: apart {d:.2e}  bound {_bound(condC, e0):.2e}")
            assert d <= _bound(condC, e0)
    M.free()


# ---- e. a compressed handle: GMRES preconditioned by the modified factorization ----------------------------------------------------------
def test_gmres_on_a_compressed_handle(hs):
    label, kind, shape, nmax, kw = COMPRESSED[0]
    P, F, _ = _problem(hs, kind, shape, nmax, want_lu=False, **kw)
    A = P["A"]
    n = A.shape[0]
    B = _rand(n, 9, True, 41)
    dA, J, _ = _entry_mod(P, 5, True, _problem(hs, *USED[2])[2])  # the same matrix, factored exactly: its SuperLU factors scale dA
    A1 = sp.csc_matrix(A + dA)
    M = hs.modify(F, dA=dA)
    X0, ch0 = hs.gmres_block(A, B, Pr=F, reltol=1e-8, restart=30, maxiter=60, log=True)
    X1, ch1 = hs.gmres_block(A1, B, Pr=M, reltol=1e-8, restart=30, maxiter=60, log=True)
    X2, ch2 = hs.gmres_block(A1, B, Pr=F, reltol=1e-8, restart=30, maxiter=60, log=True)
    it0, it1, it2 = (max(c["iters"] for c in ch) for ch in (ch0, ch1, ch2))
    res = max(np.linalg.norm(B[:, j] - A1 @ X1[:, j]) / np.linalg.norm(B[:, j]) for j in range(B.shape[1]))
    print(f"{label}: iterations unmodified {it0}, modified with Pr=M {it1}, modified with the old Pr=F {it2}; worst ||b - A1 x|| / ||b|| = {res:.2e}  rcond(C) = {M.rcond:.2e}")
    assert all(c["isconverged"] for c in ch0) and all(c["isconverged"] for c in ch1)
    assert it1 <= it0 + 2
    assert res <= 1e-8
    for t in ("T", "C"):
        Xt, cht = hs.gmres_block(A1, B[:, :3], Pr=M, trans=t, reltol=1e-8, restart=30, maxiter=60, log=True)
        At = A1.T if t == "T" else A1.conj().T
        rt = max(np.linalg.norm(B[:, j] - At @ Xt[:, j]) / np.linalg.norm(B[:, j]) for j in range(3))
        print(f"  trans={t}: iterations {max(c['iters'] for c in cht)}, residual {rt:.2e}")
        assert all(c["isconverged"] for c in cht) and rt <= 1e-8
    M.free()


# ---- f. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(hs):
    P, F, lu = _problem(hs, *USED[0])
    n = P["A"].shape[0]
    E = hs._lib
    U = _rand(n, 3, False, 1)
    with pytest.raises(hs.UnsupportedError, match="refactor"):
        hs.modify(F, U=np.zeros((n, 257)), V=np.zeros((n, 257)))
    with pytest.raises(hs.UnsupportedError, match="refactor"):
        hs.modify(F, dA=sp.eye(n, format="csc"))  # 810 modified columns
    with pytest.raises(hs.DimensionMismatch):
        hs.modify(F, U=U[:-1], V=U[:-1])
    with pytest.raises(TypeError):
        hs.modify(F, U=U.astype(complex), V=U)
    M = hs.modify(F, U=U * 1e-3, V=U)
    B = _rand(n, 4, False, 2)
    with pytest.raises(ValueError, match="trans"):
        hs.ldiv_mod(M, B, trans="X")
    with pytest.raises(hs.DimensionMismatch):
        hs.ldiv_mod(M, B[:-1])
    with pytest.raises(TypeError):
        hs.ldiv_mod(M, B.astype(complex))
    with pytest.raises(ValueError):
        hs.gmres_block(None, B, Pr=M)
    L = E.lib()
    pf = E.p_f64
    Bf = np.asfortranarray(B)
    Cf = np.full_like(Bf, 7.0)
    assert L.hs_mod_ldiv_d(M._h, 3, Cf.ctypes.data_as(pf), n, Bf.ctypes.data_as(pf), n, n, 4) == E.HS_ERR_ARGUMENT
    assert L.hs_mod_ldiv_z(M._h, 0, Cf.ctypes.data_as(pf), n, Bf.ctypes.data_as(pf), n, n, 4) == E.HS_ERR_ARGUMENT
    assert L.hs_mod_ldiv_d(M._h, 0, Cf.ctypes.data_as(pf), n - 1, Bf.ctypes.data_as(pf), n, n, 4) == E.HS_ERR_DIMENSION
    assert L.hs_mod_ldiv_d(M._h, 0, Cf.ctypes.data_as(pf), n, Bf.ctypes.data_as(pf), n, n, -1) == E.HS_ERR_DIMENSION
    assert L.hs_mod_ldiv_d(M._h, 0, None, n, Bf.ctypes.data_as(pf), n, n, 4) == E.HS_ERR_ARGUMENT
    one = np.ones(3, dtype=np.int64).ctypes.data_as(E.p_i64)
    assert L.hs_gmres_block_mod_d(M._h, 0, n, None, None, None, _vp(Bf), n, _vp(Cf), n, 4, 0, 0, -1.0, 0.0, -1, 5, None, one, None, None) == E.HS_ERR_ARGUMENT
    h = C.c_void_p()
    Uf = np.asfortranarray(U)
    assert L.hs_mod_create_z(F._h, n, 3, _vp(Uf), n, _vp(Uf), n, C.byref(h)) == E.HS_ERR_ARGUMENT and not h
    assert L.hs_mod_create_d(F._h, n, 3, _vp(Uf), n - 1, _vp(Uf), n, C.byref(h)) == E.HS_ERR_DIMENSION and not h
    assert L.hs_mod_create_d(F._h, n, 3, None, n, _vp(Uf), n, C.byref(h)) == E.HS_ERR_ARGUMENT and not h
    bad = np.array([1, 3, 2] + [2] * (n - 2), dtype=np.int64)  # decreasing column pointers
    assert L.hs_mod_create_sparse_d(F._h, n, bad.ctypes.data_as(E.p_i64), one, _vp(Uf), C.byref(h)) == E.HS_ERR_ARGUMENT and not h
    assert np.all(Cf == 7.0)
    M.free()
    # a handle the block solve does not serve: an HSS interior block (mf = 2)
    P2 = prepare(hs, (24, 24, 24), kind="convdiff", nmax=300, rhs="randn")
    F2 = hs.factor(P2["A"], P2["nd"], P2["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    n2 = P2["A"].shape[0]
    with pytest.raises(hs.UnsupportedError):
        hs.modify(F2, U=np.ones((n2, 1)), V=np.ones((n2, 1)))
    with pytest.raises(hs.UnsupportedError):
        hs.modify(F2, dA=sp.csc_matrix(([1.0], ([0], [0])), shape=(n2, n2)))
    F2.free()


# ---- g. timing guard --------------------------------------------------------------------------------------------------------------------
def test_the_correction_costs_less_than_a_block_solve(hs):
    """Poisson 40^3 exact, k = 32, 32 columns: the correction moves n (k + 2 m) values, a few percent of the factor bytes a block solve reads;
    the factor 2 is for launch overhead at this size."""
    P, F, _ = _problem(hs, "poisson", (40, 40, 40), 300, want_lu=False)
    n = P["A"].shape[0]
    U, V = _rand(n, 32, False, 1), _rand(n, 32, False, 2)
    U *= 0.5 / np.linalg.norm(V.T @ hs.ldiv_block(F, U), 2)
    M = hs.modify(F, U=U, V=V)
    B = _rand(n, 32, False, 3)
    hs.ldiv_mod(M, B)
    hs.ldiv_block(F, B)

    def med(f):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[1]

    tb = med(lambda: hs.ldiv_block(F, B))
    tm = med(lambda: hs.ldiv_mod(M, B))
    print(f"Poisson 40^3 k=32 nrhs=32: ldiv_block {tb * 1e3:.2f} ms, ldiv_mod {tm * 1e3:.2f} ms (device {M.info()['solve_seconds'] * 1e3:.2f} ms), build {M.info()['build_seconds'] * 1e3:.1f} ms")
    assert tm <= 2.0 * tb
    M.free()
