"""hs_ulv_mode on the MI355X: with the switch on, the lockstep drivers (GMRES, refined solves, the 1-norm estimator, sensitivities) and
hs_logabsdet serve handles whose fronts keep their interior block D as an HSS matrix (mf = 2, 3) through the ULV block solve; with the
switch off they refuse them as before, and a handle without such fronts does not notice the switch.  Handles and bounds come from the
tests of the same drivers on dense-front handles (test_gmres_block_gpu.py, test_refine_block_gpu.py, test_condest_gpu.py,
test_sens_gpu.py, test_ulv_t_gpu.py, test_selinv_gpu.py); one factorization per handle is shared by the tests of this file."""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sens_mirror as SM
from helpers import prepare, relerr
from test_ulv_t_gpu import ADJOINT_BOUND

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
NCOL = 35  # one full chunk of 32 columns and a ragged one
GM = dict(reltol=1e-9, restart=30, maxiter=30)
COMMON = dict(swsize=8, atol=1e-6, rtol=1e-6, leafsize=128)
HANDLES = {
    "mf2": ("convdiff", (20, 20, 20), 200, dict(swlevel=2, mf=2, **COMMON)),
    "mf3": ("convdiff", (24, 24, 24), 300, dict(swlevel=3, mf=3, **COMMON)),
    "mf2-complex": ("convdiff_helmholtz", (24, 24, 24), 300, dict(swlevel=2, mf=2, **COMMON)),
    # no HSS interior block: the exact handle, and the mf = 1 handles of the two real problems (the yardstick of the determinant test)
    "exact": ("poisson", (15, 15), 20, dict(swlevel=0)),
    "mf2-as-mf1": ("convdiff", (20, 20, 20), 200, dict(swlevel=2, mf=1, **COMMON)),
    "mf3-as-mf1": ("convdiff", (24, 24, 24), 300, dict(swlevel=3, mf=1, **COMMON)),
}
HSS = ["mf2", "mf3", "mf2-complex"]
_H = {}
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _free_handles():
    yield
    for P, F, x0 in _H.values():
        F.free()
    _H.clear()
    _REF.clear()


def handle(hs, label):
    """(problem, factorization, hs.ldiv(F, b) taken before anything else ran on the handle)"""
    if label not in _H:
        kind, shape, nmax, kw = HANDLES[label]
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        F = hs.factor(P["A"], P["nd"], P["nd_loc"], **kw)
        flow = (C.c_int64 * 8)()
        hs._lib.check(hs._lib.lib().hs_flow_info(F._h, flow))
        if label in HSS:
            assert flow[0] in (2, 3) and flow[1] > 0, list(flow)  # matrix-free fronts whose D is an HSS matrix / the 2 x 2 block form
        assert hs.ulv_mode(F) is False  # the default
        _H[label] = (P, F, hs.ldiv(F, P["b"].astype(F.dtype)))
    return _H[label]


@contextlib.contextmanager
def ulv(hs, F):
    assert hs.ulv_mode(F, True) is False
    try:
        yield F
    finally:
        assert hs.ulv_mode(F, False) is True


def _block(n, k, cplx, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    return B + 1j * rng.standard_normal((n, k)) if cplx else B


def _op(hs, F, trans):
    return (F, hs.transpose(F), hs.adjoint(F))[trans]


def _opA(A, trans):
    return (A, A.T, A.conj().T)[trans].tocsc()


def _res(A, X, B):
    R = B - A @ X
    return np.linalg.norm(R, axis=0) / np.linalg.norm(B, axis=0)


# ---- the switch ---------------------------------------------------------------------------------------------------------------------------

def test_mode_0_still_refuses(hs):
    P, F, x0 = handle(hs, "mf2")
    A, n = P["A"], P["A"].shape[0]
    B = _block(n, 3, False, 1)
    assert hs.ulv_mode(F) is False and hs.ulv_mode(hs.transpose(F)) is False
    for call in (lambda: hs.gmres_block(A, B, Pr=F, **GM), lambda: hs.ldiv_refine_block(F, B), lambda: hs.condest(F, 1),
                 lambda: hs.sensitivity(F, B, B), lambda: hs.logabsdet(F)):
        with pytest.raises(hs.UnsupportedError):
            call()
    # the three views share one setting
    assert hs.ulv_mode(hs.adjoint(F), True) is False and hs.ulv_mode(F) is True and hs.ulv_mode(hs.transpose(F), False) is True
    assert hs.ulv_mode(F) is False
    with pytest.raises(hs.UnsupportedError):
        hs.logabsdet(F)


def test_the_switch_does_not_change_a_handle_without_hss_fronts(hs):
    P, F, x0 = handle(hs, "exact")
    A, n = P["A"], P["A"].shape[0]
    B = _block(n, NCOL, False, 2)
    calls = dict(gmres_block=lambda: hs.gmres_block(A, B, Pr=F, log=True, **GM), gmres=lambda: hs.gmres(A, B[:, 0], Pr=F, log=True, **GM),
                 refine_block=lambda: hs.ldiv_refine_block(hs.transpose(F), B), refine=lambda: hs.ldiv_refine(hs.transpose(F), B[:, :3]),
                 condest=lambda: (hs.condest(F, 1), hs.condest(F, np.inf), hs.opnormestinv(hs.adjoint(F), nsolves=True)),
                 sensitivity=lambda: hs.sensitivity(F, B[:, :8], B[:, 8:16], want=("X", "Lam")), logabsdet=lambda: hs.logabsdet(F))
    off = {k: f() for k, f in calls.items()}
    with ulv(hs, F):
        on = {k: f() for k, f in calls.items()}
    for k in calls:
        assert _same_bits(off[k], on[k]), k


def _same_bits(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_bits(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a), np.asarray(b))


# ---- GMRES ----------------------------------------------------------------------------------------------------------------------------------

def _looped_reference(hs, label):
    """hs.gmres column by column in mode 0 (trans = N, the only direction that path serves on these handles); once per handle."""
    if label not in _REF:
        P, F, x0 = handle(hs, label)
        A, n = P["A"], P["A"].shape[0]
        B = _block(n, NCOL, F.dtype.kind == "c", 3)
        assert hs.ulv_mode(F) is False
        X, its = np.empty_like(B), []
        for c in range(NCOL):
            X[:, c], ch = hs.gmres(A, B[:, c], Pr=F, log=True, **GM)
            assert ch["isconverged"]
            its.append(ch["iters"])
        _REF[label] = (B, X, np.array(its), _res(A, X, B))
    return _REF[label]


@pytest.mark.parametrize("trans", [0, 1, 2])
@pytest.mark.parametrize("label", HSS)
def test_gmres_block(hs, label, trans):
    P, F, x0 = handle(hs, label)
    A = P["A"]
    B, Xl, itl, resl = _looped_reference(hs, label)
    Aop = _opA(A, trans)
    with ulv(hs, F):
        X, chs = hs.gmres_block(A, B, Pr=F, trans="NTC"[trans], log=True, **GM)
        X2, chs2 = hs.gmres_block(A, B, Pr=F, trans="NTC"[trans], log=True, **GM)
        Xo, cho = hs.gmres_block(None, B, Pr=_op(hs, F, trans), log=True, **GM)  # the handle's own A
        x1, c1 = hs.gmres(A, B[:, 0], Pr=F, trans="NTC"[trans], log=True, **GM)  # one column: the same block solve on one column
    its = np.array([c["iters"] for c in chs])
    res = _res(Aop, X, B)
    print(f"{label} trans={trans}: iterations {its.min()}..{its.max()} (looped, N: {itl.min()}..{itl.max()}), worst residual {res.max():.2e} (looped, N: {resl.max():.2e})")
    assert all(c["isconverged"] for c in chs) and all(c["isconverged"] for c in cho) and c1["isconverged"]
    if trans == 0:
        assert np.all(np.abs(its - itl) <= 1), (its, itl)
        assert np.all(res <= 2 * np.maximum(GM["reltol"], resl)), (res, resl)
    else:
        assert np.all(res <= 2 * GM["reltol"]), res
    assert np.all(_res(Aop, Xo, B) <= 2 * GM["reltol"]) and _res(Aop, x1[:, None], B[:, :1])[0] <= 2 * GM["reltol"]
    assert abs(c1["iters"] - its[0]) <= 1
    # two calls: equal bits
    assert np.array_equal(X, X2) and [c["resnorm"] for c in chs] == [c["resnorm"] for c in chs2]


@pytest.mark.parametrize("trans", [1, 2])
def test_gmres_adjoint_identity(hs, trans):
    """<y, A x> = <A^H y, x> (transpose: without the conjugate) with x and y the GMRES solutions of A x = b and op(A) y = w, as a defect
    relative to |W|_F |X|_F like test_handle_adjoint_identity.  The solutions are exact only to the tolerance GMRES was asked for, so the
    bound is that test's rounding level plus what the tolerance alone admits, fixed before any run: every converged column has
    |b - A x| <= 2 reltol |b| (the residual bound asserted in test_gmres_block), hence |Y^op B - W^op X| = |Y^op (B - A X) - (W - op(A) Y)^op X|
    <= 2 reltol (|Y| |B| + |W| |X|).  No measured residual enters: a solve in the wrong direction (the defect is then of order 1) or a
    column that stopped early fails it."""
    P, F, x0 = handle(hs, "mf2-complex")
    A, n = P["A"], P["A"].shape[0]
    B, W = _block(n, 8, True, 11), _block(n, 8, True, 12)
    with ulv(hs, F):
        X = hs.gmres_block(A, B, Pr=F, **GM)
        Y = hs.gmres_block(A, W, Pr=_op(hs, F, trans), **GM)
    t = (lambda M: M.conj().T) if trans == 2 else (lambda M: M.T)
    nrm = np.linalg.norm
    d = nrm(t(Y) @ B - t(W) @ X) / (nrm(W) * nrm(X))
    bound = ADJOINT_BOUND + 2 * GM["reltol"] * (nrm(Y) * nrm(B) / (nrm(W) * nrm(X)) + 1.0)
    wrong = nrm(t(Y) @ B - t(W) @ X.conj()) / (nrm(W) * nrm(X))  # the identity with the wrong operator on one side: what the bound must exclude
    print(f"mf2-complex trans={trans}: defect of the adjoint identity {d:.2e} (bound {bound:.2e}; with conj(X) in place of X: {wrong:.2e})")
    assert d <= bound
    assert wrong > 1e3 * bound


def test_refusals_leave_the_outputs_untouched(hs):
    """Refusals that concern the switch, through the C ABI with every output pre-filled: the mode-0 refusal of hs_gmres_block_* on an
    HSS-interior handle (what the switch turns into service), and the refusal mode 1 adds, a sparse B of hs_sens_*."""
    from hierarchicalsolvers_jl_amd.gmres import _csc_fields
    from hierarchicalsolvers_jl_amd.solver import _sens_block

    P, F, x0 = handle(hs, "mf2")
    A, n = P["A"], P["A"].shape[0]
    L, E = hs._lib.lib(), hs._lib
    colptr, rowval, nz = _csc_fields(A, np.float64)
    B = np.asfortranarray(_block(n, 3, False, 5))
    X = np.full((n, 3), 42.0, order="F")
    iters, conv = np.full(3, 7, dtype=np.int64), np.full(3, 7, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pi = E.p_i64
    gm = lambda: L.hs_gmres_block_d(F._h, n, colptr.ctypes.data_as(pi), rowval.ctypes.data_as(pi), vp(nz), vp(B), n, vp(X), n, 3, 0, 0, 1e-9, 0.0, 30, 30, None,  # noqa: E731
                                    iters.ctypes.data_as(pi), conv.ctypes.data_as(C.POINTER(C.c_int)), None)
    assert gm() == E.HS_ERR_UNSUPPORTED and b"hs_gmres_*" in L.hs_last_error()
    assert np.all(X == 42.0) and np.all(iters == 7) and np.all(conv == 7)
    with ulv(hs, F):
        assert gm() == 0 and np.all(conv == 1) and not np.any(X == 42.0)  # the same call, served
        argB, k, keepB = _sens_block("B", sp.csc_matrix(B), n, F.dtype)
        argW, _, keepW = _sens_block("W", B, n, F.dtype, k)
        G = np.full(A.nnz, 42.0)
        Xs, Lam = np.full((n, 3), 42.0, order="F"), np.full((n, 3), 42.0, order="F")
        rc = L.hs_sens_d(F._h, 0, n, k, C.byref(argB), C.byref(argW), 0, 0, G.ctypes.data, Xs.ctypes.data, n, Lam.ctypes.data, n)
        assert rc == E.HS_ERR_UNSUPPORTED and b"sparse" in L.hs_last_error()
        assert np.all(G == 42.0) and np.all(Xs == 42.0) and np.all(Lam == 42.0)
        del keepB, keepW


def test_the_mode_survives_a_refactorization(hs):
    """hs_numeric_begin .. hs_numeric_end on a handle whose switch is on: the mode is still 1 afterwards and still in effect --
    hs_logabsdet, which refuses this handle in mode 0, answers for the new values.  The second factorization is of 2 A, whose
    log|det| is larger by n log 2; both answers carry the compression error of their factorization (5.7e-7 on this problem against
    SuperLU), which 1e-3 bounds with three orders of magnitude to spare."""
    import torch

    from hierarchicalsolvers_jl_amd import dist as hsdist

    kind, shape, nmax, kw = HANDLES["mf2"]
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    S = hsdist.StagedSolver(P["A"], P["nd"], P["nd_loc"], device="cuda:0", **kw)
    L, E = hs._lib.lib(), hs._lib
    h = S.backend._h
    n = P["A"].shape[0]
    la, sg, las = C.c_double(), (C.c_double * 2)(), []
    assert L.hs_ulv_mode(h, 1) == 0  # set on the analysed handle, before any numeric factorization
    for scale in (1.0, 2.0):
        S.numeric(torch.from_numpy(np.ascontiguousarray(P["A"].data * scale)).to("cuda:0"))
        assert L.hs_ulv_mode(h, -1) == 1
        E.check(L.hs_logabsdet(h, C.byref(la), sg))
        las.append(la.value)
    print(f"mf2 refactored with 2 A: log|det| {las[0]:.9g} -> {las[1]:.9g}, difference - n log 2 = {las[1] - las[0] - n * np.log(2.0):.2e}")
    assert abs(las[1] - las[0] - n * np.log(2.0)) <= 1e-3
    assert L.hs_ulv_mode(h, 0) == 1
    assert L.hs_logabsdet(h, C.byref(la), sg) == E.HS_ERR_UNSUPPORTED


def test_column_independence_of_the_ulv_block_solve(hs):
    """The lockstep drivers are independent of the other columns of a call only as far as hs_ldiv_ulv_dev_* is.  It is: on the three
    handles and in the three directions, columns taken from both chunks of a 35-column call carry the bits of a 3-column call (DESIGN.md
    4d' records the measurement), so the property is asserted here next to "two calls return equal bits"."""
    for label in HSS:
        P, F, x0 = handle(hs, label)
        B = _block(P["A"].shape[0], NCOL, F.dtype.kind == "c", 6)
        sub = [0, 5, 33]
        for trans in (0, 1, 2):
            X = hs.ldiv_ulv(_op(hs, F, trans), B)
            Xs = hs.ldiv_ulv(_op(hs, F, trans), B[:, sub])
            print(f"{label} trans={trans}: columns {sub} of a {NCOL}-column hs.ldiv_ulv call carry the bits of a 3-column call: {np.array_equal(X[:, sub], Xs)}"
                  f" (worst relative difference {max(relerr(X[:, j], Xs[:, i]) for i, j in enumerate(sub)):.1e})")
            assert np.array_equal(X[:, sub], Xs), (label, trans)
            assert np.array_equal(X, hs.ldiv_ulv(_op(hs, F, trans), B))


# ---- refined solves -----------------------------------------------------------------------------------------------------------------------

def test_refine_block_against_looped_refine(hs):
    P, F, x0 = handle(hs, "mf2")
    n = P["A"].shape[0]
    B = _block(n, NCOL, False, 7)
    Xl, berrl, _, stepsl = hs.ldiv_refine(F, B, itmax=5, ferr=False)  # mode 0: the looped path that serves this handle
    with ulv(hs, F):
        X, berr, ferr, steps = hs.ldiv_refine_block(F, B, itmax=5, ferr=False)
        again = hs.ldiv_refine_block(F, B, itmax=5, ferr=False)
    print(f"mf2: berr {berr.max():.2e} after {steps.max()} steps (looped hs.ldiv_refine: {berrl.max():.2e} after {stepsl.max()})")
    assert ferr is None and np.all(berr <= 4 * np.maximum(berrl, EPS)), (berr, berrl)
    assert np.array_equal(X, again[0]) and np.array_equal(berr, again[1]) and np.array_equal(steps, again[3])


@pytest.mark.parametrize("trans", [0, 1, 2])
def test_refine_block_ferr_bounds_the_true_error(hs, trans):
    P, F, x0 = handle(hs, "mf2")
    n = P["A"].shape[0]
    B = _block(n, NCOL, False, 8)
    Xs = spla.splu(_opA(P["A"], trans)).solve(B)
    with ulv(hs, F):
        X, berr, ferr, steps = hs.ldiv_refine_block(_op(hs, F, trans), B, itmax=5, ferr=True)
        x1, b1, f1, s1 = hs.ldiv_refine(_op(hs, F, trans), B[:, 0], itmax=5, ferr=True) if trans == 1 else (None,) * 4
    true = np.abs(X - Xs).max(axis=0) / np.abs(X).max(axis=0)
    print(f"mf2 trans={trans}: ferr {ferr.min():.2e}..{ferr.max():.2e}, true {true.max():.2e}, berr {berr.max():.2e}")
    assert np.all(true <= ferr), (true, ferr)
    if trans == 1:  # the single-vector driver on the same route
        t1 = np.abs(x1 - Xs[:, 0]).max() / np.abs(x1).max()
        assert t1 <= f1 and np.abs(x1 - X[:, 0]).max() / np.abs(X[:, 0]).max() <= f1 + ferr[0]


# ---- estimators ---------------------------------------------------------------------------------------------------------------------------

def test_estimators_against_the_inverse_by_ulv_block_solves(hs):
    P, F, x0 = handle(hs, "mf2")
    A, n = P["A"], P["A"].shape[0]
    colsum = np.zeros(n)  # column sums of |F^-1|: ||F^-1||_1 = their maximum, ||F^-1||_Inf = ||F^-T||_1 from the row sums
    rowsum = np.zeros(n)
    for c0 in range(0, n, 512):
        c1 = min(n, c0 + 512)
        I = np.zeros((n, c1 - c0))
        I[np.arange(c0, c1), np.arange(c1 - c0)] = 1.0
        Z = np.abs(hs.ldiv_ulv(F, I))
        colsum[c0:c1] = Z.sum(axis=0)
        rowsum += Z.sum(axis=1)
    true1, trueinf = colsum.max(), rowsum.max()
    with ulv(hs, F):
        est1, estT = hs.opnormestinv(F), hs.opnormestinv(hs.transpose(F))
        c1_, cinf = hs.condest(F, 1), hs.condest(F, np.inf)
        assert hs.opnormestinv(F) == est1 and hs.condest(F, 1) == c1_
    print(f"mf2: ||F^-1||_1 {true1:.6e} (estimate {est1:.6e}), ||F^-1||_Inf {trueinf:.6e} (estimate {estT:.6e})")
    # the two-sided bounds of tests/test_condest_gpu.py: a lower bound, within the estimator's factor of 3
    for est, true in ((est1, true1), (estT, trueinf), (c1_, true1 * spla.norm(A, 1)), (cinf, trueinf * spla.norm(A, np.inf))):
        assert est <= true * (1 + 1e-10) and est >= true / 3, (est, true)


# ---- sensitivities ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("label", ["mf2", "mf2-complex"])
def test_sensitivity_carries_the_bits_of_the_ulv_solves(hs, label):
    P, F, x0 = handle(hs, label)
    A = SM.canonical(P["A"])
    n, k = A.shape[0], 8
    cplx = F.dtype.kind == "c"
    B, W = _block(n, k, cplx, 13), _block(n, k, cplx, 14)
    with ulv(hs, F):
        G, X, Lam = hs.sensitivity(F, B, W, want=("X", "Lam"))
        G2 = hs.sensitivity(F, B, W)
        for Bs, Ws in ((sp.csc_matrix(B), W), (B, sp.csc_matrix(W))):
            with pytest.raises(hs.UnsupportedError, match="sparse"):
                hs.sensitivity(F, Bs, Ws)
    with pytest.raises(hs.UnsupportedError):  # mode 0: as before
        hs.sensitivity(F, sp.csc_matrix(B), W)
    assert np.array_equal(X, hs.ldiv_ulv(F, B)) and np.array_equal(Lam, hs.ldiv_ulv(hs.adjoint(F), W)) and np.array_equal(G, G2)
    ref, S = SM.reduce(A, Lam, X, 0), SM.bound(A, Lam, X, 0)
    excess = np.abs(G - ref) - 4 * (k + 4) * EPS * S  # the inner-product bound of test_sens_gpu.py
    assert np.all(excess <= 0), float(excess.max())


def test_misfit_and_refined_sensitivity_run_on_the_same_route(hs):
    """hs_misfit_* builds its cotangent on the receiver rows itself; with the switch on it reaches the ULV block solve as a dense block.
    Checked against hs.sensitivity with that cotangent given densely, which the test above ties to the ULV solves."""
    P, F, x0 = handle(hs, "mf2")
    n, k = P["A"].shape[0], 5
    B = _block(n, k, False, 15)
    rows = np.array([3, n // 2, n - 1])
    with ulv(hs, F):
        X = hs.ldiv_ulv(F, B)
        D = X[rows] + 0.5
        out = hs.misfit(F, B, rows, D)
        J, G = out[0], out[1]
        W = np.zeros((n, k))
        W[rows] = X[rows] - D
        Gs = hs.sensitivity(F, B, W)
        Gr, Xr, Lr = hs.sensitivity(F, B, W, itmax=3, want=("X", "Lam"))
    assert np.allclose(np.asarray(J), 0.5 * np.sum(np.abs(W[rows]) ** 2, axis=0), rtol=1e-12)
    assert np.array_equal(np.asarray(G), Gs)
    assert relerr(Xr, spla.splu(P["A"].tocsc()).solve(B)) < 1e-8  # refined to the accuracy of A, not of F


# ---- the determinant --------------------------------------------------------------------------------------------------------------------

def _superlu_slogdet(A):
    lu = spla.splu(A.tocsc())
    d = lu.U.diagonal()

    def parity(p):
        seen, odd = np.zeros(len(p), bool), 0
        for i in range(len(p)):
            j, ln = i, 0
            while not seen[j]:
                seen[j] = True
                j = p[j]
                ln += 1
            odd ^= (ln - 1) & 1 if ln else 0
        return odd

    sign = np.prod(np.sign(d)) * (-1.0) ** (parity(lu.perm_r) ^ parity(lu.perm_c))
    return sign, float(np.sum(np.log(np.abs(d))))


@pytest.mark.parametrize("label", ["mf2", "mf3"])
def test_logabsdet_of_hss_interior_handles(hs, label):
    P, F, x0 = handle(hs, label)
    P1, F1, _ = handle(hs, label + "-as-mf1")  # the same problem and tolerance with dense interior blocks: hs.logabsdet serves it as it is
    sref, lref = _superlu_slogdet(P["A"])
    la1, s1 = hs.logabsdet(F1)
    with ulv(hs, F):
        la, s = hs.logabsdet(F)
        assert hs.logabsdet(F) == (la, s) and hs.logabsdet(hs.transpose(F)) == (la, s)
        assert hs.logdet(F) == la if s > 0 else True
        with np.errstate(over="ignore"):  # exp(log|det|) overflows on these sizes, as Julia's det does
            assert hs.det(F) == s * np.exp(la)
        with pytest.raises(hs.UnsupportedError):
            hs.selinv(F)
    d, d1 = abs(la - lref), abs(la1 - lref)
    print(f"{label}: log|det A| {lref:.12g}; |log|det F| - log|det A||: {d:.3e} with HSS interior blocks, {d1:.3e} on the mf = 1 handle (bound 10 x)")
    assert s == sref and s1 == sref
    assert d <= 10 * d1, (d, d1)


# ---- guard and aftermath ------------------------------------------------------------------------------------------------------------------

def test_guard_one_block_call_is_not_slower_than_the_looped_gmres(hs):
    """32 columns on the mf = 2 handle: one lockstep call through the ULV block solve against the 32 hs.gmres calls it replaces."""
    P, F, x0 = handle(hs, "mf2")
    A = P["A"]
    B = _block(A.shape[0], 32, False, 41)
    hs.gmres(A, B[:, 0], Pr=F, **GM)
    t0 = time.perf_counter()
    for c in range(32):
        hs.gmres(A, B[:, c], Pr=F, **GM)
    t1 = time.perf_counter()
    with ulv(hs, F):
        hs.gmres_block(A, B[:, :2], Pr=F, **GM)
        t2 = time.perf_counter()
        hs.gmres_block(A, B, Pr=F, **GM)
        t3 = time.perf_counter()
    print(f"mf2, 32 columns: one mode-1 hs.gmres_block call {1e3 * (t3 - t2):.1f} ms, 32 hs.gmres calls {1e3 * (t1 - t0):.1f} ms")
    assert t3 - t2 <= t1 - t0


def test_zz_stored_factors_are_unchanged_and_the_mode_is_off(hs):
    """After everything above: hs.ldiv(F, b) on every handle still returns the bits it returned first, and no test left the switch on."""
    for label in list(_H):
        P, F, x0 = handle(hs, label)
        assert hs.ulv_mode(F) is False, label
        assert np.array_equal(hs.ldiv(F, P["b"].astype(F.dtype)), x0), label
