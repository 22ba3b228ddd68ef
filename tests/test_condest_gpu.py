"""Norm and condition estimates and refined solves with error bounds on the MI355X (csrc/hs_condest.hip): hs_opnorm, hs_normestinv,
hs_condest and hs_ldiv_refine_*, against dense NumPy, scipy and the NumPy restatement of the estimator (tests/normest_mirror.py).

Poisson is symmetric, `convdiff` is not (A and A^T differ), `convdiff_helmholtz` is complex and nonsymmetric."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import normest_mirror as M
from helpers import prepare, relerr

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for _, F in _CACHE.values():
        F.free()
    _CACHE.clear()


def _factor(hs, kind, shape, nmax, **kw):
    key = (kind, shape, nmax, tuple(sorted(kw.items())))
    if key not in _CACHE:
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        F = hs.factor(P["A"], P["nd"], P["nd_loc"], **(kw or dict(swlevel=0)))
        _CACHE[key] = (P, F)
    return _CACHE[key]


def _rand(n, k, cplx, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    if cplx:
        B = B + 1j * rng.standard_normal((n, k))
    return B


EXACT = [("poisson", (30, 27), 40), ("convdiff", (30, 27), 40), ("convdiff_helmholtz", (30, 27), 40), ("convdiff", (12, 12, 12), 100)]


@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_exact_factor_condest_and_norms(hs, kind, shape, nmax):
    P, F = _factor(hs, kind, shape, nmax)
    A = P["A"]
    Ad = A.toarray()
    for p in (1, np.inf):
        assert hs.opnorm(F, p) == pytest.approx(spla.norm(A, p), rel=1e-14)
        assert hs.opnorm(hs.transpose(F), p) == pytest.approx(spla.norm(A.T, p), rel=1e-14)
        true = np.linalg.cond(Ad, p)
        est = hs.condest(F, p)
        assert est <= true * (1 + 1e-10) and est >= true / 3, (p, est, true)
        # transpose(F): cond_p(A^T) = cond_q(A)
        estT = hs.condest(hs.transpose(F), p)
        trueT = np.linalg.cond(Ad.T, p)
        assert estT <= trueT * (1 + 1e-10) and estT >= trueT / 3
    # the C entry point returns both factors
    c, na, ne = C.c_double(), C.c_double(), C.c_double()
    hs._lib.check(hs._lib.lib().hs_condest(F._h, 0, 2, C.byref(c), C.byref(na), C.byref(ne), None))
    assert na.value == hs.opnorm(F, np.inf) and c.value == na.value * ne.value
    assert ne.value == hs.opnormestinv(hs.transpose(F))


@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_estimator_matches_the_mirror(hs, kind, shape, nmax):
    P, F = _factor(hs, kind, shape, nmax)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    for trans, op in ((0, F), (1, hs.transpose(F)), (2, hs.adjoint(F))):
        for t in (1, 2, 3):
            est, ns = hs.opnormestinv(op, t=t, nsolves=True)
            ref, nref = M.normestinv(lambda X, tr: F.solve(X, tr), n, trans=trans, t=t, seed=123, cplx=cplx)
            assert est == pytest.approx(ref, rel=1e-10), (trans, t)
            assert ns == nref, (trans, t)
            # reproducible: bitwise the same
            assert hs.opnormestinv(op, t=t, nsolves=True) == (est, ns)
    assert hs.condest(F, 1) == hs.condest(F, 1)


def _replaced_values(A, cplx):
    """A's pattern with standard normal values and 3 added to the diagonal.  With the PDE values the estimator stops after 3-4 half-steps with
    the exact norm and never selects rows against a non-empty index history; with these it runs 4 half-steps for every op and t below, so the
    history-exclusion branch of the top-t selection runs once."""
    rng = np.random.default_rng(1)
    vals = rng.standard_normal(A.nnz)
    if cplx:
        vals = vals + 1j * rng.standard_normal(A.nnz)
    A2 = A.copy()
    A2.data[:] = vals
    A2.setdiag(A2.diagonal() + 3.0)
    assert A2.nnz == A.nnz
    return A2


# n = 9: one more row than t = 8, the candidate lists are mostly sentinels; n = 810; n = 2250 > 2048 rows per workgroup: two workgroups'
# candidate lists are merged
WIDE = [((3, 3), 100), ((30, 27), 40), ((50, 45), 40)]


@pytest.mark.parametrize("replaced", [False, True], ids=["pde", "randn"])
@pytest.mark.parametrize("kind", ["convdiff", "convdiff_helmholtz"])
@pytest.mark.parametrize("shape,nmax", WIDE)
def test_wide_estimator_matches_the_mirror(hs, shape, nmax, kind, replaced):
    """t = 8 with the largest itmax (the wide instantiation of the estimator kernels) and t = 2 at the same itmax, against the mirror."""
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    cplx = kind == "convdiff_helmholtz"
    A = _replaced_values(P["A"], cplx) if replaced else P["A"]
    n = A.shape[0]
    F = hs.factor(A, P["nd"], P["nd_loc"], swlevel=0)
    try:
        for trans, op in ((0, F), (1, hs.transpose(F)), (2, hs.adjoint(F))):
            for t in (8, 2):
                est, ns = hs.opnormestinv(op, t=t, itmax=16, nsolves=True)
                ref, nref = M.normestinv(lambda X, tr: F.solve(X, tr), n, trans=trans, t=t, itmax=16, seed=123, cplx=cplx)
                print(f"{kind} {shape} replaced={replaced} trans={trans} t={t}: est {est:.17g} mirror {ref:.17g} nsolves {ns} mirror {nref}")
                assert est == pytest.approx(ref, rel=1e-10), (trans, t)
                assert ns == nref, (trans, t)
                assert hs.opnormestinv(op, t=t, itmax=16, nsolves=True) == (est, ns)  # bitwise repeatable
    finally:
        F.free()


COMPRESSED = [("convdiff", (20, 20, 20), 200, (0, 1)), ("convdiff_helmholtz", (20, 20, 20), 200, (0, 1, 2))]
CKW = dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, leafsize=32)


@pytest.mark.parametrize("kind,shape,nmax,transes", COMPRESSED)
def test_compressed_factor_refined_to_working_accuracy(hs, kind, shape, nmax, transes):
    P, F = _factor(hs, kind, shape, nmax, **CKW)
    assert any(F.node_ranks(i)[0] for i in range(F.nnodes))  # at least one compressed front
    A = P["A"]
    n = A.shape[0]
    cplx = F.dtype.kind == "c"
    b = _rand(n, 1, cplx, 21)[:, 0]
    cond = hs.condest(F, np.inf)
    for trans in transes:
        op = (F, hs.transpose(F), hs.adjoint(F))[trans]
        opA = (A, A.T, A.conj().T)[trans].tocsr()
        nz = int(np.diff(opA.indptr).max()) + 1
        x, berr, ferr, steps = hs.ldiv_refine(op, b)
        x0, berr0, _, steps0 = hs.ldiv_refine(op, b, itmax=0, ferr=False)
        assert steps0 == 0 and np.array_equal(x0, hs.ldiv(op, b))
        assert berr <= 10 * EPS, (trans, berr)
        assert steps > 0 and berr * 1e4 <= berr0, (trans, berr, berr0)
        bn, _, _ = M.gerfs_berr(opA, x, b, nz)
        assert berr == pytest.approx(bn, rel=1e-12), (trans, berr, bn)
        xs = spla.spsolve(opA.tocsc(), b)
        assert relerr(x, xs) <= cond * 1e-13
        true_ferr = np.abs(x - xs).max() / M.cabs1(x).max()
        assert ferr >= true_ferr, (trans, ferr, true_ferr)
        print(f"{kind} trans={trans}: berr {berr0:.1e} -> {berr:.1e} in {steps} steps, ferr {ferr:.1e} (true {true_ferr:.1e}), cond ~ {cond:.1e}")
        # reproducible
        x2, berr2, ferr2, steps2 = hs.ldiv_refine(op, b)
        assert np.array_equal(x, x2) and (berr, ferr, steps) == (berr2, ferr2, steps2)


def test_exact_factor_itmax0_is_the_plain_solve(hs):
    P, F = _factor(hs, "convdiff_helmholtz", (30, 27), 40)
    b = _rand(P["A"].shape[0], 1, True, 4)[:, 0]
    for trans, op in ((0, F), (1, hs.transpose(F)), (2, hs.adjoint(F))):
        x, berr, ferr, steps = hs.ldiv_refine(op, b, itmax=0)
        assert steps == 0 and np.array_equal(x, hs.ldiv(op, b))
        assert berr < 1e-13 and 0 < ferr < 1e-10


@pytest.mark.parametrize("kind", ["convdiff", "convdiff_helmholtz"])
def test_multiple_right_hand_sides_host_and_device(hs, kind):
    import torch

    P, F = _factor(hs, kind, (20, 20, 20), 200, **CKW)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    B = _rand(n, 3, cplx, 8)
    X, berr, ferr, steps = hs.ldiv_refine(F, B)
    assert X.shape == (n, 3) and berr.shape == (3,) and np.all(berr <= 10 * EPS) and np.all(steps > 0)
    for j in range(3):
        xj, bj, fj, sj = hs.ldiv_refine(F, B[:, j])
        assert np.array_equal(xj, X[:, j]) and (bj, fj, sj) == (berr[j], ferr[j], steps[j])
    # device variant on a side stream, leading dimension > n
    L = hs._lib.lib()
    dev = torch.device("cuda:0")
    ld = n + 3
    Bp = np.zeros((ld, 3), dtype=F.dtype, order="F")
    Bp[:n] = B
    dB = torch.from_numpy(Bp.T.copy()).to(dev)  # row j of dB = column j of Bp
    dX = torch.zeros_like(dB)
    be, fe, st = np.zeros(3), np.zeros(3), np.zeros(3, dtype=np.int64)
    s = torch.cuda.Stream(device=dev)
    fn = L.hs_ldiv_refine_dev_z if cplx else L.hs_ldiv_refine_dev_d
    with torch.cuda.stream(s):
        hs._lib.check(fn(F._h, 0, C.c_void_p(dX.data_ptr()), ld, C.c_void_p(dB.data_ptr()), ld, n, 3, 5, be.ctypes.data_as(hs._lib.p_f64),
                         fe.ctypes.data_as(hs._lib.p_f64), st.ctypes.data_as(hs._lib.p_i64), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    Xd = dX.cpu().numpy().T
    assert np.array_equal(Xd[:n], X) and np.all(Xd[n:] == 0)
    assert np.array_equal(be, berr) and np.array_equal(fe, ferr) and np.array_equal(st, steps)


def test_refusals(hs):
    import torch

    L = hs._lib.lib()
    f64 = hs._lib.p_f64
    i64p = hs._lib.p_i64
    est, ns = C.c_double(), hs._lib.i64()
    # rank 0 of a two-rank factorization, made like hs.dist.StagedSolver makes it (one process: nothing is factored or solved)
    P = prepare(hs, (16, 16), kind="convdiff", nmax=20, rhs="randn")
    be = hs.dist.HipBackend(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=2, device=torch.device("cuda:0"), swlevel=0)
    assert L.hs_normestinv(be._h, 0, 2, 5, C.byref(est), C.byref(ns), None) == hs._lib.HS_ERR_UNSUPPORTED
    assert b"ranks" in L.hs_last_error()
    assert L.hs_condest(be._h, 1, 2, C.byref(est), None, None, None) == hs._lib.HS_ERR_UNSUPPORTED
    n = P["A"].shape[0]
    b = np.asfortranarray(P["b"])
    x = np.zeros_like(b)
    berr, ferr, steps = np.zeros(1), np.zeros(1), np.zeros(1, dtype=np.int64)
    args = (x.ctypes.data_as(f64), n, b.ctypes.data_as(f64), n, n, 1, 5, berr.ctypes.data_as(f64), None, steps.ctypes.data_as(i64p))
    assert L.hs_ldiv_refine_d(be._h, 0, *args) == hs._lib.HS_ERR_UNSUPPORTED and b"ranks" in L.hs_last_error()
    del be
    # mf = 2: interior blocks kept as HSS matrices -- no transposed solves, so no estimator and no ferr; refinement with trans = 0 still runs
    P2 = prepare(hs, (20, 20, 20), kind="convdiff", nmax=200, rhs="randn")
    F2 = hs.factor(P2["A"], P2["nd"], P2["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    with pytest.raises(hs.UnsupportedError, match="ULV"):
        hs.opnormestinv(F2)
    with pytest.raises(hs.UnsupportedError, match="ULV"):
        hs.condest(F2)
    with pytest.raises(hs.UnsupportedError, match="ULV"):
        hs.ldiv_refine(F2, P2["b"])  # ferr=True
    with pytest.raises(hs.UnsupportedError, match="ULV"):
        hs.ldiv_refine(hs.transpose(F2), P2["b"], ferr=False)
    x2, berr2, _, steps2 = hs.ldiv_refine(F2, P2["b"], ferr=False)
    assert berr2 <= 10 * EPS and relerr(P2["A"] @ x2, P2["b"]) < 1e-13
    F2.free()
    # argument errors on an exact factorization
    P, F = _factor(hs, "convdiff", (30, 27), 40)
    n = P["A"].shape[0]
    b = np.asfortranarray(P["b"])
    x = np.zeros_like(b)
    for t in (0, 9, -1):
        assert L.hs_normestinv(F._h, 0, t, 5, C.byref(est), None, None) == hs._lib.HS_ERR_ARGUMENT and b"t =" in L.hs_last_error()
        assert L.hs_condest(F._h, 1, t, C.byref(est), None, None, None) == hs._lib.HS_ERR_ARGUMENT
    for itmax in (0, -2):
        assert L.hs_normestinv(F._h, 0, 2, itmax, C.byref(est), None, None) == hs._lib.HS_ERR_ARGUMENT and b"itmax" in L.hs_last_error()
    for trans in (3, -1):
        assert L.hs_normestinv(F._h, trans, 2, 5, C.byref(est), None, None) == hs._lib.HS_ERR_ARGUMENT and b"trans" in L.hs_last_error()
    for p in (2, -1):
        assert L.hs_condest(F._h, p, 2, C.byref(est), None, None, None) == hs._lib.HS_ERR_ARGUMENT and b"p =" in L.hs_last_error()
        assert L.hs_opnorm(F._h, p, C.byref(est)) == hs._lib.HS_ERR_ARGUMENT
    args = lambda trans, nn, itmax: (F._h, trans, x.ctypes.data_as(f64), n, b.ctypes.data_as(f64), n, nn, 1, itmax, berr.ctypes.data_as(f64),
                                     ferr.ctypes.data_as(f64), steps.ctypes.data_as(i64p))
    assert L.hs_ldiv_refine_d(*args(0, n, -1)) == hs._lib.HS_ERR_ARGUMENT and b"itmax" in L.hs_last_error()
    assert L.hs_ldiv_refine_d(*args(5, n, 5)) == hs._lib.HS_ERR_ARGUMENT and b"trans" in L.hs_last_error()
    assert L.hs_ldiv_refine_d(*args(0, n - 1, 5)) == hs._lib.HS_ERR_DIMENSION
    assert L.hs_ldiv_refine_z(*args(0, n, 5)) == hs._lib.HS_ERR_ARGUMENT and b"MethodError" in L.hs_last_error()
    with pytest.raises(ValueError, match="ArgumentError"):
        hs.condest(F, p=2)
    # a refusal did no harm: the handle still solves
    assert relerr(P["A"] @ hs.ldiv(F, P["b"]), P["b"]) < 1e-12
