"""Lockstep refined solves with error bounds for a block of right-hand sides on the MI355X (csrc/hs_refine_block.hip, hs_ldiv_refine_block_*):
against the block solve, the looped hs_ldiv_refine_*, scipy, and the NumPy restatements tests/normest_mirror.py and
tests/refine_block_mirror.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import normest_mirror as M
import refine_block_mirror as RB
from helpers import prepare, relerr

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CACHE = {}
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for _, F in _CACHE.values():
        F.free()
    _CACHE.clear()
    _RUNS.clear()


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


def _ops(hs, F, A, trans):
    op = (F, hs.transpose(F), hs.adjoint(F))[trans]
    opA = (A, A.T, A.conj().T)[trans].tocsr()
    opA.sort_indices()
    return op, opA, int(np.diff(opA.indptr).max()) + 1


EXACT = [("convdiff", (30, 27), 40), ("convdiff_helmholtz", (30, 27), 40), ("convdiff", (12, 12, 12), 100), ("convdiff_helmholtz", (12, 12, 12), 100)]


@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_exact_handles(hs, kind, shape, nmax):
    P, F = _factor(hs, kind, shape, nmax)
    A = P["A"]
    n = A.shape[0]
    cplx = F.dtype.kind == "c"
    for trans in (0, 1, 2):
        op, opA, nz = _ops(hs, F, A, trans)
        for nrhs in (35, 1):  # two chunks with a ragged second; a single column
            B = _rand(n, nrhs, cplx, 11 + trans)
            X0, berr0, ferr0, steps0 = hs.ldiv_refine_block(op, B, itmax=0)
            assert np.all(steps0 == 0) and np.array_equal(X0, hs.ldiv_block_t(op, B)), (trans, nrhs)
            X, berr, ferr, steps = hs.ldiv_refine_block(op, B)
            assert X.shape == (n, nrhs) and berr.shape == ferr.shape == steps.shape == (nrhs,)
            assert np.all(berr <= 10 * EPS), (trans, nrhs, berr.max())
            for c in range(nrhs):
                bn, _, _ = M.gerfs_berr(opA, X[:, c], B[:, c], nz)
                assert berr[c] == pytest.approx(bn, rel=1e-12), (trans, nrhs, c, berr[c], bn)
            assert np.all(ferr > 0) and np.all(np.isfinite(ferr))
    # a vector in, scalars out, as ldiv_refine
    x, be, fe, st = hs.ldiv_refine_block(F, B[:, 0])
    assert x.shape == (n,) and isinstance(be, float) and isinstance(fe, float) and isinstance(st, int)
    assert hs.ldiv_refine_block(F, B[:, 0], ferr=False)[2] is None


COMPRESSED = [("convdiff", 0), ("convdiff", 1), ("convdiff_helmholtz", 0), ("convdiff_helmholtz", 1), ("convdiff_helmholtz", 2)]
CKW = dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, leafsize=32)
NRHS, ZERO, COPY_OF, COPY = 35, 5, 3, 33  # column ZERO is all zero, column COPY repeats column COPY_OF (in another chunk)


def _block_rhs(n, cplx):
    B = _rand(n, NRHS, cplx, 8)
    B[:, ZERO] = 0.0
    B[:, COPY] = B[:, COPY_OF]
    return B


def _compressed_run(hs, kind, trans):
    """One lockstep call per (problem, op), shared by the tests below and left unchanged."""
    key = (kind, trans)
    if key not in _RUNS:
        P, F = _factor(hs, kind, (20, 20, 20), 200, **CKW)
        assert any(F.node_ranks(i)[0] for i in range(F.nnodes))  # at least one compressed front
        op, opA, nz = _ops(hs, F, P["A"], trans)
        B = _block_rhs(P["A"].shape[0], F.dtype.kind == "c")
        res = hs.ldiv_refine_block(op, B)
        info = hs.ldiv_refine_block_info()
        for a in res:
            a.setflags(write=False)
        _RUNS[key] = (P, F, op, opA, nz, B, res, info)
    return _RUNS[key]


@pytest.mark.parametrize("kind,trans", COMPRESSED)
def test_compressed_handles_refined_to_working_accuracy(hs, kind, trans):
    P, F, op, opA, nz, B, (X, berr, ferr, steps), info = _compressed_run(hs, kind, trans)
    n = P["A"].shape[0]
    nzc = [c for c in range(NRHS) if c != ZERO]
    X0, berr0, _, steps0 = hs.ldiv_refine_block(op, B, itmax=0, ferr=False)
    assert np.all(steps0 == 0) and np.array_equal(X0, hs.ldiv_block_t(op, B))
    print(f"{kind} trans={trans}: steps {steps.tolist()}, berr0 max {berr0[nzc].max():.1e} -> berr max {berr[nzc].max():.1e}")
    assert np.all(berr[nzc] <= 10 * EPS) and np.all(steps[nzc] > 0) and np.all(berr[nzc] * 1e4 <= berr0[nzc])
    for c in range(NRHS):
        bn, _, _ = M.gerfs_berr(opA, X[:, c], B[:, c], nz)
        assert berr[c] == pytest.approx(bn, rel=1e-12), (c, berr[c], bn)
    # the two copies
    assert np.array_equal(X[:, COPY], X[:, COPY_OF]) and (berr[COPY], ferr[COPY], steps[COPY]) == (berr[COPY_OF], ferr[COPY_OF], steps[COPY_OF])
    # columns freeze at different corrections (the zero column after one: berr = 1 by the safe1 guard, then no halving)
    assert len(set(steps.tolist())) >= 2, steps
    assert steps[ZERO] == 1 and berr[ZERO] == 1.0 and np.all(X[:, ZERO] == 0)
    # the refinement: the first solve and one block solve per lockstep correction; compaction shrinks them
    assert info["groups"] == 1 and info["max_active"] == NRHS and info["residual_launches"] == 1 + steps.max()
    est_calls = info["block_solves"] - (1 + steps.max())
    assert 2 <= est_calls <= 2 * (RB.EST_ITMAX + 1)
    assert info["column_applications"] - info["estimator_column_applications"] == NRHS + steps.sum()
    # against the looped entry point
    Xl, berrl, ferrl, stepsl = hs.ldiv_refine(op, B)
    cond = hs.condest(F, np.inf)
    assert np.all(np.abs(steps - stepsl) <= 1), (steps, stepsl)
    for c in nzc:
        assert relerr(X[:, c], Xl[:, c]) <= cond * 1e-13, (c, relerr(X[:, c], Xl[:, c]))
    assert np.all(Xl[:, ZERO] == 0)
    # ferr: a bound of the true forward error, the looped estimate within the estimator's factor of 3, the mirror's value
    lu = spla.splu(opA.tocsc())
    Xs = lu.solve(B)
    cplx = F.dtype.kind == "c"
    fwd, adj = RB._ops(lambda Y, tr: hs.ldiv_block_t({"N": F, "T": hs.transpose(F), "C": hs.adjoint(F)}[tr], np.asfortranarray(Y)), trans, cplx)
    V = np.zeros((n, NRHS))
    for c in range(NRHS):
        _, r, w = M.gerfs_berr(opA, X[:, c], B[:, c], nz)
        V[:, c] = RB._weights(r, w, nz)
    est = RB._estimate_lockstep(fwd, adj, V, 123, cplx, lambda kind_, cols: None)
    for c in range(NRHS):
        xn = M.cabs1(X[:, c]).max()
        true_ferr = np.abs(X[:, c] - Xs[:, c]).max() / (xn if xn != 0.0 else 1.0)
        mirror = est[c] / xn if xn != 0.0 else est[c]
        ratio = lambda a, b: a / b if b else float("inf")
        print(f"  column {c}: ferr {ferr[c]:.3e}, true {true_ferr:.3e} (ferr / true {ratio(ferr[c], true_ferr):.1f}), "
              f"ferr / looped {ratio(ferr[c], ferrl[c]):.3f}, ferr / mirror - 1 {ratio(ferr[c], mirror) - 1:.1e}")
        assert ferr[c] >= true_ferr, (c, ferr[c], true_ferr)
        assert ferrl[c] / 3 <= ferr[c] <= 3 * ferrl[c], (c, ferr[c], ferrl[c])
        assert ferr[c] == pytest.approx(mirror, rel=1e-8), (c, ferr[c], mirror)


@pytest.mark.parametrize("kind,trans", [("convdiff", 0), ("convdiff_helmholtz", 1), ("convdiff_helmholtz", 2)])
def test_determinism_and_column_independence(hs, kind, trans):
    P, F, op, opA, nz, B, (X, berr, ferr, steps), info = _compressed_run(hs, kind, trans)
    X2, berr2, ferr2, steps2 = hs.ldiv_refine_block(op, B)
    assert np.array_equal(X, X2) and np.array_equal(berr, berr2) and np.array_equal(ferr, ferr2) and np.array_equal(steps, steps2)
    perm = np.random.default_rng(3).permutation(NRHS)
    Xp, bp, fp, sp_ = hs.ldiv_refine_block(op, B[:, perm])
    assert np.array_equal(Xp, X[:, perm]) and np.array_equal(bp, berr[perm]) and np.array_equal(fp, ferr[perm]) and np.array_equal(sp_, steps[perm])
    sub = [34, ZERO, 0, 17, 32]
    Xq, bq, fq, sq = hs.ldiv_refine_block(op, B[:, sub])
    assert np.array_equal(Xq, X[:, sub]) and np.array_equal(bq, berr[sub]) and np.array_equal(fq, ferr[sub]) and np.array_equal(sq, steps[sub])
    x1, b1, f1, s1 = hs.ldiv_refine_block(op, B[:, 17])
    assert np.array_equal(x1, X[:, 17]) and (b1, f1, s1) == (berr[17], ferr[17], steps[17])


_GROUP_CHILD = """
import os, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import hsamd
from helpers import prepare
from test_refine_block_gpu import CKW, _block_rhs
hs = hsamd.load()
P = prepare(hs, (20, 20, 20), kind="convdiff_helmholtz", nmax=200, rhs="randn")
F = hs.factor(P["A"], P["nd"], P["nd_loc"], **CKW)
B = _block_rhs(P["A"].shape[0], True)
for op in (F, hs.transpose(F)):
    os.environ.pop("HS_REFINE_BLOCK_GROUP", None)
    a = hs.ldiv_refine_block(op, B)
    assert hs.ldiv_refine_block_info()["groups"] == 1
    os.environ["HS_REFINE_BLOCK_GROUP"] = "32"  # read per call
    b = hs.ldiv_refine_block(op, B)
    assert hs.ldiv_refine_block_info()["groups"] == 2 and hs.ldiv_refine_block_info()["max_active"] == 32
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
F.free()
print("GROUP OK")
"""


def test_group_width_does_not_change_the_bits(hs):
    code = _GROUP_CHILD % (ROOT, os.path.join(ROOT, "tests"))
    env = {k: v for k, v in os.environ.items() if k != "HS_REFINE_BLOCK_GROUP"}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "GROUP OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("kind,trans", [("convdiff", 0), ("convdiff_helmholtz", 2)])
def test_device_form_on_a_side_stream(hs, kind, trans):
    import torch

    P, F, op, opA, nz, B, (X, berr, ferr, steps), info = _compressed_run(hs, kind, trans)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    L = hs._lib.lib()
    dev = torch.device("cuda:0")
    ld = n + 3
    Bp = np.zeros((ld, NRHS), dtype=F.dtype, order="F")
    Bp[:n] = B
    dB = torch.from_numpy(Bp.T.copy()).to(dev)  # row j of dB = column j of Bp
    dX = torch.full_like(dB, 7.0)
    be, fe, st = np.zeros(NRHS), np.zeros(NRHS), np.zeros(NRHS, dtype=np.int64)
    s = torch.cuda.Stream(device=dev)
    fn = L.hs_ldiv_refine_block_dev_z if cplx else L.hs_ldiv_refine_block_dev_d
    with torch.cuda.stream(s):
        hs._lib.check(fn(F._h, trans, C.c_void_p(dX.data_ptr()), ld, C.c_void_p(dB.data_ptr()), ld, n, NRHS, 5, be.ctypes.data_as(hs._lib.p_f64),
                         fe.ctypes.data_as(hs._lib.p_f64), st.ctypes.data_as(hs._lib.p_i64), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    Xd = dX.cpu().numpy().T
    assert np.array_equal(Xd[:n], X) and np.all(Xd[n:] == 7.0)  # the padding rows are untouched
    assert np.array_equal(dB.cpu().numpy().T, Bp)
    assert np.array_equal(be, berr) and np.array_equal(fe, ferr) and np.array_equal(st, steps)


def test_refusals(hs):
    import torch

    L = hs._lib.lib()
    f64, i64p = hs._lib.p_f64, hs._lib.p_i64
    # mf = 2: interior blocks kept as HSS matrices -- the block solve does not serve them, and there is no fallback here
    P2 = prepare(hs, (20, 20, 20), kind="convdiff", nmax=200, rhs="randn")
    F2 = hs.factor(P2["A"], P2["nd"], P2["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    n2 = P2["A"].shape[0]
    b2 = np.asfortranarray(_rand(n2, 2, False, 1))
    x2 = np.full_like(b2, 7.0)
    berr, ferr, steps = np.zeros(2), np.zeros(2), np.zeros(2, dtype=np.int64)
    for op in (F2, hs.transpose(F2)):
        for fe in (True, False):
            with pytest.raises(hs.UnsupportedError, match="HSS"):
                hs.ldiv_refine_block(op, b2, ferr=fe)
    st = L.hs_ldiv_refine_block_d(F2._h, 0, x2.ctypes.data_as(f64), n2, b2.ctypes.data_as(f64), n2, n2, 2, 5, berr.ctypes.data_as(f64), None, steps.ctypes.data_as(i64p))
    assert st == hs._lib.HS_ERR_UNSUPPORTED and np.all(x2 == 7.0)
    F2.free()
    # argument errors on an exact factorization
    P, F = _factor(hs, "convdiff", (30, 27), 40)
    n = P["A"].shape[0]
    b = np.asfortranarray(_rand(n, 2, False, 2))
    x = np.full_like(b, 7.0)

    def call(fn=L.hs_ldiv_refine_block_d, trans=0, X=x.ctypes.data_as(f64), B=b.ctypes.data_as(f64), nn=n, nrhs=2, itmax=5):
        return fn(F._h, trans, X, n, B, n, nn, nrhs, itmax, berr.ctypes.data_as(f64), ferr.ctypes.data_as(f64), steps.ctypes.data_as(i64p))

    assert call(X=b.ctypes.data_as(f64)) == hs._lib.HS_ERR_ARGUMENT and b"alias" in L.hs_last_error()
    assert call(trans=3) == hs._lib.HS_ERR_ARGUMENT and b"trans" in L.hs_last_error()
    assert call(itmax=-1) == hs._lib.HS_ERR_ARGUMENT and b"itmax" in L.hs_last_error()
    assert call(fn=L.hs_ldiv_refine_block_z) == hs._lib.HS_ERR_ARGUMENT and b"MethodError" in L.hs_last_error()
    assert call(nn=n - 1) == hs._lib.HS_ERR_DIMENSION
    assert call(X=None) == hs._lib.HS_ERR_ARGUMENT
    with pytest.raises(TypeError, match="MethodError"):
        hs.ldiv_refine_block(F, b.astype(np.complex128))
    with pytest.raises(hs.DimensionMismatch):
        hs.ldiv_refine_block(F, b[:-1])
    # the device form: X inside B
    dB = torch.from_numpy(b.T.copy()).to("cuda:0")
    dX = torch.full_like(dB, 7.0)
    st = L.hs_ldiv_refine_block_dev_d(F._h, 0, C.c_void_p(dB.data_ptr() + 8 * n), n, C.c_void_p(dB.data_ptr()), n, n, 2, 5, berr.ctypes.data_as(f64),
                                      ferr.ctypes.data_as(f64), steps.ctypes.data_as(i64p), None)
    assert st == hs._lib.HS_ERR_ARGUMENT and b"alias" in L.hs_last_error()
    assert np.array_equal(dB.cpu().numpy().T, b)
    # nrhs = 0 touches nothing
    berr[:], ferr[:], steps[:] = 9.0, 9.0, 9
    assert call(nrhs=0) == 0
    st = L.hs_ldiv_refine_block_dev_d(F._h, 1, C.c_void_p(dX.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, 0, 5, None, None, None, None)
    assert st == 0 and torch.all(dX == 7.0)
    assert np.all(x == 7.0) and np.all(berr == 9.0) and np.all(ferr == 9.0) and np.all(steps == 9)
    Xe, be, fe, se = hs.ldiv_refine_block(F, np.zeros((n, 0)))
    assert Xe.shape == (n, 0) and be.shape == fe.shape == se.shape == (0,)
    # a refusal did no harm: the handle still solves
    assert relerr(P["A"] @ hs.ldiv(F, P["b"]), P["b"]) < 1e-12


def test_factors_are_read_per_chunk_not_per_column(hs):
    """A guard, not a target: with 32 columns and one correction the looped entry point reads the factors 64 times, the lockstep one twice.
    Device times of the two device entry points on the same block, alternating in one process, median of 3 after a warm-up."""
    import torch

    P = prepare(hs, (40, 40, 40), kind="poisson", rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
    n = P["A"].shape[0]
    L = hs._lib.lib()
    nrhs = 32
    dB = torch.from_numpy(np.ascontiguousarray(_rand(n, nrhs, False, 51).T)).to("cuda:0")
    dX, dXl = torch.zeros_like(dB), torch.zeros_like(dB)
    be, st = np.zeros(nrhs), np.zeros(nrhs, dtype=np.int64)
    bel, stl = np.zeros(nrhs), np.zeros(nrhs, dtype=np.int64)
    pf, pi = hs._lib.p_f64, hs._lib.p_i64
    tb, tl = [], []
    for it in range(4):
        hs._lib.check(L.hs_ldiv_refine_block_dev_d(F._h, 0, C.c_void_p(dX.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, nrhs, 1, be.ctypes.data_as(pf), None,
                                                   st.ctypes.data_as(pi), None))
        info = hs.ldiv_refine_block_info()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hs._lib.check(L.hs_ldiv_refine_dev_d(F._h, 0, C.c_void_p(dXl.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, nrhs, 1, bel.ctypes.data_as(pf), None,
                                             stl.ctypes.data_as(pi), None))
        e1.record()
        e1.synchronize()
        if it > 0:
            tb.append(info["seconds"])
            tl.append(e0.elapsed_time(e1) * 1e-3)
    assert info["block_solves"] == 1 + st.max() and info["groups"] == 1 and info["estimator_column_applications"] == 0
    assert info["column_applications"] == nrhs + st.sum()
    assert np.all(np.abs(st - stl) <= 1) and np.all(be <= 10 * EPS)
    t_block, t_loop = float(np.median(tb)), float(np.median(tl))
    print(f"Poisson 40^3, nrhs = 32, itmax = 1: lockstep {t_block * 1e3:.3f} ms, looped {t_loop * 1e3:.3f} ms, lockstep / looped {t_block / t_loop:.3f}")
    assert t_block / t_loop < 1
    F.free()
