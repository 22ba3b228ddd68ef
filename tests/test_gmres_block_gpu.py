"""Lockstep GMRES on a block of right-hand sides (hs_gmres_block_*, csrc/hs_gmres_block.hip) on the MI355X: per column against `hs.gmres`
on the scenarios of test_gmres_gpu.py, the lockstep schedule through hs_gmres_block_info, bitwise determinism and column independence,
one column bitwise against `hs.gmres` (the same driver at width 1), the other paths of the ABI, the refusals, and the SpMM kernel alone on
exact integer data."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from gmres_block_mirror import rhs_mix
from helpers import prepare, relerr
from test_gmres_gpu import SCENARIOS

pytestmark = pytest.mark.gpu

NRHS = 40  # one full chunk of the block solve plus a ragged one
ZERO = 3   # the zero column of rhs_mix

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for P, Fs in _CACHE.values():
        for F in Fs.values():
            if F is not None:
                F.free()
    _CACHE.clear()


def _scenario(hs, i):
    if i not in _CACHE:
        name, copts = SCENARIOS[i]
        P = prepare(hs, name, rhs="randn") if isinstance(name, str) else prepare(hs, name[0], rhs="randn", **name[1])
        _CACHE[i] = (P, dict(exact=hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0), compressed=hs.factor(P["A"], P["nd"], P["nd_loc"], **copts), none=None))
    return _CACHE[i]


def _kw(F):
    return dict(Pr=F, reltol=1e-9, restart=30, maxiter=30 if F is not None else 45)


def _same(r1, r2):
    (X1, c1), (X2, c2) = r1, r2
    return np.array_equal(X1, X2) and all(a["iters"] == b["iters"] and a["isconverged"] == b["isconverged"] and a["resnorm"] == b["resnorm"] for a, b in zip(c1, c2))


@pytest.mark.parametrize("label", ["exact", "compressed", "none"])
@pytest.mark.parametrize("si", range(len(SCENARIOS)))
def test_every_column_matches_hs_gmres_and_the_schedule_is_lockstep(hs, si, label):
    P, Fs = _scenario(hs, si)
    F = Fs[label]
    A = P["A"]
    n = A.shape[0]
    B = rhs_mix(n, NRHS, np.iscomplexobj(A.data), seed=2)
    kw = _kw(F)
    X, chs = hs.gmres_block(A, B, log=True, **kw)
    info = hs.gmres_block_info()
    chunks_last = hs.ldiv_block_info(F)["chunks"] if F is not None else None
    assert X.shape == B.shape and len(chs) == NRHS
    near = 0
    its = []
    for c in range(NRHS):
        x1, c1 = hs.gmres(A, B[:, c], log=True, **kw)
        c2 = chs[c]
        its.append(c2["iters"])
        h1, h2 = np.array(c1["resnorm"]), np.array(c2["resnorm"])
        if c2["iters"] != c1["iters"]:
            # the only allowance: the deciding residual of the reference lies within a relative 1e-6 of tol_c; then one iteration more or less
            tol_c = max(kw["reltol"] * h1[0], 0.0)
            k = min(c1["iters"], c2["iters"])
            assert abs(c2["iters"] - c1["iters"]) == 1 and 0 < k < len(h1) and abs(h1[k] - tol_c) <= 1e-6 * tol_c, (label, c, c1["iters"], c2["iters"])
            near += 1
            m = min(len(h1), len(h2))
            h1, h2 = h1[:m], h2[:m]
        else:
            assert c2["isconverged"] == c1["isconverged"], (label, c)
            assert relerr(X[:, c], x1) < 1e-6, (label, c, relerr(X[:, c], x1))
        assert np.allclose(h1, h2, rtol=1e-6, atol=1e-12 * h1[0]), (label, c, h1, h2)
        if c2["isconverged"]:
            assert np.linalg.norm(A @ X[:, c] - B[:, c]) <= 1e-8 * np.linalg.norm(B[:, c]), (label, c)
    print(f"scenario {si} {label}: iterations {its}  columns within 1e-6 of their tolerance: {near}  info {info}")
    assert near <= 1
    assert its[ZERO] == 0 and chs[ZERO]["isconverged"] and not np.any(X[:, ZERO])
    # the schedule: one block application per lockstep step and per cycle end, not one per column and iteration
    assert info["groups"] == 1 and info["max_active"] == NRHS - 1 and info["seconds"] > 0 and info["workspace_bytes"] > 0
    assert info["cycles"] >= 1 and info["spmm_launches"] >= max(its) + info["cycles"]
    if F is not None:
        assert max(its) + 1 <= info["prec_calls"] <= max(its) + info["cycles"]
        assert info["prec_calls"] < sum(its)
        assert info["column_applications"] <= info["prec_calls"] * (NRHS - 1)
        assert chunks_last == -(-(NRHS - 1) // 32) or info["cycles"] > 1
    else:
        assert info["prec_calls"] == 0 and info["column_applications"] == 0


def test_columns_leave_and_the_block_solve_sees_compaction(hs):
    """GMRES(3) on 3-D Poisson with a loose compressed preconditioner (tolerance 0.3; with the oracle's factorization of that tolerance the
    columns of rhs_mix need 11 to 15 iterations): the columns finish in different cycles, the later cycles run on fewer columns, and the last
    block solve of the handle ran on the columns of the last cycle only."""
    P, _ = _scenario(hs, 2)
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=3, swsize=8, atol=0.3, rtol=0.3)
    A = P["A"]
    B = rhs_mix(A.shape[0], NRHS, False, seed=2)
    m = 3
    kw = dict(Pr=F, reltol=1e-9, restart=m, maxiter=30)
    X, chs = hs.gmres_block(A, B, log=True, **kw)
    info = hs.gmres_block_info()
    chunks = hs.ldiv_block_info(F)["chunks"]
    its = [c["iters"] for c in chs]
    print("restart 3, loosely compressed Poisson 24^3: iterations", its, info, "chunks of the last block solve", chunks)
    nz = [v for c, v in enumerate(its) if c != ZERO]
    assert max(nz) - min(nz) >= 2 and max(nz) > m and info["cycles"] >= 2
    assert info["prec_calls"] <= max(its) + info["cycles"] and info["prec_calls"] < sum(its)
    assert info["column_applications"] < info["prec_calls"] * (NRHS - 1)  # column-applications shrink as columns finish
    last_cycle = sum(1 for v in nz if v > m * (info["cycles"] - 1))  # a column that goes on runs all m steps of a cycle
    assert 0 < last_cycle < NRHS - 1
    assert chunks == -(-last_cycle // 32)
    for c in (0, 1, 5, 17, 39):
        x1, c1 = hs.gmres(A, B[:, c], log=True, **kw)
        assert c1["iters"] == its[c] and c1["isconverged"] == chs[c]["isconverged"] and relerr(X[:, c], x1) < 1e-6
        assert np.allclose(c1["resnorm"], chs[c]["resnorm"], rtol=1e-6, atol=1e-12 * c1["resnorm"][0])
    F.free()


@pytest.mark.parametrize("si", [2, 3])
def test_determinism_and_column_independence_bitwise(hs, si, monkeypatch):
    P, Fs = _scenario(hs, si)
    F = Fs["compressed"]
    A = P["A"]
    n = A.shape[0]
    cplx = np.iscomplexobj(A.data)
    kw = dict(Pr=F, reltol=1e-9, restart=5, maxiter=30, log=True)
    B = rhs_mix(n, NRHS, cplx, seed=2)
    ref = hs.gmres_block(A, B, **kw)
    assert _same(ref, hs.gmres_block(A, B, **kw))
    perm = np.random.default_rng(3).permutation(NRHS)
    Xp, cp = hs.gmres_block(A, B[:, perm], **kw)
    assert _same((Xp, cp), (ref[0][:, perm], [ref[1][j] for j in perm]))
    for j in (0, 5, 17, 32, 39):
        x, ch = hs.gmres_block(A, B[:, j], **kw)
        assert np.array_equal(x, ref[0][:, j]) and ch["resnorm"] == ref[1][j]["resnorm"] and ch["iters"] == ref[1][j]["iters"]
    # groups of 32 columns against one group of 70
    B70 = rhs_mix(n, 70, cplx, seed=4)
    one = hs.gmres_block(A, B70, **kw)
    assert hs.gmres_block_info()["groups"] == 1
    monkeypatch.setenv("HS_GMRES_BLOCK_GROUP", "32")
    grouped = hs.gmres_block(A, B70, **kw)
    assert hs.gmres_block_info()["groups"] == 3 and hs.gmres_block_info()["max_active"] <= 32
    monkeypatch.delenv("HS_GMRES_BLOCK_GROUP")
    assert _same(one, grouped)
    # without a preconditioner too
    kw0 = dict(reltol=1e-3, restart=5, maxiter=20, log=True)
    r0 = hs.gmres_block(A, B, **kw0)
    assert _same(r0, hs.gmres_block(A, B, **kw0))
    Xq, cq = hs.gmres_block(A, B[:, perm], **kw0)
    assert _same((Xq, cq), (r0[0][:, perm], [r0[1][j] for j in perm]))


@pytest.mark.parametrize("shape,kind,nmax", [((15, 15), "poisson", 20), ((15, 15), "helmholtz", 20), ((20, 20, 20), "helmholtz", 512)])
def test_one_column_is_one_column_bitwise(hs, shape, kind, nmax):
    """Without a preconditioner `hs.gmres` (hs_gmres_*, hs_gmres_t_*) and `hs.gmres_block` on a 1-D b do the same arithmetic: equal x,
    history, iteration count and flag, over several restart cycles, for A, transpose(A) and adjoint(A), from zero and from a guess.
    n = 225 is less than one 256-row workgroup, n = 8000 is ragged against the 256-row and the 1024-row tiles."""
    A, b, _ = hs.problems.make_problem(shape, kind=kind, nmax=nmax, rhs="randn")
    x0 = np.random.default_rng(5).standard_normal(A.shape[0]).astype(b.dtype)
    kw = dict(Pr=None, reltol=1e-3, restart=5, maxiter=20, log=True)
    for trans in (None, "T", "C"):
        for guess in (None, x0):
            x1, c1 = hs.gmres(A, b, x0=guess, trans=trans, **kw)
            x2, c2 = hs.gmres_block(A, b, X0=guess, trans=trans, **kw)
            what = (kind, shape, trans, guess is not None, c1["iters"], c2["iters"])
            assert c1["iters"] > kw["restart"], what  # more than one cycle
            assert np.array_equal(x1, x2), what
            assert c1["resnorm"] == c2["resnorm"] and c1["iters"] == c2["iters"] and c1["isconverged"] == c2["isconverged"], what


@pytest.mark.parametrize("si", [0, 1])
def test_other_paths_and_edge_cases(hs, si):
    import torch

    P, Fs = _scenario(hs, si)
    F = Fs["exact"]
    Fc = Fs["compressed"]
    A = P["A"]
    n = A.shape[0]
    cplx = np.iscomplexobj(A.data)
    dt = np.complex128 if cplx else np.float64
    k = 7
    B = rhs_mix(n, k, cplx, seed=6)
    kw = dict(Pr=Fc, reltol=1e-9, restart=30, maxiter=30, log=True)
    # initial guesses: the residual of the guess is the reference of reltol, as in hs.gmres
    X0 = np.asfortranarray(np.random.default_rng(7).standard_normal((n, k)).astype(dt))
    Xg, cg = hs.gmres_block(A, B, X0=X0, **kw)
    for c in (0, ZERO, 5):
        x1, c1 = hs.gmres(A, B[:, c], x0=X0[:, c], **kw)
        assert cg[c]["iters"] == c1["iters"] and cg[c]["isconverged"] == c1["isconverged"]
        if c == ZERO:  # b = 0: both solutions are what is left of the guess, 1e-9 of it, and have no digits in common; the residual is what counts
            assert c1["isconverged"] and np.linalg.norm(A @ Xg[:, c]) <= 1e-8 * np.linalg.norm(A @ X0[:, c])
        else:
            assert relerr(Xg[:, c], x1) < 1e-6
        assert np.allclose(cg[c]["resnorm"], c1["resnorm"], rtol=1e-6, atol=1e-12 * c1["resnorm"][0])
    # device pointers on a torch stream, leading dimensions above n: bitwise the host form, the padding untouched
    ref, cref = hs.gmres_block(A, B, **kw)
    L = hs._lib.lib()
    fn = L.hs_gmres_block_z if cplx else L.hs_gmres_block_d
    from hierarchicalsolvers_jl_amd.gmres import _csc_fields

    colptr, rowval, nz = _csc_fields(A, dt)
    pi = hs._lib.p_i64
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    ld = n + 3
    Bp = np.zeros((k, ld), dtype=dt)
    Bp[:, :n] = B.T
    dB = torch.from_numpy(Bp).to(dev)  # row r of dB = column r of B (column-major, ld n + 3)
    dX = torch.full((k, ld), 7.0, dtype=dB.dtype, device=dev)
    maxit = 30
    hist = np.zeros((maxit + 1, k), order="F")
    iters = np.zeros(k, dtype=np.int64)
    conv = np.zeros(k, dtype=np.int32)
    with torch.cuda.stream(s):
        hs._lib.check(fn(Fc._h, n, colptr.ctypes.data_as(pi), rowval.ctypes.data_as(pi), nz.ctypes.data_as(C.c_void_p), C.c_void_p(dB.data_ptr()), ld,
                         C.c_void_p(dX.data_ptr()), ld, k, 1, 0, 1e-9, 0.0, 30, maxit, hist.ctypes.data_as(hs._lib.p_f64), iters.ctypes.data_as(pi),
                         conv.ctypes.data_as(C.POINTER(C.c_int)), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    Xd = dX.cpu().numpy()
    assert np.array_equal(Xd[:, :n].T, ref) and np.all(Xd[:, n:] == 7.0)
    assert [int(v) for v in iters] == [c["iters"] for c in cref] and [bool(v) for v in conv] == [c["isconverged"] for c in cref]
    for c in range(k):
        assert [float(v) for v in hist[: iters[c] + 1, c]] == cref[c]["resnorm"]
    # nrhs = 0, a vector, an all-zero block
    assert hs.gmres_block(A, np.zeros((n, 0), dtype=dt), **kw)[0].shape == (n, 0)
    x, ch = hs.gmres_block(A, B[:, 1], **kw)
    assert x.shape == (n,) and isinstance(ch, dict) and np.array_equal(x, ref[:, 1])
    Xz, cz = hs.gmres_block(A, np.zeros((n, 3), dtype=dt), **kw)
    assert not np.any(Xz) and all(c["iters"] == 0 and c["isconverged"] and c["resnorm"] == [0.0] for c in cz)
    assert hs.gmres_block_info()["prec_calls"] == 0 and hs.gmres_block_info()["cycles"] == 0
    # maxiter exhaustion: three unpreconditioned iterations bring no non-zero column anywhere near 1e-12
    Xm, cm = hs.gmres_block(A, B, reltol=1e-12, restart=2, maxiter=3, log=True)
    assert all((c["iters"] == 3 and not c["isconverged"]) for j, c in enumerate(cm) if j != ZERO) and cm[ZERO]["isconverged"]
    for c in (0, 5):
        x1, c1 = hs.gmres(A, B[:, c], reltol=1e-12, restart=2, maxiter=3, log=True)
        assert c1["iters"] == 3 and np.allclose(cm[c]["resnorm"], c1["resnorm"], rtol=1e-6, atol=1e-12 * c1["resnorm"][0]) and relerr(Xm[:, c], x1) < 1e-6
    # one column exhausts maxiter while the others converge.  GMRES is invariant to the scale of b, so with an absolute tolerance of half of
    # ||b|| and the iteration count i1 that b needs for it as maxiter, b converges in i1 iterations and 1e6 b, which needs a relative 5e-7,
    # cannot (unpreconditioned, its residual has barely moved by then)
    b = B[:, 2]
    _, c1 = hs.gmres(A, b, reltol=0.5, restart=30, maxiter=45, log=True)
    i1 = c1["iters"]
    assert c1["isconverged"] and 1 <= i1 < 45 and c1["resnorm"][-1] > 1e-3 * c1["resnorm"][0]
    Xs, cs = hs.gmres_block(A, np.stack([b, 1e6 * b, b], axis=1), reltol=0.0, abstol=0.5 * np.linalg.norm(b), restart=30, maxiter=i1, log=True)
    assert [(c["iters"], c["isconverged"]) for c in cs] == [(i1, True), (i1, False), (i1, True)], [(c["iters"], c["isconverged"]) for c in cs]
    assert np.array_equal(Xs[:, 0], Xs[:, 2]) and relerr(Xs[:, 1], 1e6 * Xs[:, 0]) < 1e-10
    # interleaving with the other solves of the handle leaves their results unchanged
    b2 = rhs_mix(n, 2, cplx, seed=8)[:, ::-1].copy() + 1.0
    x0, X0b, g0 = hs.ldiv(Fc, b2), hs.ldiv_block(Fc, B), hs.gmres(A, b2[:, 0], Pr=Fc, reltol=1e-9, restart=30, maxiter=30, log=True)
    again = hs.gmres_block(A, B, **kw)
    info = hs.gmres_block_info()
    x1, X1b, g1 = hs.ldiv(Fc, b2), hs.ldiv_block(Fc, B), hs.gmres(A, b2[:, 0], Pr=Fc, reltol=1e-9, restart=30, maxiter=30, log=True)
    assert info["cycles"] >= 1 and hs.gmres_block_info() == info  # the figures are those of the last hs_gmres_block_* call: hs.gmres leaves them
    assert np.array_equal(again[0], ref) and np.array_equal(x0, x1) and np.array_equal(X0b, X1b)
    assert np.array_equal(g0[0], g1[0]) and g0[1]["resnorm"] == g1[1]["resnorm"]
    # the exact preconditioner: one step for every column
    Xe, ce = hs.gmres_block(A, B, Pr=F, reltol=1e-9, restart=30, maxiter=30, log=True)
    assert all(c["isconverged"] and c["iters"] <= 2 for c in ce)


def test_refusals(hs):
    L = hs._lib.lib()
    E = hs._lib
    from hierarchicalsolvers_jl_amd.gmres import _csc_fields

    # a handle whose interior blocks are HSS matrices: the block solve does not serve it, hs_gmres_* does; X untouched
    P = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, hss_min=1024)
    A = P["A"]
    n = A.shape[0]
    B = np.asfortranarray(rhs_mix(n, 3, False, seed=9))
    with pytest.raises(hs.UnsupportedError, match=r"hs_gmres_\*"):
        hs.gmres_block(A, B, Pr=F, reltol=1e-9, restart=30, maxiter=30)
    colptr, rowval, nz = _csc_fields(A, np.float64)
    pi = E.p_i64
    X = np.full((n, 3), 42.0, order="F")
    iters = np.zeros(3, dtype=np.int64)
    conv = np.zeros(3, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.hs_gmres_block_d(F._h, n, colptr.ctypes.data_as(pi), rowval.ctypes.data_as(pi), vp(nz), vp(B), n, vp(X), n, 3, 0, 0, 1e-9, 0.0, 30, 30, None,
                            iters.ctypes.data_as(pi), conv.ctypes.data_as(C.POINTER(C.c_int)), None)
    assert rc == E.HS_ERR_UNSUPPORTED and np.all(X == 42.0)
    x, ch = hs.gmres(A, B[:, 0], Pr=F, reltol=1e-9, restart=30, maxiter=30, log=True)  # the path that serves it
    assert ch["iters"] >= 1
    F.free()
    # a real factorization cannot precondition a complex system; a restart above the limit
    Pc = prepare(hs, (15, 15), kind="helmholtz", nmax=20, rhs="randn")
    Pr = prepare(hs, (15, 15), kind="poisson", nmax=20, rhs="randn")
    Fr = hs.factor(Pr["A"], Pr["nd"], Pr["nd_loc"], swlevel=0)
    Fz = hs.factor(Pc["A"], Pc["nd"], Pc["nd_loc"], swlevel=0)
    Bz = rhs_mix(Pc["A"].shape[0], 3, True, seed=9)
    with pytest.raises(hs.DimensionMismatch):
        hs.gmres_block(Pc["A"], Bz, Pr=Fr, reltol=1e-9, restart=30, maxiter=10)
    with pytest.raises(ValueError):
        hs.gmres_block(Pc["A"], Bz, Pr=Fz, restart=1000, maxiter=10)
    with pytest.raises(hs.DimensionMismatch):
        hs.gmres_block(Pc["A"], Bz[:-1], Pr=Fz, maxiter=10)
    Fr.free()
    Fz.free()


@pytest.mark.parametrize("cplx", [False, True])
def test_spmm_kernel_exact_on_integers(hs, cplx):
    """The kernel alone (hsk_spmm_*) on small integers, where every product and sum is exact in Float64: equality with SciPy for ragged n
    (against the 256-row tile) and nrhs 1, 17, 40 (against the 8- / 4-column register chunk), both forms, leading dimensions above n."""
    L = hs._lib.lib()
    fn = L.hsk_spmm_z if cplx else L.hsk_spmm_d
    dt = np.complex128 if cplx else np.float64
    rng = np.random.default_rng(11)
    pi = hs._lib.p_i64
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def ints(shape):
        v = rng.integers(-7, 8, size=shape).astype(np.float64)
        return (v + 1j * rng.integers(-7, 8, size=shape)).astype(dt) if cplx else v

    for n in (1, 255, 257, 1000, 2049):
        pat = sp.random(n, n, density=min(1.0, 9.0 / n), random_state=5, format="csc") + sp.eye(n, format="csc")
        A = sp.csc_matrix((ints(pat.nnz), pat.indices, pat.indptr), shape=(n, n))
        A.sort_indices()
        colptr, rowval, nz = A.indptr.astype(np.int64) + 1, A.indices.astype(np.int64) + 1, np.ascontiguousarray(A.data, dtype=dt)
        for nrhs in (1, 17, 40):
            X = np.asfortranarray(ints((n + 2, nrhs)))
            X[:n] += (np.arange(n)[:, None] - 2 * np.arange(nrhs)[None, :]) % 5  # columns differ: a swapped column map cannot pass
            Bm = np.asfortranarray(ints((n + 1, nrhs)))
            for minus in (0, 1):
                Y0 = np.asfortranarray(ints((n + 3, nrhs)))
                Y = Y0.copy(order="F")
                hs._lib.check(fn(n, colptr.ctypes.data_as(pi), rowval.ctypes.data_as(pi), vp(nz), vp(X), n + 2, vp(Bm) if minus else None, n + 1, vp(Y), n + 3, nrhs))
                want = (Bm[:n] - A @ X[:n]) if minus else A @ X[:n]
                assert np.array_equal(Y[:n], want), (n, nrhs, minus)
                assert np.array_equal(Y[n:], Y0[n:])
