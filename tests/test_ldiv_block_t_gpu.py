"""The transposed / adjoint block solve (hs_ldiv_block_t_*, csrc/hs_solve_multi.hip + kernels_solve_multi_t.hip) on the MI355X: against
SuperLU's transposed and adjoint solves, against the looped single-vector transposed path of the same handle (hs_ldiv_t_*), and bitwise
against itself.  Structure, problems and tolerances as in test_ldiv_block_gpu.py.

The trapezoid form of a low-rank C (LowRank::Lp without Cd) is not reachable through a factorization: every flow that builds low-rank Gauss
transforms expands them (lowrank_expand after the compression in hs_compress.h and hs_hssfront.h, dense C_L / G in hs_mffront.h) and fails
with HS_ERR_NOMEM when the dense C cannot be allocated, and hs_ldiv_t_* refuses a transform without it.  The driver still serves it; the
kernel's side of it (input row map aside) is checked on the hook below."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from helpers import prepare, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-10
NRHS = (1, 2, 15, 16, 17, 33, 64, 70)  # below, at and across a 16-column MFMA tile and the chunk width


def _rand(n, k, cplx, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    if cplx:
        B = B + 1j * rng.standard_normal((n, k))
    return B


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for _, F, _ in _CACHE.values():
        F.free()
    _CACHE.clear()


def _exact(hs, kind, shape, nmax):
    key = (kind, shape, nmax)
    if key not in _CACHE:
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
        _CACHE[key] = (P, F, spla.splu(P["A"]))
    return _CACHE[key]


EXACT = [("convdiff", (30, 27), 40), ("convdiff_helmholtz", (30, 27), 40), ("convdiff", (24, 24, 24), 300), ("convdiff_helmholtz", (24, 24, 24), 300)]


def _kc():
    v = int(os.environ.get("HS_LDIV_BLOCK_COLS", "32") or 32)
    return v if v in (16, 32, 48, 64) else 32


def _worst_col(X, R):
    return max(relerr(X[:, j], R[:, j]) for j in range(X.shape[1]))


def _op(hs, F, trans):
    return hs.adjoint(F) if trans == 2 else hs.transpose(F)


@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_block_solve_matches_splu_and_the_looped_path(hs, kind, shape, nmax):
    P, F, lu = _exact(hs, kind, shape, nmax)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    assert abs(P["A"] - P["A"].T).max() > 0
    ni_max = max(F.node_info(i)[0] for i in range(F.nnodes))
    if len(shape) == 3:
        assert ni_max > 256 and ni_max % 256 != 0
    for trans in (1, 2):
        Ft = _op(hs, F, trans)
        for nrhs in NRHS:
            B = _rand(n, nrhs, cplx, 100 + nrhs)
            X = hs.ldiv_block_t(Ft, B)
            R = lu.solve(B, trans="TH"[trans - 1])
            e, ec = relerr(X, R), _worst_col(X, R)
            Xl = hs.ldiv(Ft, B)
            el = _worst_col(X, Xl)
            print(f"{kind} {shape} trans={trans} nrhs={nrhs}: vs splu {e:.2e} (worst column {ec:.2e}), vs looped {el:.2e}")
            assert X.shape == B.shape and e < TOL and ec < TOL
            assert el < 1e-11
        b = _rand(n, 1, cplx, 5)[:, 0]
        x = hs.ldiv_block_t(Ft, b)
        assert x.shape == (n,) and relerr(x, lu.solve(b, trans="TH"[trans - 1])) < TOL
    # a plain F goes through hs_ldiv_block_*
    B = _rand(n, 37, cplx, 9)
    assert np.array_equal(hs.ldiv_block_t(F, B), hs.ldiv_block(F, B))


@pytest.mark.parametrize("kind", ["convdiff", "convdiff_helmholtz"])
def test_determinism_and_column_independence(hs, kind, tmp_path):
    shape, nmax = (24, 24, 24), 300
    P, F, lu = _exact(hs, kind, shape, nmax)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    B = _rand(n, 70, cplx, 21)
    for trans in (1, 2) if cplx else (1,):
        Ft = _op(hs, F, trans)
        X = hs.ldiv_block_t(Ft, B)
        assert np.array_equal(X, hs.ldiv_block_t(Ft, B))
        perm = np.random.default_rng(3).permutation(70)
        assert np.array_equal(hs.ldiv_block_t(Ft, B[:, perm]), X[:, perm])
        for j in (0, 13, 31, 32, 47, 69):
            assert np.array_equal(hs.ldiv_block_t(Ft, B[:, j]), X[:, j])
            assert np.array_equal(hs.ldiv_block_t(Ft, B[:, j : j + 1])[:, 0], X[:, j])
    Ft = hs.transpose(F)
    X = hs.ldiv_block_t(Ft, B)
    # another chunk width (read once per process: a child process): not required to be bitwise equal
    np.save(tmp_path / "B.npy", B)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, "tests")!r})
import hsamd
from helpers import prepare
hs = hsamd.load()
P = prepare(hs, {shape!r}, kind={kind!r}, nmax={nmax}, rhs="randn")
F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
X = hs.ldiv_block_t(hs.transpose(F), np.load({str(tmp_path / "B.npy")!r}))
assert hs.ldiv_block_info(F)["chunks"] == 5
np.save({str(tmp_path / "X16.npy")!r}, X)
"""
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, HS_LDIV_BLOCK_COLS="16"), timeout=300)
    X16 = np.load(tmp_path / "X16.npy")
    assert _worst_col(X16, X) < 1e-11


@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_adjoint_against_transpose(hs, kind, shape, nmax):
    P, F, lu = _exact(hs, kind, shape, nmax)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    B = _rand(n, 35, cplx, 61)
    Xh = hs.ldiv_block_t(hs.adjoint(F), B)
    if cplx:
        Xt = np.conj(hs.ldiv_block_t(hs.transpose(F), np.conj(B)))
        e = _worst_col(Xh, Xt)
        print(f"{kind} {shape}: adjoint vs conj(transpose(conj)) worst column {e:.2e}, bitwise equal: {np.array_equal(Xh, Xt)}")
        assert e < 1e-12
    else:
        assert np.array_equal(Xh, hs.ldiv_block_t(hs.transpose(F), B))


@pytest.mark.parametrize("kind", ["convdiff", "convdiff_helmholtz"])
def test_abi_details(hs, kind):
    import torch

    P, F, lu = _exact(hs, kind, (24, 24, 24), 300)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    L = hs._lib.lib()
    fn = L.hs_ldiv_block_t_z if cplx else L.hs_ldiv_block_t_d
    fdev = L.hs_ldiv_block_dev_t_z if cplx else L.hs_ldiv_block_dev_t_d
    pf = hs._lib.p_f64
    k = 37
    B = _rand(n, k, cplx, 7)
    for trans in (1, 2):
        Ft = _op(hs, F, trans)
        ref = hs.ldiv_block_t(Ft, B)
        assert F.stats()["t_solve"] > 0
        assert relerr(ref, lu.solve(B, trans="TH"[trans - 1])) < TOL
        # ld > n, the padding rows untouched
        ld = n + 5
        Bp = np.zeros((ld, k), dtype=F.dtype, order="F")
        Bp[:n] = B
        Cp = np.full((ld + 3, k), 7.0, dtype=F.dtype, order="F")
        hs._lib.check(fn(F._h, trans, Cp.ctypes.data_as(pf), ld + 3, Bp.ctypes.data_as(pf), ld, n, k))
        assert np.array_equal(Cp[:n], ref) and np.all(Cp[n:] == 7.0)
        # C aliasing B
        Bq = Bp.copy(order="F")
        hs._lib.check(fn(F._h, trans, Bq.ctypes.data_as(pf), ld, Bq.ctypes.data_as(pf), ld, n, k))
        assert np.array_equal(Bq[:n], ref) and np.all(Bq[n:] == 0)
        Br = B.copy(order="F")
        assert hs.ldiv_block_t(Br, Ft, Br) is Br and np.array_equal(Br, ref)
        # info of the last call
        info = hs.ldiv_block_info(F)
        kc = _kc()
        esz = 16 if cplx else 8
        sum_fac = sum(float(F.node_info(i)[0]) ** 2 + 2.0 * F.node_info(i)[0] * F.node_info(i)[1] for i in range(F.nnodes))
        assert info["chunks"] == -(-k // kc)
        assert info["factor_bytes"] == info["chunks"] * sum_fac * esz
        assert 0 < info["flops_useful"] <= info["flops_executed"]
        assert info["seconds"] > 0 and info["workspace_bytes"] > 0
        assert info["seconds"] == F.stats()["t_solve"]
        # nrhs = 0 touches nothing
        Cz = np.full((n, 1), 3.0, dtype=F.dtype, order="F")
        hs._lib.check(fn(F._h, trans, Cz.ctypes.data_as(pf), n, Cz.ctypes.data_as(pf), n, n, 0))
        assert np.all(Cz == 3.0)
        assert hs.ldiv_block_t(Ft, np.zeros((n, 0), dtype=F.dtype)).shape == (n, 0)
        # the device form on a non-default stream: bitwise the host form
        dev = torch.device("cuda:0")
        s = torch.cuda.Stream(device=dev)
        dB = torch.from_numpy(np.asfortranarray(B).T.copy()).to(dev)  # row r of dB = column r of B (column-major n x k, ld n)
        dC = torch.empty_like(dB)
        with torch.cuda.stream(s):
            hs._lib.check(fdev(F._h, trans, C.c_void_p(dC.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, k, C.c_void_p(s.cuda_stream)))
        s.synchronize()
        assert np.array_equal(dC.cpu().numpy().T, ref)
        hs._lib.check(fdev(F._h, trans, C.c_void_p(dB.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, k, C.c_void_p(s.cuda_stream)))
        s.synchronize()
        assert np.array_equal(dB.cpu().numpy().T, ref)
        assert hs.ldiv_block_info(F)["seconds"] > 0
    # hs_ldiv_block_info reports the last block solve, whichever direction it had
    hs.ldiv_block(F, B[:, :3])
    assert hs.ldiv_block_info(F)["chunks"] == 1
    hs.ldiv_block_t(hs.transpose(F), B)
    assert hs.ldiv_block_info(F)["chunks"] == -(-k // _kc())


@pytest.mark.parametrize("kind", ["convdiff", "convdiff_helmholtz"])
def test_interleaving_with_the_other_solves(hs, kind):
    """The four paths share a handle (the two block solves share their work blocks as well) and every one repeats its own bits."""
    P, F, lu = _exact(hs, kind, (24, 24, 24), 300)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    B = _rand(n, 40, cplx, 31)
    b = _rand(n, 2, cplx, 32)
    Ft = hs.transpose(F)
    first = None
    for _ in range(2):
        got = (hs.ldiv(F, b), hs.ldiv(Ft, b), hs.ldiv_block(F, B), hs.ldiv_block_t(Ft, B), hs.ldiv_block_t(hs.adjoint(F), B))
        if first is None:
            first = got
        else:
            assert all(np.array_equal(x, y) for x, y in zip(first, got))
    assert relerr(first[2], lu.solve(B)) < TOL
    assert relerr(first[3], lu.solve(B, trans="T")) < TOL
    assert relerr(first[4], lu.solve(B, trans="H")) < TOL


COMPRESSED = [
    ("tol1e-4", "convdiff_helmholtz", (24, 24, 24), 300, dict(swlevel=2, swsize=8, atol=1e-4, rtol=1e-4)),
    ("tol1e-8", "convdiff", (24, 24, 24), 300, dict(swlevel=3, swsize=8, atol=1e-8, rtol=1e-8)),
    ("split", "convdiff", (24, 24, 24), 300, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, split_size=256)),
    ("mf-dense-D", "convdiff_helmholtz", (24, 24, 24), 300, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=True, leafsize=128)),
]


@pytest.mark.parametrize("label,kind,shape,nmax,kw", COMPRESSED, ids=[c[0] for c in COMPRESSED])
def test_compressed_handles_agree_with_the_looped_solve(hs, label, kind, shape, nmax, kw):
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], **kw)
    assert hs.maxrank(F) > 0  # low-rank Gauss transforms are in the solve
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    B = _rand(n, 35, cplx, 41)
    for trans in (1, 2) if cplx else (1,):
        Ft = _op(hs, F, trans)
        X = hs.ldiv_block_t(Ft, B)
        Xl = hs.ldiv(Ft, B)
        e = _worst_col(X, Xl)
        print(f"{label} trans={trans}: block vs looped, worst column {e:.2e}  maxrank {hs.maxrank(F)}")
        assert e < 1e-10
        assert np.array_equal(X, hs.ldiv_block_t(Ft, B))
    F.free()


def _untouched_after(hs, F, trans, want, n, dtype):
    L = hs._lib.lib()
    fn = L.hs_ldiv_block_t_z if np.dtype(dtype).kind == "c" else L.hs_ldiv_block_t_d
    pf = hs._lib.p_f64
    Bm = np.asfortranarray(_rand(n, 3, np.dtype(dtype).kind == "c", 1).astype(dtype))
    Cm = np.full((n, 3), 42.0, dtype=dtype, order="F")
    assert fn(F._h, trans, Cm.ctypes.data_as(pf), n, Bm.ctypes.data_as(pf), n, n, 3) == want
    assert np.all(Cm == 42.0)


def test_refusals(hs):
    L = hs._lib.lib()
    E = hs._lib
    P = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, hss_min=1024)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.ldiv_block_t(hs.transpose(F), P["b"])
    for trans in (0, 1, 2):
        _untouched_after(hs, F, trans, E.HS_ERR_UNSUPPORTED, P["A"].shape[0], F.dtype)
    F.free()
    P = prepare(hs, (24, 24, 24), kind="convdiff", nmax=300, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.ldiv_block_t(hs.adjoint(F), P["b"])
    for trans in (0, 1, 2):
        _untouched_after(hs, F, trans, E.HS_ERR_UNSUPPORTED, P["A"].shape[0], F.dtype)
    F.free()
    P, F, _ = _exact(hs, "convdiff", (30, 27), 40)
    n = P["A"].shape[0]
    _untouched_after(hs, F, 3, E.HS_ERR_ARGUMENT, n, F.dtype)
    _untouched_after(hs, F, -1, E.HS_ERR_ARGUMENT, n, F.dtype)
    with pytest.raises(TypeError, match="MethodError"):
        hs.ldiv_block_t(hs.transpose(F), P["b"] + 1j)
    with pytest.raises(hs.DimensionMismatch):
        hs.ldiv_block_t(hs.transpose(F), P["b"][:-1])
    with pytest.raises(TypeError):
        hs.ldiv_block_t(F)
    pf = hs._lib.p_f64
    Bm = np.asfortranarray(_rand(n, 2, False, 2))
    Cm = np.full((n, 2), 42.0, order="F")
    assert L.hs_ldiv_block_t_d(F._h, 1, Cm.ctypes.data_as(pf), n, Bm.ctypes.data_as(pf), n, n - 1, 2) == E.HS_ERR_DIMENSION
    assert L.hs_ldiv_block_t_d(F._h, 1, Cm.ctypes.data_as(pf), n - 1, Bm.ctypes.data_as(pf), n, n, 2) == E.HS_ERR_DIMENSION
    assert L.hs_ldiv_block_t_d(F._h, 1, None, n, Bm.ctypes.data_as(pf), n, n, 2) == E.HS_ERR_ARGUMENT  # null block
    Bz = np.asfortranarray(_rand(n, 2, True, 2))
    Cz = np.full((n, 2), 42.0, dtype=np.complex128, order="F")
    assert L.hs_ldiv_block_t_z(F._h, 2, Cz.ctypes.data_as(pf), n, Bz.ctypes.data_as(pf), n, n, 2) == E.HS_ERR_ARGUMENT  # eltype of F and B differ
    assert np.all(Cm == 42.0) and np.all(Cz == 42.0)


@pytest.mark.parametrize("cplx", [False, True])
def test_transposed_panel_product_kernel_lane_map_exact(hs, cplx):
    """The kernel alone (hsk_multi_prob_t_*) on small integers, where every product and sum is exact in Float64: exact equality with
    op(A).T @ X.  X is asymmetric (a swapped row / column map of the MFMA result, or an A operand and an X operand that disagree about
    which k a lane holds, cannot pass), M, K, kc ragged against the 16 x 16 x 4 tile, the 16-row chunk, the four-way split of K over the
    waves and the 64- / 32-row workgroup tile; lda = K + 3 and an odd lda (16-byte loads from 8-byte aligned columns)."""
    L = hs._lib.lib()
    fn = L.hsk_multi_prob_t_z if cplx else L.hsk_multi_prob_t_d
    pf = hs._lib.p_f64
    pi = C.POINTER(C.c_int32)
    dt = np.complex128 if cplx else np.float64
    rng = np.random.default_rng(17)

    def ints(shape):
        v = rng.integers(-7, 8, size=shape).astype(np.float64)
        return (v + 1j * rng.integers(-7, 8, size=shape)).astype(dt) if cplx else v

    cases = [(16, 4, 16), (1, 1, 1), (64, 32, 16), (65, 33, 17), (255, 31, 1), (300, 70, 33), (700, 130, 64), (129, 257, 47), (37, 5, 15), (100, 420, 32)]
    for M, K, kc in cases:
        for lda in (K + 3, K + 4):  # one of the two is odd
            for minus in (0, 1):
                for conj in (0, 1) if cplx else (0,):
                    A = np.asfortranarray(ints((lda, M)))
                    X = np.asfortranarray(ints((K + 2, kc)))
                    X[:K] += (np.arange(K)[:, None] * 2 - np.arange(kc)[None, :]) % 5  # asymmetric
                    C0 = np.asfortranarray(ints((M + 1, kc)))
                    Cm = C0.copy(order="F")
                    hs._lib.check(fn(M, K, kc, A.ctypes.data_as(pf), lda, X.ctypes.data_as(pf), K + 2, Cm.ctypes.data_as(pf), M + 1, minus, 0, conj, None))
                    At = (np.conj(A[:K]) if conj else A[:K]).T
                    want = (C0[:M] - At @ X[:K]) if minus else At @ X[:K]
                    assert np.array_equal(Cm[:M], want), (M, K, kc, lda, minus, conj)
                    assert np.array_equal(Cm[M:], C0[M:])
    # the transposed unit lower trapezoid of a packed sketch (LowRank::Lp: rows x r, here K x M)
    K, M, kc = 150, 40, 20
    for conj in (0, 1) if cplx else (0,):
        A = np.asfortranarray(ints((K, M)))
        X = np.asfortranarray(ints((K, kc)))
        C0 = np.asfortranarray(ints((M, kc)))
        Cm = C0.copy(order="F")
        hs._lib.check(fn(M, K, kc, A.ctypes.data_as(pf), K, X.ctypes.data_as(pf), K, Cm.ctypes.data_as(pf), M, 1, 1, conj, None))
        T = np.tril(np.conj(A) if conj else A, -1)
        T[np.arange(M), np.arange(M)] = 1
        assert np.array_equal(Cm, C0 - T.T @ X)
        # the row map that goes with the trapezoid (MultiProbT::xmap = LowRank::rperm): row k of A meets row map[k] of X
        xmap = rng.permutation(K).astype(np.int32)
        Cm = C0.copy(order="F")
        hs._lib.check(fn(M, K, kc, A.ctypes.data_as(pf), K, X.ctypes.data_as(pf), K, Cm.ctypes.data_as(pf), M, 1, 1, conj, xmap.ctypes.data_as(pi)))
        assert np.array_equal(Cm, C0 - T.T @ X[xmap])
    # ... and without the trapezoid, ragged against every tile, odd and even lda
    M, K, kc = 65, 33, 17
    for lda in (K + 3, K + 4):
        for minus in (0, 1):
            for conj in (0, 1) if cplx else (0,):
                A = np.asfortranarray(ints((lda, M)))
                X = np.asfortranarray(ints((K + 2, kc)))
                X[:K] += (np.arange(K)[:, None] * 2 - np.arange(kc)[None, :]) % 5
                C0 = np.asfortranarray(ints((M + 1, kc)))
                xmap = rng.permutation(K).astype(np.int32)
                Cm = C0.copy(order="F")
                hs._lib.check(fn(M, K, kc, A.ctypes.data_as(pf), lda, X.ctypes.data_as(pf), K + 2, Cm.ctypes.data_as(pf), M + 1, minus, 0, conj, xmap.ctypes.data_as(pi)))
                At = (np.conj(A[:K]) if conj else A[:K]).T
                want = (C0[:M] - At @ X[:K][xmap]) if minus else At @ X[:K][xmap]
                assert np.array_equal(Cm[:M], want), (lda, minus, conj)
                assert np.array_equal(Cm[M:], C0[M:])


def test_factors_are_not_read_once_per_column(hs):
    """A guard, not a target: 32 looped transposed solves read the factors 32 times, a block solve once, so the block solve takes at most
    half the time of the loop by a wide margin unless it falls back to a loop over the columns.  Device times (stats.t_solve), the two
    paths alternating in one process, median of 5 after a warm-up."""
    P = prepare(hs, (40, 40, 40), kind="poisson", rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
    Ft = hs.transpose(F)
    n = P["A"].shape[0]
    B = _rand(n, 32, False, 51)
    tb, tl = [], []
    for it in range(6):
        X = hs.ldiv_block_t(Ft, B)
        t1 = F.stats()["t_solve"]
        Xl = hs.ldiv(Ft, B)
        t2 = F.stats()["t_solve"]
        if it > 0:
            tb.append(t1)
            tl.append(t2)
    t_block, t_loop = float(np.median(tb)), float(np.median(tl))
    print(f"Poisson 40^3, nrhs = 32, transposed: block {t_block * 1e3:.3f} ms, looped {t_loop * 1e3:.3f} ms, ratio {t_loop / t_block:.1f}")
    assert _worst_col(X, Xl) < 1e-11
    assert t_block <= t_loop / 2
    F.free()
