"""The blocked multi-right-hand-side ldiv! (hs_ldiv_block_*, csrc/hs_solve_multi.hip + kernels_solve_multi.hip) on the MI355X: against
SuperLU, against the looped single-vector path of the same handle, and bitwise against itself.  Problems and factor cache as in
test_ldiv_transpose_gpu.py: fronts above 256 interior columns with ragged sizes, real and complex."""
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


@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_block_solve_matches_splu_and_the_looped_path(hs, kind, shape, nmax):
    P, F, lu = _exact(hs, kind, shape, nmax)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    ni_max = max(F.node_info(i)[0] for i in range(F.nnodes))
    if len(shape) == 3:
        assert ni_max > 256 and ni_max % 256 != 0
    for nrhs in NRHS:
        B = _rand(n, nrhs, cplx, 100 + nrhs)
        X = hs.ldiv_block(F, B)
        R = lu.solve(B)
        e, ec = relerr(X, R), _worst_col(X, R)
        Xl = hs.ldiv(F, B)
        el = _worst_col(X, Xl)
        print(f"{kind} {shape} nrhs={nrhs}: vs splu {e:.2e} (worst column {ec:.2e}), vs looped {el:.2e}")
        assert X.shape == B.shape and e < TOL and ec < TOL
        assert el < 1e-11
    b = _rand(n, 1, cplx, 5)[:, 0]
    x = hs.ldiv_block(F, b)
    assert x.shape == (n,) and relerr(x, lu.solve(b)) < TOL


@pytest.mark.parametrize("kind", ["convdiff", "convdiff_helmholtz"])
def test_determinism_and_column_independence(hs, kind, tmp_path):
    shape, nmax = (24, 24, 24), 300
    P, F, lu = _exact(hs, kind, shape, nmax)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    B = _rand(n, 70, cplx, 21)
    X = hs.ldiv_block(F, B)
    assert np.array_equal(X, hs.ldiv_block(F, B))
    perm = np.random.default_rng(3).permutation(70)
    assert np.array_equal(hs.ldiv_block(F, B[:, perm]), X[:, perm])
    for j in (0, 13, 31, 32, 47, 69):
        assert np.array_equal(hs.ldiv_block(F, B[:, j]), X[:, j])
        assert np.array_equal(hs.ldiv_block(F, B[:, j : j + 1])[:, 0], X[:, j])
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
X = hs.ldiv_block(F, np.load({str(tmp_path / "B.npy")!r}))
assert hs.ldiv_block_info(F)["chunks"] == 5
np.save({str(tmp_path / "X16.npy")!r}, X)
"""
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, HS_LDIV_BLOCK_COLS="16"), timeout=300)
    X16 = np.load(tmp_path / "X16.npy")
    assert _worst_col(X16, X) < 1e-11


@pytest.mark.parametrize("kind", ["convdiff", "convdiff_helmholtz"])
def test_abi_details(hs, kind):
    import torch

    P, F, lu = _exact(hs, kind, (24, 24, 24), 300)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    L = hs._lib.lib()
    fn = L.hs_ldiv_block_z if cplx else L.hs_ldiv_block_d
    fdev = L.hs_ldiv_block_dev_z if cplx else L.hs_ldiv_block_dev_d
    pf = hs._lib.p_f64
    k = 37
    B = _rand(n, k, cplx, 7)
    ref = hs.ldiv_block(F, B)
    assert F.stats()["t_solve"] > 0
    # ld > n, the padding rows untouched
    ld = n + 5
    Bp = np.zeros((ld, k), dtype=F.dtype, order="F")
    Bp[:n] = B
    Cp = np.full((ld + 3, k), 7.0, dtype=F.dtype, order="F")
    hs._lib.check(fn(F._h, 0, Cp.ctypes.data_as(pf), ld + 3, Bp.ctypes.data_as(pf), ld, n, k))
    assert np.array_equal(Cp[:n], ref) and np.all(Cp[n:] == 7.0)
    # C aliasing B
    Bq = Bp.copy(order="F")
    hs._lib.check(fn(F._h, 0, Bq.ctypes.data_as(pf), ld, Bq.ctypes.data_as(pf), ld, n, k))
    assert np.array_equal(Bq[:n], ref) and np.all(Bq[n:] == 0)
    Br = B.copy(order="F")
    assert hs.ldiv_block(Br, F, Br) is Br and np.array_equal(Br, ref)
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
    hs._lib.check(fn(F._h, 0, Cz.ctypes.data_as(pf), n, Cz.ctypes.data_as(pf), n, n, 0))
    assert np.all(Cz == 3.0)
    assert hs.ldiv_block(F, np.zeros((n, 0), dtype=F.dtype)).shape == (n, 0)
    # the device form on a non-default stream: bitwise the host form
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    dB = torch.from_numpy(np.asfortranarray(B).T.copy()).to(dev)  # row r of dB = column r of B (column-major n x k, ld n)
    dC = torch.empty_like(dB)
    with torch.cuda.stream(s):
        hs._lib.check(fdev(F._h, 0, C.c_void_p(dC.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, k, C.c_void_p(s.cuda_stream)))
    s.synchronize()
    assert np.array_equal(dC.cpu().numpy().T, ref)
    hs._lib.check(fdev(F._h, 0, C.c_void_p(dB.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, k, C.c_void_p(s.cuda_stream)))
    s.synchronize()
    assert np.array_equal(dB.cpu().numpy().T, ref)
    assert hs.ldiv_block_info(F)["seconds"] > 0


@pytest.mark.parametrize("kind", ["convdiff", "convdiff_helmholtz"])
def test_interleaving_with_the_single_vector_solves(hs, kind):
    """The block path leaves nothing behind in the single-vector workspaces or the exchange vectors of the dataflow sweeps."""
    P, F, lu = _exact(hs, kind, (24, 24, 24), 300)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    B = _rand(n, 40, cplx, 31)
    b = _rand(n, 2, cplx, 32)
    x0 = hs.ldiv(F, b)
    xt0 = hs.ldiv(hs.transpose(F), b)
    X0 = hs.ldiv_block(F, B)
    x1 = hs.ldiv(F, b)
    xt1 = hs.ldiv(hs.transpose(F), b)
    X1 = hs.ldiv_block(F, B)
    assert np.array_equal(X0, X1)
    assert np.array_equal(x0, x1) and np.array_equal(xt0, xt1)
    assert relerr(X0, lu.solve(B)) < TOL


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
    B = _rand(n, 35, F.dtype.kind == "c", 41)
    X = hs.ldiv_block(F, B)
    Xl = hs.ldiv(F, B)
    e = _worst_col(X, Xl)
    print(f"{label}: block vs looped, worst column {e:.2e}  maxrank {hs.maxrank(F)}")
    assert e < 1e-10
    assert np.array_equal(X, hs.ldiv_block(F, B))
    F.free()


def _untouched_after(hs, F, trans, want, n, dtype):
    L = hs._lib.lib()
    fn = L.hs_ldiv_block_z if np.dtype(dtype).kind == "c" else L.hs_ldiv_block_d
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
        hs.ldiv_block(F, P["b"])
    _untouched_after(hs, F, 0, E.HS_ERR_UNSUPPORTED, P["A"].shape[0], F.dtype)
    F.free()
    P = prepare(hs, (24, 24, 24), kind="convdiff", nmax=300, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.ldiv_block(F, P["b"])
    _untouched_after(hs, F, 0, E.HS_ERR_UNSUPPORTED, P["A"].shape[0], F.dtype)
    F.free()
    P, F, _ = _exact(hs, "convdiff", (30, 27), 40)
    n = P["A"].shape[0]
    _untouched_after(hs, F, 1, E.HS_ERR_UNSUPPORTED, n, F.dtype)
    _untouched_after(hs, F, 2, E.HS_ERR_UNSUPPORTED, n, F.dtype)
    _untouched_after(hs, F, 3, E.HS_ERR_ARGUMENT, n, F.dtype)
    with pytest.raises(hs.UnsupportedError):
        hs.ldiv_block(hs.transpose(F), P["b"])
    with pytest.raises(TypeError, match="MethodError"):
        hs.ldiv_block(F, P["b"] + 1j)
    with pytest.raises(hs.DimensionMismatch):
        hs.ldiv_block(F, P["b"][:-1])
    pf = hs._lib.p_f64
    Bm = np.asfortranarray(_rand(n, 2, False, 2))
    Cm = np.full((n, 2), 42.0, order="F")
    assert L.hs_ldiv_block_d(F._h, 0, Cm.ctypes.data_as(pf), n, Bm.ctypes.data_as(pf), n, n - 1, 2) == E.HS_ERR_DIMENSION
    Bz = np.asfortranarray(_rand(n, 2, True, 2))
    Cz = np.full((n, 2), 42.0, dtype=np.complex128, order="F")
    assert L.hs_ldiv_block_z(F._h, 0, Cz.ctypes.data_as(pf), n, Bz.ctypes.data_as(pf), n, n, 2) == E.HS_ERR_ARGUMENT  # eltype of F and B differ
    assert np.all(Cm == 42.0) and np.all(Cz == 42.0)


@pytest.mark.parametrize("cplx", [False, True])
def test_panel_product_kernel_lane_map_exact(hs, cplx):
    """The kernel alone (hsk_multi_prob_*) on small integers, where every product and sum is exact in Float64: exact equality with A @ X.
    X is asymmetric (a swapped row / column map of the MFMA result cannot pass), M, K, kc ragged against the 16 x 16 x 4 tile, the 16-column
    chunk, the four-way split of K over the waves and the 64- / 32-row workgroup tile."""
    L = hs._lib.lib()
    fn = L.hsk_multi_prob_z if cplx else L.hsk_multi_prob_d
    pf = hs._lib.p_f64
    dt = np.complex128 if cplx else np.float64
    rng = np.random.default_rng(17)

    def ints(shape):
        v = rng.integers(-7, 8, size=shape).astype(np.float64)
        return (v + 1j * rng.integers(-7, 8, size=shape)).astype(dt) if cplx else v

    cases = [(16, 4, 16), (1, 1, 1), (64, 32, 16), (65, 33, 17), (255, 31, 1), (300, 70, 33), (700, 130, 64), (129, 257, 47), (37, 5, 15), (100, 420, 32)]
    for M, K, kc in cases:
        for minus in (0, 1):
            A = np.asfortranarray(ints((M + 3, K))[: M + 3])
            X = np.asfortranarray(ints((K + 2, kc)))
            X[:K] += (np.arange(K)[:, None] * 2 - np.arange(kc)[None, :]) % 5  # asymmetric
            C0 = np.asfortranarray(ints((M + 1, kc)))
            Cm = C0.copy(order="F")
            hs._lib.check(fn(M, K, kc, A.ctypes.data_as(pf), M + 3, X.ctypes.data_as(pf), K + 2, Cm.ctypes.data_as(pf), M + 1, minus, 0, None))
            want = (C0[:M] - A[:M] @ X[:K]) if minus else A[:M] @ X[:K]
            assert np.array_equal(Cm[:M], want), (M, K, kc, minus)
            assert np.array_equal(Cm[M:], C0[M:])
    # the unit lower trapezoid of a packed sketch (LowRank::Lp)
    M, K, kc = 150, 40, 20
    A = np.asfortranarray(ints((M, K)))
    X = np.asfortranarray(ints((K, kc)))
    C0 = np.asfortranarray(ints((M, kc)))
    Cm = C0.copy(order="F")
    hs._lib.check(fn(M, K, kc, A.ctypes.data_as(pf), M, X.ctypes.data_as(pf), K, Cm.ctypes.data_as(pf), M, 1, 1, None))
    T = np.tril(A, -1)
    T[np.arange(K), np.arange(K)] = 1
    assert np.array_equal(Cm, C0 - T @ X)
    # the row map that goes with the trapezoid (MultiProb::cmap = LowRank::rperm): row i of the product belongs to row map[i] of C
    pi = C.POINTER(C.c_int32)
    cmap = rng.permutation(M).astype(np.int32)
    Cm = C0.copy(order="F")
    hs._lib.check(fn(M, K, kc, A.ctypes.data_as(pf), M, X.ctypes.data_as(pf), K, Cm.ctypes.data_as(pf), M, 1, 1, cmap.ctypes.data_as(pi)))
    want = C0.copy()
    want[cmap] = C0[cmap] - T @ X
    assert np.array_equal(Cm, want)
    # ... and without the trapezoid, ragged against every tile: with minus = 0 every row of C is written exactly once, rows past M stay
    M, K, kc = 65, 33, 17
    A = np.asfortranarray(ints((M + 3, K)))
    X = np.asfortranarray(ints((K + 2, kc)))
    X[:K] += (np.arange(K)[:, None] * 2 - np.arange(kc)[None, :]) % 5
    C0 = np.asfortranarray(ints((M + 1, kc)))
    cmap = rng.permutation(M).astype(np.int32)
    for minus in (0, 1):
        Cm = C0.copy(order="F")
        hs._lib.check(fn(M, K, kc, A.ctypes.data_as(pf), M + 3, X.ctypes.data_as(pf), K + 2, Cm.ctypes.data_as(pf), M + 1, minus, 0, cmap.ctypes.data_as(pi)))
        want = C0.copy()
        want[cmap] = (C0[cmap] - A[:M] @ X[:K]) if minus else A[:M] @ X[:K]
        assert np.array_equal(Cm, want), minus
        assert np.array_equal(Cm[M:], C0[M:])


def test_factors_are_not_read_once_per_column(hs):
    """A guard, not a target: 32 looped solves read the factors 32 times, a block solve once, so the block solve takes at most half the
    time of the loop by a wide margin unless it falls back to a loop over the columns.  Device times (stats.t_solve), the two paths
    alternating in one process, median of 5 after a warm-up."""
    P = prepare(hs, (40, 40, 40), kind="poisson", rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
    n = P["A"].shape[0]
    B = _rand(n, 32, False, 51)
    tb, tl = [], []
    for it in range(6):
        X = hs.ldiv_block(F, B)
        t1 = F.stats()["t_solve"]
        Xl = hs.ldiv(F, B)
        t2 = F.stats()["t_solve"]
        if it > 0:
            tb.append(t1)
            tl.append(t2)
    t_block, t_loop = float(np.median(tb)), float(np.median(tl))
    print(f"Poisson 40^3, nrhs = 32: block {t_block * 1e3:.3f} ms, looped {t_loop * 1e3:.3f} ms, ratio {t_loop / t_block:.1f}")
    assert _worst_col(X, Xl) < 1e-11
    assert t_block <= t_loop / 2
    F.free()
