"""The stored factorization applied as an operator (hs_mul_*, hs_factor_error_*; csrc/hs_solve_multi.hip: hs_mul_run,
csrc/kernels_solve_multi_mul.hip, csrc/hs_mul.hip) on the MI355X: the triangular products alone on exact integer data, the product of exact
handles against op(A) X, the round trip with the block solve, the adjoint identity, the bitwise properties, hs.factor_error, the refusals.
The problems are those of tests/test_f32_gpu.py (EXACT, COMPRESSED) and one real indefinite matrix whose fronts pivot.

Bounds.
 * MIRROR_ERROR: the worst-column error of the NumPy mirror (tests/mul_mirror.py over the oracle's exact factors, 70 columns, the three
   trans) against op(A) X on each problem, measured on the CPU.  The device is held to 100 times that (its own pivot sequence and
   summation order), capped by the project's TOL = 1e-10.
 * round trip: n eps cond_1, cond_1 = hs.condest of the same handle and direction: the block solve is backward stable, so
   op(F) x - b = -dF x with |dF| of the order of eps |F| (derived in tests/test_mul_host.py, not measured).
 * adjoint identity: tests/test_ulv_t_gpu.py's normalisation.  Its ADJOINT_BOUND is 3.13e-16; the NumPy mirror gives 4.67e-17 for this
   identity on convdiff_helmholtz 24^3 (exact factors, 35 columns), and 10 times that, 4.67e-16, is the larger one: it is the bound used.
 * hs.factor_error with k = 32 default probes within a factor 2 of ||A - F||_F / ||A||_F: the Hutchinson estimate of the squared norm has
   a relative deviation of about sqrt(2 / k) = 0.25, so a factor 2 on the norm (4 on its square) is a condition, not a measurement.  On
   the CPU, with E = A - (the mirror with its low-rank pairs truncated at 1e-2, 1e-4, 1e-6) on the 30 x 27 Helmholtz problem, the NumPy
   restatement of the same +-1 probes gave ratios 1.09, 1.00, 0.96 for seed 0 (0.92 .. 1.07 over seeds 0, 1, 2)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import prepare, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-10
EPS = np.finfo(np.float64).eps
NRHS = (1, 2, 15, 16, 17, 33, 64, 70)  # tests/test_ldiv_block_gpu.py: below, at and across a 16-column MFMA tile and the chunk width
CKW = dict(swlevel=2, swsize=8, atol=1e-4, rtol=1e-4)
# label -> (kind, shape, nmax, shift, factor options)
HANDLES = {
    "2d-real": ("convdiff", (30, 27), 40, 0.0, None),
    "2d-complex": ("convdiff_helmholtz", (30, 27), 40, 0.0, None),
    "3d-complex": ("convdiff_helmholtz", (24, 24, 24), 300, 0.0, None),
    "2d-indefinite": ("poisson", (30, 27), 40, 0.35, None),  # poisson - 0.35 I as in tests/test_selinv_gpu.py: rows moved by pivoting
    "3d-complex-tol1e-4": ("convdiff_helmholtz", (24, 24, 24), 300, 0.0, CKW),
}
EXACT = ["2d-real", "2d-complex", "3d-complex", "2d-indefinite"]
COMPRESSED = "3d-complex-tol1e-4"
# measured on the CPU with tests/mul_mirror.py (see above)
MIRROR_ERROR = {"2d-real": 2.0e-16, "2d-complex": 3.7e-15, "3d-complex": 6.0e-16, "2d-indefinite": 6.3e-13}
ADJOINT_MIRROR = 4.67e-17
ADJOINT_BOUND = 10 * ADJOINT_MIRROR
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for _, F in _CACHE.values():
        F.free()
    _CACHE.clear()


def _handle(hs, label):
    if label not in _CACHE:
        kind, shape, nmax, shift, kw = HANDLES[label]
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        if shift:
            P["A"] = sp.csc_matrix(P["A"] - shift * sp.identity(P["A"].shape[0]))
            P["A"].sort_indices()
        _CACHE[label] = (P, hs.factor(P["A"], P["nd"], P["nd_loc"], **(kw or dict(swlevel=0))))
    return _CACHE[label]


def _rand(n, k, cplx, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    return B + 1j * rng.standard_normal((n, k)) if cplx else B


def _op(hs, F, t):
    return (F, hs.transpose(F), hs.adjoint(F))[t]


def _opmat(A, t):
    return (A, A.T, A.conj().T)[t]


def _worst_col(X, R):
    return max(relerr(X[:, j], R[:, j]) for j in range(X.shape[1]))


# ---- 1. the triangular products alone ------------------------------------------------------------------------------------------------------
SIZES = (1, 15, 16, 17, 63, 64, 65, 130, 257)  # across a 16-column chunk, the 4-wave split, the 64- / 32-row tile and 256
KCS = (1, 16, 17, 33, 64)
TALL = 37  # the trapezoid case: 37 more rows than columns


def _tri_call(hs, name, cplx, M, K, kc, A, X, C0, plus, tri, conj, mp):
    fn = getattr(hs._lib.lib(), name + ("_z" if cplx else "_d"))
    p = hs._lib.p_f64
    Cm = np.array(C0, order="F")
    m = None if mp is None else mp.ctypes.data_as(C.POINTER(C.c_int32))
    args = [M, K, kc, A.ctypes.data_as(p), A.shape[0], X.ctypes.data_as(p), X.shape[0], Cm.ctypes.data_as(p), Cm.shape[0], plus, tri]
    if name.endswith("_t"):
        args.append(conj)
    hs._lib.check(fn(*args, m))
    return Cm


def _tri_data(rng, rows, cols, kx, kc, mout, cplx, tri):
    """(A with NaN wherever the product must not look, its triangle as the product means it, X, C0): small integers, every sum exact."""

    def draw(shape):
        v = rng.integers(-3, 4, size=shape).astype(np.float64)
        return v + 1j * rng.integers(-3, 4, size=shape) if cplx else v

    T = draw((rows, cols))
    i, j = np.arange(rows)[:, None], np.arange(cols)[None, :]
    keep = (i > j) if tri == 1 else (i <= j)
    A = np.full((rows + 3, cols), complex(np.nan, np.nan) if cplx else np.nan, dtype=T.dtype, order="F")  # the rows of the padding too
    A[:rows] = np.where(keep, T, np.nan)
    T = np.where(keep, T, 0)
    if tri == 1:
        T[np.arange(min(rows, cols)), np.arange(min(rows, cols))] = 1
    X = np.asfortranarray(draw((kx + 2, kc)))
    X[:kx] += (np.arange(kx)[:, None] * 2 - np.arange(kc)[None, :]) % 5  # asymmetric: a swapped row / column map cannot pass
    return A, T, X, np.asfortranarray(draw((mout + 1, kc)))


def _tri_shapes():
    for s in SIZES:
        yield s, s
    yield 64 + TALL, 64
    yield 130 + TALL, 130


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_triangular_products_are_exact_and_read_their_triangle_only(hs, cplx):
    """hsk_multi_tri_*: C = tri(A) X and C + tri(A) X, A M x K read in place, on small integers: equality with NumPy's product.  The other
    triangle of A (and, for the unit trapezoid, the diagonal) holds NaN: a kernel that reads it and multiplies by zero, or that puts a
    skipped chunk in the wrong place, fails."""
    rng = np.random.default_rng(41)
    for M, K in _tri_shapes():
        for kc in KCS:
            for tri in (1, 2):
                A, T, X, C0 = _tri_data(rng, M, K, K, kc, M, cplx, tri)
                for plus in (0, 1):
                    for use_map in (False, True):
                        mp = rng.permutation(M).astype(np.int32) if use_map else None
                        want = C0.copy()
                        rows = np.arange(M) if mp is None else mp
                        want[rows] = (C0[rows] if plus else 0) + T @ X[:K]
                        got = _tri_call(hs, "hsk_multi_tri", cplx, M, K, kc, A, X, C0, plus, tri, 0, mp)
                        assert np.array_equal(got, want), (M, K, kc, tri, plus, use_map)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_transposed_triangular_products_are_exact_and_read_their_triangle_only(hs, cplx):
    """hsk_multi_tri_t_*: C = op(tri(A))^T X and C + op(tri(A))^T X, A K x M, with and without conj and the row map of X."""
    rng = np.random.default_rng(43)
    for K, M in _tri_shapes():
        for kc in KCS:
            for tri in (1, 2):
                A, T, X, C0 = _tri_data(rng, K, M, K, kc, M, cplx, tri)
                for plus in (0, 1):
                    for conj in ((0, 1) if cplx else (0,)):
                        for use_map in (False, True):
                            mp = rng.permutation(K).astype(np.int32) if use_map else None
                            Xk = X[:K] if mp is None else X[mp]
                            want = C0.copy()
                            want[:M] = (C0[:M] if plus else 0) + (T.conj() if conj else T).T @ Xk
                            got = _tri_call(hs, "hsk_multi_tri_t", cplx, M, K, kc, A, X, C0, plus, tri, conj, mp)
                            assert np.array_equal(got, want), (M, K, kc, tri, plus, conj, use_map)


# ---- 2. exact handles against op(A) X -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", EXACT)
def test_product_of_an_exact_factorization_is_the_matrix(hs, label):
    P, F = _handle(hs, label)
    A = P["A"]
    n = A.shape[0]
    cplx = F.dtype.kind == "c"
    bound = min(100 * MIRROR_ERROR[label], TOL)
    ni_max = max(F.node_info(i)[0] for i in range(F.nnodes))
    if len(HANDLES[label][1]) == 3:
        assert ni_max > 256 and ni_max % 256 != 0
    if cplx or HANDLES[label][3]:
        moved = sum(int((F.node_blocks(k)["rperm"] != np.arange(F.node_info(k)[0])).sum()) for k in range(F.nnodes))
        print(f"{label}: rows moved by pivoting: {moved}")
        if label != "3d-complex":  # (the 24^3 Helmholtz fronts keep their row order; the 2-D one and the shifted Poisson matrix do not)
            assert moved > 0
    worst = 0.0
    for t in (0, 1, 2):
        Ft, At = _op(hs, F, t), _opmat(A, t)
        for nrhs in NRHS:
            X = _rand(n, nrhs, cplx, 200 + nrhs)
            Y = hs.mul(Ft, X)
            e = _worst_col(Y, At @ X)
            worst = max(worst, e)
            assert Y.shape == X.shape and e < bound, (label, t, nrhs, e, bound)
        x = _rand(n, 1, cplx, 6)[:, 0]
        y = hs.mul(Ft, x)
        assert y.shape == (n,) and relerr(y, At @ x) < bound
    print(f"{label}: hs.mul against op(A) X, worst column over trans and nrhs {worst:.2e} (bound {bound:.1e})")


# ---- 3. round trip with the block solve ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(HANDLES))
def test_round_trip_with_the_block_solve(hs, label):
    P, F = _handle(hs, label)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    B = _rand(n, 40, cplx, 51)
    for t in (0, 1, 2):
        Ft = _op(hs, F, t)
        bound = n * EPS * hs.condest(Ft, 1)
        e1 = _worst_col(hs.mul(Ft, hs.ldiv_block_t(Ft, B)), B)
        e2 = _worst_col(hs.ldiv_block_t(Ft, hs.mul(Ft, B)), B)
        print(f"{label} trans={t}: mul(ldiv(B)) vs B {e1:.2e}, ldiv(mul(X)) vs X {e2:.2e} (bound n eps cond_1 = {bound:.2e})")
        assert e1 < bound and e2 < bound


# ---- 4. adjoint identity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2])
def test_adjoint_identity_on_the_compressed_handle(hs, t):
    """<F X, Y> = <X, op(F) Y> for the compressed factorization: whatever F approximates, its transpose and adjoint are those of F."""
    P, F = _handle(hs, COMPRESSED)
    n = P["A"].shape[0]
    X, Y = _rand(n, 35, True, 11), _rand(n, 35, True, 12)
    tt = (lambda Q: Q.conj().T) if t == 2 else (lambda Q: Q.T)
    d = np.linalg.norm(tt(Y) @ hs.mul(F, X) - tt(hs.mul(_op(hs, F, t), Y)) @ X) / (np.linalg.norm(X) * np.linalg.norm(Y))
    print(f"{COMPRESSED} trans={t}: defect of the adjoint identity {d:.2e} (bound {ADJOINT_BOUND:.2e})")
    assert d <= ADJOINT_BOUND


# ---- 5. bits ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["3d-complex", COMPRESSED, "2d-indefinite"])
def test_bitwise_properties(hs, label):
    import torch

    P, F = _handle(hs, label)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    L = hs._lib.lib()
    fn = L.hs_mul_z if cplx else L.hs_mul_d
    pf = hs._lib.p_f64
    k = 70
    X = _rand(n, k, cplx, 61)
    perm = np.random.default_rng(62).permutation(k)
    for t in (0, 1, 2):
        Ft = _op(hs, F, t)
        ref = hs.mul(Ft, X)
        assert np.array_equal(ref, hs.mul(Ft, X))  # two calls
        assert np.array_equal(hs.mul(Ft, X[:, perm]), ref[:, perm])  # a permuted block
        for j in (0, 31, 32, 69):  # a column alone
            assert np.array_equal(hs.mul(Ft, X[:, j]), ref[:, j])
            assert np.array_equal(hs.mul(Ft, X[:, j : j + 1])[:, 0], ref[:, j])
        # C aliasing B, and ld > n with the padding rows untouched
        ld = n + 5
        Xp = np.zeros((ld, k), dtype=F.dtype, order="F")
        Xp[:n] = X
        Cp = np.full((ld + 3, k), 7.0, dtype=F.dtype, order="F")
        hs._lib.check(fn(F._h, t, Cp.ctypes.data_as(pf), ld + 3, Xp.ctypes.data_as(pf), ld, n, k))
        assert np.array_equal(Cp[:n], ref) and np.all(Cp[n:] == 7.0)
        hs._lib.check(fn(F._h, t, Xp.ctypes.data_as(pf), ld, Xp.ctypes.data_as(pf), ld, n, k))
        assert np.array_equal(Xp[:n], ref) and np.all(Xp[n:] == 0)
        Xr = X.copy(order="F")
        assert hs.mul(Xr, Ft, Xr) is Xr and np.array_equal(Xr, ref)
        # a device tensor, out of place and in place
        dX = torch.from_numpy(np.asfortranarray(X).T.copy()).to("cuda:0").T  # n x k, column-major
        dY = hs.mul(Ft, dX)
        torch.cuda.synchronize()
        assert np.array_equal(dY.cpu().numpy(), ref) and np.array_equal(dX.cpu().numpy(), X)
        assert hs.mul(dX, Ft, dX) is dX
        torch.cuda.synchronize()
        assert np.array_equal(dX.cpu().numpy(), ref)
        dx = torch.from_numpy(X[:, 3].copy()).to("cuda:0")
        assert np.array_equal(hs.mul(Ft, dx).cpu().numpy(), ref[:, 3])
        assert hs.mul(Ft, np.zeros((n, 0), dtype=F.dtype)).shape == (n, 0)
    info = hs.mul_info(F)
    esz = 16 if cplx else 8
    sum_fac = sum(float(F.node_info(i)[0]) ** 2 + 2.0 * F.node_info(i)[0] * F.node_info(i)[1] for i in range(F.nnodes))
    assert info["chunks"] >= 1 and info["factor_bytes"] == info["chunks"] * sum_fac * esz
    assert 0 < info["flops_useful"] <= info["flops_executed"] and info["workspace_bytes"] > 0


@pytest.mark.parametrize("label", ["3d-complex", COMPRESSED])
def test_interleaving_leaves_the_solves_and_their_figures_alone(hs, label):
    P, F = _handle(hs, label)
    n = P["A"].shape[0]
    B, b = _rand(n, 40, True, 71), _rand(n, 2, True, 72)
    Ft = hs.transpose(F)
    first = (hs.ldiv(F, b), hs.ldiv(Ft, b), hs.ldiv_block(F, B), hs.ldiv_block_t(hs.adjoint(F), B))
    before = hs.ldiv_block_info(F)
    assert before["seconds"] > 0
    m1 = hs.mul(F, B)
    m2 = hs.mul(hs.adjoint(F), B[:, :3])
    assert hs.ldiv_block_info(F) == before  # a product is not the handle's last block solve
    assert hs.mul_info(F)["chunks"] == 1 and hs.mul_info(F)["seconds"] > 0
    got = (hs.ldiv(F, b), hs.mul(F, B), hs.ldiv(Ft, b), hs.ldiv_block(F, B), hs.mul(hs.adjoint(F), B[:, :3]), hs.ldiv_block_t(hs.adjoint(F), B))
    assert np.array_equal(got[1], m1) and np.array_equal(got[4], m2)
    assert all(np.array_equal(x, y) for x, y in zip(first, (got[0], got[2], got[3], got[5])))


# ---- 6. hs.factor_error --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(HANDLES))
def test_factor_error_with_given_probes(hs, label):
    """With probes = W the figure is norm(op(A) W - hs.mul(op(F), W)) / norm(op(A) W).  On the compressed handle it equals the NumPy
    value to 1e-12 relative: the two differ by the rounding of op(A) W (device SpMM against SciPy), eps |AW| in norm, against a residual of
    1e-4 |AW|, and an uncorrelated perturbation of that size moves a norm by far less than its own relative size 2e-12.  On the exact
    handles the residual IS rounding, so the two values are not comparable digit by digit; there the figure is held below the bound of the
    product itself."""
    P, F = _handle(hs, label)
    A = P["A"]
    n = A.shape[0]
    cplx = F.dtype.kind == "c"
    W = _rand(n, 19, cplx, 81)
    for t in (0, 1, 2):
        Ft, At = _op(hs, F, t), _opmat(A, t)
        AW = At @ W
        want = np.linalg.norm(AW - hs.mul(Ft, W)) / np.linalg.norm(AW)
        got = hs.factor_error(Ft, probes=W)
        full = hs.factor_error(Ft, probes=W, full=True)
        print(f"{label} trans={t}: factor_error {got:.6e}, NumPy on hs.mul {want:.6e}, relative difference {abs(got - want) / want:.1e}")
        assert full["error"] == got and full["norm_r"] / full["norm_aw"] == pytest.approx(got, rel=1e-14) and full["seconds"] > 0
        assert full["norm_aw"] == pytest.approx(np.linalg.norm(AW), rel=1e-12)
        if label in EXACT:
            assert got < min(100 * MIRROR_ERROR[label], TOL)
        else:
            assert abs(got - want) <= 1e-12 * want
    assert hs.factor_error(F) == hs.factor_error(F)  # default probes: no generator state
    dW = __import__("torch").from_numpy(np.asfortranarray(W).T.copy()).to("cuda:0").T
    assert hs.factor_error(F, probes=dW) == hs.factor_error(F, probes=W)  # device probes


def test_factor_error_tracks_the_compression_tolerance(hs):
    """convdiff_helmholtz 30 x 27 compressed at 1e-2, 1e-4, 1e-6: the figure decreases with the tolerance, and with the 32 default probes it
    lies within a factor 2 of the true ||A - F||_F / ||A||_F, F = hs.mul(F, I)."""
    P = prepare(hs, (30, 27), kind="convdiff_helmholtz", nmax=40, rhs="randn")
    A = P["A"]
    n = A.shape[0]
    Ad = A.toarray()
    prev = np.inf
    for tol in (1e-2, 1e-4, 1e-6):
        F = hs.factor(A, P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=tol, rtol=tol)
        try:
            true = np.linalg.norm(Ad - hs.mul(F, np.eye(n, dtype=F.dtype))) / np.linalg.norm(Ad)
            est = hs.factor_error(F)
            print(f"tol {tol:g}: ||A - F||_F / ||A||_F = {true:.3e}, hs.factor_error (k = 32, seed 0) = {est:.3e}, ratio {est / true:.2f}, maxrank {hs.maxrank(F)}")
            assert hs.maxrank(F) > 0
            assert true / 2 <= est <= 2 * true
            assert est < prev
            prev = est
        finally:
            F.free()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def _untouched_after(hs, F, trans, want, n, word):
    L = hs._lib.lib()
    pf = hs._lib.p_f64
    Bm = np.asfortranarray(_rand(n, 3, False, 1))
    Cm = np.full((n, 3), 42.0, order="F")
    assert L.hs_mul_d(F._h, trans, Cm.ctypes.data_as(pf), n, Bm.ctypes.data_as(pf), n, n, 3) == want
    msg = L.hs_last_error().decode()
    assert "hs_mul_*" in msg and word in msg, msg
    out = np.full(4, 42.0)
    assert L.hs_factor_error_d(F._h, trans, None, 0, 4, 0, 0, out.ctypes.data_as(pf)) == want
    assert "hs_factor_error_*" in L.hs_last_error().decode()
    assert np.all(Cm == 42.0) and np.all(out == 42.0)


def test_refusals(hs):
    L = hs._lib.lib()
    E = hs._lib
    P = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, hss_min=1024)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.mul(hs.transpose(F), P["b"])
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.factor_error(F)
    for trans in (0, 1, 2):
        _untouched_after(hs, F, trans, E.HS_ERR_UNSUPPORTED, P["A"].shape[0], "HSS")
    F.free()
    P = prepare(hs, (24, 24, 24), kind="convdiff", nmax=300, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.mul(hs.adjoint(F), P["b"])
    for trans in (0, 1, 2):
        _untouched_after(hs, F, trans, E.HS_ERR_UNSUPPORTED, P["A"].shape[0], "HSS")
    F.free()
    P, F = _handle(hs, "2d-real")
    n = P["A"].shape[0]
    _untouched_after(hs, F, 3, E.HS_ERR_ARGUMENT, n, "trans")
    _untouched_after(hs, F, -1, E.HS_ERR_ARGUMENT, n, "trans")
    G = hs.demote(F)
    Mo = hs.modify(F, np.ones(n), np.ones(n))
    try:
        for obj in (G, Mo):
            with pytest.raises(hs.UnsupportedError):
                hs.mul(obj, P["b"])
            with pytest.raises(hs.UnsupportedError):
                hs.factor_error(obj)
    finally:
        G.free()
        Mo.free()
    with pytest.raises(TypeError, match="MethodError"):
        hs.mul(hs.transpose(F), P["b"] + 1j)
    with pytest.raises(hs.DimensionMismatch):
        hs.mul(hs.transpose(F), P["b"][:-1])
    with pytest.raises(TypeError):
        hs.mul(F)
    pf = hs._lib.p_f64
    Bm = np.asfortranarray(_rand(n, 2, False, 2))
    Cm = np.full((n, 2), 42.0, order="F")
    assert L.hs_mul_d(F._h, 1, Cm.ctypes.data_as(pf), n, Bm.ctypes.data_as(pf), n, n - 1, 2) == E.HS_ERR_DIMENSION
    assert L.hs_mul_d(F._h, 1, Cm.ctypes.data_as(pf), n - 1, Bm.ctypes.data_as(pf), n, n, 2) == E.HS_ERR_DIMENSION
    assert L.hs_mul_d(F._h, 1, None, n, Bm.ctypes.data_as(pf), n, n, 2) == E.HS_ERR_ARGUMENT  # null block
    Bz = np.asfortranarray(_rand(n, 2, True, 3))
    Cz = np.full((n, 2), 42.0, dtype=complex, order="F")
    assert L.hs_mul_z(F._h, 2, Cz.ctypes.data_as(pf), n, Bz.ctypes.data_as(pf), n, n, 2) == E.HS_ERR_ARGUMENT  # eltype of F and B differ
    out = np.full(4, 42.0)
    assert L.hs_factor_error_d(F._h, 0, None, 0, 0, 0, 0, out.ctypes.data_as(pf)) == E.HS_ERR_ARGUMENT  # k < 1
    assert L.hs_factor_error_d(F._h, 0, None, 0, 4, 0, 2, out.ctypes.data_as(pf)) == E.HS_ERR_ARGUMENT  # where
    assert np.all(Cm == 42.0) and np.all(Cz == 42.0) and np.all(out == 42.0)
