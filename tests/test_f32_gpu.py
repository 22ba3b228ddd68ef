"""Float32-stored factors (hs_f32_*, csrc/hs_f32.hip + kernels_f32.hip + kernels_solve_multi_f32.hip) on the MI355X: the two panel products
over a Float32 panel with exact integer data and, bit for bit, against the FP64 products on rounded data; the demoted solve bit for bit
against the FP64 block solve of a handle whose stored factors were rounded in place (hsk_round_factors_f32); the bitwise properties; the
accuracy of one solve; GMRES preconditioned by the demoted copy; the refusals; and a timing guard.

Accuracy bound (test 5): factors perturbed by 2^-24 relatively move the solution by cond_1(A) 2^-24 to first order; the factor 10 is the
slack the modified solves give their first-order bound (tests/test_mod_gpu.py).  cond_1 is hs.condest of the same handle, in the same test.

GMRES cap (test 6): 6 iterations to a residual of 1e-9 on the exact handles.  A condition, not a measurement: SuperLU factors rounded
through Float32 needed 2 iterations on these matrices on the CPU; the library pivots differently, and the cap leaves a factor of 3."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import f32_mirror as FM
from helpers import prepare, relerr

pytestmark = pytest.mark.gpu

EXACT = [("convdiff", (30, 27), 40), ("convdiff_helmholtz", (30, 27), 40), ("convdiff_helmholtz", (24, 24, 24), 300)]
COMPRESSED = ("convdiff_helmholtz", (24, 24, 24), 300)
CKW = dict(swlevel=2, swsize=8, atol=1e-4, rtol=1e-4)
IDS = ["2d-real", "2d-complex", "3d-complex", "3d-complex-tol1e-4"]
ALL = [e + (None,) for e in EXACT] + [COMPRESSED + (CKW,)]
TRANS = ("N", "T", "H")
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for v in _CACHE.values():
        for x in v[1:4]:
            x.free()
    _CACHE.clear()


def _problem(hs, kind, shape, nmax, kw):
    """(P, F, G = demote(F), F2 = a second factorization rounded in place, counts of the rounding, SuperLU), built once per module"""
    key = (kind, shape, nmax, kw is not None)
    if key not in _CACHE:
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        F = hs.factor(P["A"], P["nd"], P["nd_loc"], **(kw or dict(swlevel=0)))
        F2 = hs.factor(P["A"], P["nd"], P["nd_loc"], **(kw or dict(swlevel=0)))
        G = hs.demote(F)
        cnt = np.zeros(2, dtype=np.int64)
        hs._lib.check(hs._lib.lib().hsk_round_factors_f32(F2._h, cnt.ctypes.data_as(hs._lib.p_i64)))
        _CACHE[key] = (P, F, G, F2, cnt, spla.splu(P["A"]))
    return _CACHE[key]


def _rand(n, k, cplx, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    return B + 1j * rng.standard_normal((n, k)) if cplx else B


def _op(hs, F, t):
    return {"N": F, "T": hs.transpose(F), "H": hs.adjoint(F)}[t]


def _opmat(A, t):
    return {"N": A, "T": A.T, "H": A.conj().T, "C": A.conj().T}[t]


# ---- 1, 2. the kernels alone ------------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 16, 16), (70, 37, 5), (257, 256, 33), (33, 300, 64), (70, 37, 17)]  # the last: trap and a map at ragged M, K with a ragged second column tile


def _call(hs, name, cplx, M, K, kc, A, X, C0, minus, trap, conj, cmap):
    """one panel product through a hook: name = hsk_multi_prob[_t][_f32]; A is M x K (forward) or K x M (transposed)"""
    L = hs._lib.lib()
    fn = getattr(L, name + ("_z" if cplx else "_d"))
    p = hs._lib.p_f64
    A, X = np.asfortranarray(A), np.asfortranarray(X)
    Cm = np.array(C0, order="F")
    m = None if cmap is None else cmap.ctypes.data_as(C.POINTER(C.c_int32))
    args = [M, K, kc, A.ctypes.data_as(p), A.shape[0], X.ctypes.data_as(p), X.shape[0], Cm.ctypes.data_as(p), Cm.shape[0], minus, trap]
    if "prob_t" in name:
        args.append(conj)
    hs._lib.check(fn(*args, m))
    return Cm


def _trapezoid(A):
    T = np.tril(A, -1)
    d = np.arange(min(A.shape))
    T[d, d] = 1
    return T


def _cases(cplx):
    for M, K, kc in SHAPES:
        for minus in (0, 1):
            for trap in (0, 1):
                for use_map in (False, True):
                    for conj in ((0, 1) if cplx else (0,)):
                        yield M, K, kc, minus, trap, use_map, conj


def _data(rng, M, K, kc, cplx, integers, transposed):
    def draw(shape):
        if integers:
            v = rng.integers(-3, 4, size=shape).astype(np.float64)
            return v + 1j * rng.integers(-3, 4, size=shape) if cplx else v
        v = rng.standard_normal(shape)
        return v + 1j * rng.standard_normal(shape) if cplx else v

    ld = (K if transposed else M) + 3  # odd and even leading dimensions of the Float64 source both occur over the shapes
    A = draw((ld, M if transposed else K))
    X = draw((K + 2, kc))
    if integers:
        X[:K] += (np.arange(K)[:, None] * 2 - np.arange(kc)[None, :]) % 5  # asymmetric: a swapped row / column map cannot pass
    C0 = draw((M + 1, kc))
    return A, X, C0


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_panel_products_are_exact_on_integer_data(hs, cplx):
    """Integers in -3..3 are Float32 numbers and every product and sum is exact in Float64: equality with the integer product."""
    rng = np.random.default_rng(23)
    for M, K, kc, minus, trap, use_map, conj in _cases(cplx):
        # forward: D = C - A X, A M x K, cmap sends row i of the product to row map[i] of C
        A, X, C0 = _data(rng, M, K, kc, cplx, True, False)
        cmap = rng.permutation(M).astype(np.int32) if use_map else None
        got = _call(hs, "hsk_multi_prob_f32", cplx, M, K, kc, A, X, C0, minus, trap, 0, cmap)
        Aop = _trapezoid(A[:M]) if trap else A[:M]
        prod = Aop @ X[:K]
        want = C0.copy()
        rows = np.arange(M) if cmap is None else cmap
        want[rows] = (C0[rows] - prod) if minus else prod
        assert np.array_equal(got, want), ("fwd", M, K, kc, minus, trap, use_map)
        # transposed: D = C - op(A)^T X, A K x M, xmap pairs row k of A with row map[k] of X
        A, X, C0 = _data(rng, M, K, kc, cplx, True, True)
        xmap = rng.permutation(K).astype(np.int32) if use_map else None
        got = _call(hs, "hsk_multi_prob_t_f32", cplx, M, K, kc, A, X, C0, minus, trap, conj, xmap)
        Aop = _trapezoid(A[:K]) if trap else A[:K]
        Aop = (np.conj(Aop) if conj else Aop).T
        prod = Aop @ (X[:K] if xmap is None else X[:K][xmap])
        want = C0.copy()
        want[:M] = (C0[:M] - prod) if minus else prod
        assert np.array_equal(got, want), ("tr", M, K, kc, minus, trap, use_map, conj)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_panel_products_have_the_bits_of_the_fp64_products_on_rounded_data(hs, cplx):
    """Random Float64 A: the Float32 product returns, bit for bit, what the FP64 product returns for A rounded through Float32 (real and
    imaginary parts separately) -- the same summation order, and a widening that is exact."""
    rng = np.random.default_rng(29)
    for M, K, kc, minus, trap, use_map, conj in _cases(cplx):
        A, X, C0 = _data(rng, M, K, kc, cplx, False, False)
        cmap = rng.permutation(M).astype(np.int32) if use_map else None
        got = _call(hs, "hsk_multi_prob_f32", cplx, M, K, kc, A, X, C0, minus, trap, 0, cmap)
        ref = _call(hs, "hsk_multi_prob", cplx, M, K, kc, FM.rounded(A), X, C0, minus, trap, 0, cmap)
        assert np.array_equal(got, ref), ("fwd", M, K, kc, minus, trap, use_map)
        if not trap:
            assert not np.array_equal(got, _call(hs, "hsk_multi_prob", cplx, M, K, kc, A, X, C0, minus, trap, 0, cmap))  # the rounding is there
        A, X, C0 = _data(rng, M, K, kc, cplx, False, True)
        xmap = rng.permutation(K).astype(np.int32) if use_map else None
        got = _call(hs, "hsk_multi_prob_t_f32", cplx, M, K, kc, A, X, C0, minus, trap, conj, xmap)
        ref = _call(hs, "hsk_multi_prob_t", cplx, M, K, kc, FM.rounded(A), X, C0, minus, trap, conj, xmap)
        assert np.array_equal(got, ref), ("tr", M, K, kc, minus, trap, use_map, conj)


# ---- 3. the handle, bit for bit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax,kw", ALL, ids=IDS)
def test_demoted_solve_has_the_bits_of_the_fp64_solve_on_rounded_factors(hs, kind, shape, nmax, kw):
    P, F, G, F2, cnt, _ = _problem(hs, kind, shape, nmax, kw)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    info = G.info()
    print(f"{kind} {shape}: {info['value_bytes']} Float32 value bytes, {info['index_bytes']} index bytes, flushed {info['flushed']}, rounding hook counts {cnt.tolist()}")
    assert cnt[0] == 0 and cnt[1] == info["flushed"]
    for t in TRANS:
        for k in (1, 17, 33, 70):
            B = _rand(n, k, cplx, 100 + k)
            X = hs.ldiv_f32(G, B, trans=t)
            R = hs.ldiv_block_t(_op(hs, F2, t), B)
            assert np.array_equal(X, R), (t, k, relerr(X, R))
    # the unrounded handle gives other bits: the comparison above is not vacuous
    B = _rand(n, 3, cplx, 7)
    assert not np.array_equal(hs.ldiv_f32(G, B), hs.ldiv_block_t(F, B))


# ---- 4. properties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax,kw", ALL, ids=IDS)
def test_determinism_column_independence_and_the_byte_counts(hs, kind, shape, nmax, kw):
    P, F, G, _, _, _ = _problem(hs, kind, shape, nmax, kw)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    B = _rand(n, 40, cplx, 3)
    for t in TRANS:
        X = hs.ldiv_f32(G, B, trans=t)
        assert np.array_equal(X, hs.ldiv_f32(G, B, trans=t))
        assert np.array_equal(X[:, 35], hs.ldiv_f32(G, B[:, 35], trans=t))  # alone
        Bs = _rand(n, 9, cplx, 4)
        Bs[:, 2] = B[:, 35]
        assert np.array_equal(X[:, 35], hs.ldiv_f32(G, Bs, trans=t)[:, 2])  # at another position of another block
        Cout = np.empty_like(B, order="F")
        assert hs.ldiv_f32(Cout, G, B, trans=t) is Cout and np.array_equal(Cout, X)
    out = np.zeros(8)
    hs._lib.check(hs._lib.lib().hs_f32_info(G._h, out.ctypes.data_as(hs._lib.p_f64)))
    assert out[2] == 2 * out[1] and out[1] > 0 and G.nbytes == out[1] + out[3] and out[6] >= 1 and out[4] > 0 and out[0] > 0 and out[7] > 0
    st = F.stats()
    print(f"{kind} {shape}: Float32 values {out[1]:.0f} B, padding + indices {out[3]:.0f} B, hs_get_stats.bytes_factors {st['bytes_factors']:.0f} B, demotion {out[7] * 1e3:.1f} ms")


@pytest.mark.parametrize("kind,shape,nmax", EXACT[:2], ids=IDS[:2])
def test_the_copy_outlives_the_handle(hs, kind, shape, nmax):
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
    n = P["A"].shape[0]
    B = _rand(n, 33, F.dtype.kind == "c", 9)
    with hs.demote(F) as G:
        X = {t: hs.ldiv_f32(G, B, trans=t) for t in TRANS}
        F.free()
        hs.trim()
        F3 = hs.factor(P["A"] * 3.0, P["nd"], P["nd_loc"], swlevel=0)  # the freed blocks are taken again and overwritten
        for t in TRANS:
            assert np.array_equal(hs.ldiv_f32(G, B, trans=t), X[t]), t
        F3.free()
    assert G._h is None


# ---- 5. accuracy of one solve -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,nmax", EXACT, ids=IDS[:3])
def test_one_solve_is_accurate_to_the_rounding_of_the_factors(hs, kind, shape, nmax):
    P, F, G, _, _, lu = _problem(hs, kind, shape, nmax, None)
    A = P["A"]
    n = A.shape[0]
    B = _rand(n, 5, F.dtype.kind == "c", 61)
    for t in TRANS:
        cond = hs.condest(_op(hs, F, t))
        R = lu.solve(B, trans=t)
        X32, X64 = hs.ldiv_f32(G, B, trans=t), hs.ldiv_block_t(_op(hs, F, t), B)
        Aop = _opmat(A, t)
        for j in range(B.shape[1]):
            e32, e64 = relerr(X32[:, j], R[:, j]), relerr(X64[:, j], R[:, j])
            r32 = np.linalg.norm(B[:, j] - Aop @ X32[:, j]) / np.linalg.norm(B[:, j])
            r64 = np.linalg.norm(B[:, j] - Aop @ X64[:, j]) / np.linalg.norm(B[:, j])
            print(f"{kind} {shape} trans={t} col {j}: error f32 {e32:.2e} / f64 {e64:.2e}, residual f32 {r32:.2e} / f64 {r64:.2e}, bound {10 * cond * 2.0**-24:.2e} (cond_1 {cond:.2e})")
            assert e32 <= 10.0 * cond * 2.0**-24, (t, j)
            assert e32 >= e64, (t, j)


# ---- 6. GMRES -------------------------------------------------------------------------------------------------------------------------------------
def _true_residuals(A, X, B, t):
    Aop = _opmat(A, t)
    return [float(np.linalg.norm(B[:, j] - Aop @ X[:, j]) / np.linalg.norm(B[:, j])) for j in range(B.shape[1])]


@pytest.mark.parametrize("kind,shape,nmax", EXACT, ids=IDS[:3])
def test_gmres_preconditioned_by_the_copy_reaches_full_accuracy(hs, kind, shape, nmax):
    P, F, G, _, _, _ = _problem(hs, kind, shape, nmax, None)
    A = P["A"]
    B = _rand(A.shape[0], 5, F.dtype.kind == "c", 71)
    for t in ("N", "C"):
        X, ch = hs.gmres_block(A, B, Pr=G, trans=t, reltol=1e-9, restart=30, maxiter=6, log=True)
        _, chF = hs.gmres_block(A, B, Pr=F, trans=t, reltol=1e-9, restart=30, maxiter=6, log=True)
        res = _true_residuals(A, X, B, t)
        print(f"{kind} {shape} trans={t}: iterations Pr=G {[c['iters'] for c in ch]}, Pr=F {[c['iters'] for c in chF]}, true residuals {['%.1e' % r for r in res]}")
        assert all(c["isconverged"] for c in ch)
        assert max(res) <= 1e-8


def test_gmres_on_the_compressed_handle_costs_at_most_one_iteration(hs):
    P, F, G, _, _, _ = _problem(hs, *COMPRESSED, CKW)
    A = P["A"]
    B = _rand(A.shape[0], 5, True, 73)
    for t in ("N", "C"):
        X, ch = hs.gmres_block(A, B, Pr=G, trans=t, reltol=1e-9, restart=30, maxiter=60, log=True)
        _, chF = hs.gmres_block(A, B, Pr=F, trans=t, reltol=1e-9, restart=30, maxiter=60, log=True)
        res = _true_residuals(A, X, B, t)
        print(f"tol 1e-4 trans={t}: iterations Pr=G {[c['iters'] for c in ch]}, Pr=F {[c['iters'] for c in chF]}, true residuals {['%.1e' % r for r in res]}")
        assert all(c["isconverged"] for c in ch) and max(res) <= 1e-8
        for c, cF in zip(ch, chF):
            assert c["iters"] <= cF["iters"] + 1


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------
def _untouched_after(hs, G, trans, want, n, dtype, nrows=None, ldc=None, null=False):
    L = hs._lib.lib()
    cplx = np.dtype(dtype).kind == "c"
    fn = L.hs_f32_ldiv_z if cplx else L.hs_f32_ldiv_d
    p = hs._lib.p_f64
    Bm = np.asfortranarray(_rand(n, 3, cplx, 1).astype(dtype))
    Cm = np.full((n, 3), 42.0, dtype=dtype, order="F")
    assert fn(G._h, trans, Cm.ctypes.data_as(p), n if ldc is None else ldc, None if null else Bm.ctypes.data_as(p), n, n if nrows is None else nrows, 3) == want
    assert np.all(Cm == 42.0)


def test_refusals(hs):
    E = hs._lib
    P = prepare(hs, (30, 27), kind="convdiff", nmax=40, rhs="randn")
    F = hs.factor(P["A"] * 1e39, P["nd"], P["nd_loc"], swlevel=0)
    with pytest.raises(hs.UnsupportedError, match=r"[1-9][0-9]* stored factor entries .* overflow Float32") as ei:
        hs.demote(F)
    assert ei.value.info > 0 and str(ei.value.info) in str(ei.value)
    F.free()
    P3 = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512, rhs="randn")
    F = hs.factor(P3["A"], P3["nd"], P3["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, hss_min=1024)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.demote(F)
    F.free()
    P3 = prepare(hs, (24, 24, 24), kind="convdiff", nmax=300, rhs="randn")
    F = hs.factor(P3["A"], P3["nd"], P3["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.demote(F)
    F.free()
    _, F, G, _, _, _ = _problem(hs, *EXACT[0], None)
    n = F.n
    _untouched_after(hs, G, 3, E.HS_ERR_ARGUMENT, n, np.float64)
    _untouched_after(hs, G, -1, E.HS_ERR_ARGUMENT, n, np.float64)
    _untouched_after(hs, G, 1, E.HS_ERR_DIMENSION, n, np.float64, nrows=n - 1)
    _untouched_after(hs, G, 1, E.HS_ERR_DIMENSION, n, np.float64, ldc=n - 1)
    _untouched_after(hs, G, 0, E.HS_ERR_ARGUMENT, n, np.float64, null=True)
    _untouched_after(hs, G, 2, E.HS_ERR_ARGUMENT, n, np.complex128)  # eltype of G and B differ
    # GMRES: the size and the element type of A and B against the object's
    A = P["A"]
    X0 = np.full((n, 2), 42.0)
    import scipy.sparse as sp

    with pytest.raises(hs.DimensionMismatch, match="preconditioner"):
        hs.gmres_block(sp.eye(n + 1, format="csc"), np.ones((n + 1, 2)), Pr=G)
    with pytest.raises(hs.DimensionMismatch, match="ComplexF64"):
        hs.gmres_block(A, _rand(n, 2, True, 5), Pr=G)
    with pytest.raises(ValueError, match="holds no matrix"):
        hs.gmres_block(None, X0, Pr=G)
    L = E.lib()
    colptr, rowval = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1, np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    nz = np.ascontiguousarray(A.data, dtype=np.float64)
    Bm = np.asfortranarray(_rand(n, 2, False, 6))
    Xm = np.full((n, 2), 42.0, order="F")
    it, cv = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tail = (vp(Bm), n, vp(Xm), n, 2, 0, 0, 1e-9, 0.0, 30, 6, None, it.ctypes.data_as(E.p_i64), cv.ctypes.data_as(C.POINTER(C.c_int)), None)
    assert L.hs_gmres_block_f32_d(G._h, 0, n, None, None, None, *tail) == E.HS_ERR_ARGUMENT and "holds no matrix" in L.hs_last_error().decode()
    assert L.hs_gmres_block_f32_d(G._h, 3, n, colptr.ctypes.data_as(E.p_i64), rowval.ctypes.data_as(E.p_i64), vp(nz), *tail) == E.HS_ERR_ARGUMENT
    assert L.hs_gmres_block_f32_z(G._h, 0, n, colptr.ctypes.data_as(E.p_i64), rowval.ctypes.data_as(E.p_i64), vp(nz), *tail) == E.HS_ERR_DIMENSION
    assert np.all(Xm == 42.0) and np.all(X0 == 42.0)


# ---- 8. guard ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_demoted_solve_is_not_grossly_slower(hs):
    """A cap against a gross regression, not the result: the same launches and the same MFMAs run in both solves, so a factor of 2 can only
    come from a defect such as spills.  Poisson 40^3 exact, 32 columns, device arrays, device seconds of the library's own event pairs, the
    two solves alternating, median of 5 after a warm-up."""
    import torch

    P = prepare(hs, (40, 40, 40), kind="poisson", rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
    G = hs.demote(F)
    L = hs._lib.lib()
    n, k = P["A"].shape[0], 32
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev)
    sp_ = C.c_void_p(s.cuda_stream)
    dB = torch.from_numpy(np.asfortranarray(_rand(n, k, False, 51)).T.copy()).to(dev)
    dX, dY = torch.empty_like(dB), torch.empty_like(dB)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    t32, t64 = [], []
    for it in range(6):
        hs._lib.check(L.hs_f32_ldiv_dev_d(G._h, 0, p(dX), n, p(dB), n, n, k, sp_))
        a = G.info()["solve_seconds"]
        hs._lib.check(L.hs_ldiv_block_dev_t_d(F._h, 0, p(dY), n, p(dB), n, n, k, sp_))
        b = hs.ldiv_block_info(F)["seconds"]
        if it > 0:
            t32.append(a)
            t64.append(b)
    a, b = float(np.median(t32)), float(np.median(t64))
    e = relerr(dX.cpu().numpy(), dY.cpu().numpy())
    print(f"Poisson 40^3, nrhs = 32: ldiv_f32 {a * 1e3:.3f} ms, ldiv_block_t {b * 1e3:.3f} ms, ratio {a / b:.2f}; difference of the solutions {e:.2e}")
    assert 0 < e < 1e-3
    assert a <= 2 * b
    G.free()
    F.free()
