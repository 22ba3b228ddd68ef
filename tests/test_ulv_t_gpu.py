"""Transposed and adjoint ULV solves of the HSS module on the device (hs_hss_ldiv_t, csrc/kernels_ulv_t.hip).

The grouped kernel alone runs on small integers, where every product and sum is exact in Float64, so its operand maps are checked with
exact equality.  The solves H^-T B and H^-H B are checked against dense solves with the expanded matrix, at the bound the forward solve
holds on the same matrices (tests/test_hss_gpu.py), and the forward solve is asserted next to them so that a failure isolates the
transposed path."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-9  # relative, against a dense solve with H.expand(): the bound of the forward solve in tests/test_hss_gpu.py


def kernel_matrix(n, complex_=False, seed=0):
    """Non-symmetric, diagonally dominant matrix with smooth off-diagonal blocks (1-D points); as in tests/test_hss_oracle.py."""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.random(n))
    d = np.abs(x[:, None] - x[None, :])
    A = 1.0 / (1.0 + 40.0 * d) + 0.3 * np.sin(3.0 * x)[:, None] * np.cos(2.0 * x)[None, :]
    if complex_:
        A = A * np.exp(1j * 2.0 * d)
    return A + n * 0.05 * np.eye(n)


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------------

# (M, K, N, tri): the ragged edges of the 16-wide MFMA tiles and of the K chunking (8 k per step for Float64, 4 for ComplexF64),
# more than one workgroup in M (70 > 64), one to three column tiles per wave, an empty job in every launch
GROUPS = [
    [(1, 1, 1, 0), (15, 16, 3, 0), (0, 17, 16, 0), (17, 33, 17, 0), (70, 15, 35, 0), (33, 70, 16, 0)],
    [(16, 17, 35, 0), (33, 0, 3, 0), (70, 70, 1, 0), (15, 1, 17, 0), (1, 33, 16, 0)],
    [(33, 33, 3, 1), (17, 17, 35, 2), (16, 16, 16, 1), (15, 15, 0, 2), (1, 1, 17, 2), (70, 70, 17, 1)],
]


def int_block(rng, rows, cols, cplx):
    a = rng.integers(-4, 5, size=(rows, cols)).astype(np.float64)
    if cplx:
        a = a + 1j * rng.integers(-4, 5, size=(rows, cols))
    return a


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("conj", [0, 1])
@pytest.mark.parametrize("minus", [0, 1])
@pytest.mark.parametrize("group", range(len(GROUPS)))
def test_grouped_kernel_exact_integers(hs, group, minus, conj, cplx):
    L = hs._lib.lib()
    fn = L.hsk_ulv_t_group_z if cplx else L.hsk_ulv_t_group_d
    dt = np.complex128 if cplx else np.float64
    rng = np.random.default_rng(100 * group + 10 * minus + conj)
    jobs, desc = [], []
    Ab, Xb, Cb = [], [], []
    na = nx = nc = 0
    for (M, K, N, tri) in GROUPS[group]:
        lda, ldx, ldc = K + 3, K + 1, M + 2
        A = int_block(rng, lda, max(M, 1), cplx)
        X = int_block(rng, ldx, max(N, 1), cplx)
        C0 = int_block(rng, ldc, max(N, 1), cplx)
        desc += [M, K, N, lda, ldx, ldc, na, nx, nc, minus | (tri << 1)]
        jobs.append((M, K, N, tri, A, X, C0, nc, ldc))
        Ab.append(A.ravel(order="F")); Xb.append(X.ravel(order="F")); Cb.append(C0.ravel(order="F"))
        na += A.size; nx += X.size; nc += C0.size
    Abuf = np.ascontiguousarray(np.concatenate(Ab), dtype=dt)
    Xbuf = np.ascontiguousarray(np.concatenate(Xb), dtype=dt)
    Cbuf = np.ascontiguousarray(np.concatenate(Cb), dtype=dt)
    before = Cbuf.copy()
    d = (C.c_int64 * len(desc))(*desc)
    p = lambda a: a.ctypes.data_as(hs._lib.p_f64)
    hs._lib.check(fn(len(jobs), d, p(Abuf), na, p(Xbuf), nx, p(Cbuf), nc, conj))
    expect = before.copy()
    for (M, K, N, tri, A, X, C0, off, ldc) in jobs:
        if M == 0 or K == 0 or N == 0:
            continue  # skipped: C as it was
        Ak = A[:K, :M]
        if tri == 1:
            Ak = np.tril(Ak)
        elif tri == 2:
            Ak = np.triu(Ak)
        opA = Ak.conj() if (conj and cplx) else Ak
        P = opA.T @ X[:K, :N]
        R = C0.copy()
        R[:M, :N] = C0[:M, :N] - P if minus else P
        expect[off:off + R.size] = R.ravel(order="F")
    # everything outside the M x N blocks (padding rows, skipped jobs) must be untouched as well
    assert np.array_equal(Cbuf, expect)


def test_grouped_kernel_hook_refuses_bad_jobs(hs):
    L = hs._lib.lib()
    a = np.zeros(4)
    p = lambda v: v.ctypes.data_as(hs._lib.p_f64)
    d = (C.c_int64 * 10)(2, 2, 2, 2, 2, 2, 0, 0, 1, 0)  # C block: offset 1 + 4 entries > 4
    assert L.hsk_ulv_t_group_d(1, d, p(a), 4, p(a), 4, p(a), 4, 0) == hs._lib.HS_ERR_ARGUMENT


# ---- the HSS module ------------------------------------------------------------------------------------------------------------------------

def dense_of(H, perm=None):
    E = H.expand()
    if perm is None:
        return E
    F = np.zeros_like(E)
    F[np.ix_(perm, perm)] = E  # expand() is in the tree's order A[perm][:, perm]
    return F


def rhs(n, q, complex_, seed=7):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, q))
    return X + 1j * rng.standard_normal((n, q)) if complex_ else X


def relerr(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def check_solves(H, complex_, perm=None, cols=(1, 3, 35)):
    n = H.shape[0]
    E = dense_of(H, perm)
    for q in cols:
        X = rhs(n, q, complex_, seed=q)
        fwd = H.ldiv(X)
        e0 = relerr(fwd, np.linalg.solve(E, X))
        et = relerr(H.ldiv(X, trans="T"), np.linalg.solve(E.T, X))
        ec = relerr(H.ldiv(X, trans="C"), np.linalg.solve(E.conj().T, X))
        print(f"n={n} q={q} complex={complex_}: forward {e0:.2e}  transposed {et:.2e}  adjoint {ec:.2e}")
        assert e0 < TOL, e0
        assert et < TOL, et
        assert ec < TOL, ec
        assert np.array_equal(H.ldiv(X, trans="N"), fwd)
    # a vector
    x = rhs(n, 1, complex_, seed=99)[:, 0]
    y = H.ldiv(x, trans="T")
    assert y.shape == (n,) and relerr(y, np.linalg.solve(E.T, x)) < TOL
    # two calls: equal bits; a real matrix: "C" is "T"
    X = rhs(n, 3, complex_, seed=5)
    for t in ("T", "C"):
        assert np.array_equal(H.ldiv(X, trans=t), H.ldiv(X, trans=t))
    if not complex_:
        assert np.array_equal(H.ldiv(X, trans="C"), H.ldiv(X, trans="T"))
    else:
        assert not np.array_equal(H.ldiv(X, trans="C"), H.ldiv(X, trans="T"))


@pytest.mark.parametrize("complex_", [False, True])
@pytest.mark.parametrize("n,leaf,tol", [(500, 40, 1e-4), (1200, 64, 1e-8), (70, 16, 1e-6)])
def test_hss_ldiv_t_against_dense(hs, complex_, n, leaf, tol):
    A = kernel_matrix(n, complex_)
    H = hs.hss.compress(A, leafsize=leaf, atol=tol, rtol=tol, kest=32)
    assert H.num_nodes >= 3
    check_solves(H, complex_)


@pytest.mark.parametrize("complex_", [False, True])
def test_hss_ldiv_t_single_leaf(hs, complex_):
    H = hs.hss.compress(kernel_matrix(48, complex_), leafsize=64)
    assert H.num_nodes == 1
    check_solves(H, complex_)


@pytest.mark.parametrize("complex_", [False, True])
def test_hss_ldiv_t_uneven_first_split(hs, complex_):
    A = kernel_matrix(300, complex_)
    H = hs.hss.compress(A, hs.hss.bisection_cluster((100, 300), leafsize=50), atol=1e-8, rtol=1e-8)
    check_solves(H, complex_, cols=(3,))


@pytest.mark.parametrize("complex_", [False, True])
def test_hss_ldiv_t_permuted(hs, complex_):
    n = 400
    perm = np.random.default_rng(11).permutation(n)
    A = np.zeros((n, n), dtype=np.complex128 if complex_ else np.float64)
    A[np.ix_(perm, perm)] = kernel_matrix(n, complex_)  # A[perm][:, perm] is the smooth matrix
    H = hs.hss.compress(A, leafsize=40, atol=1e-8, rtol=1e-8, kest=32, perm=perm)
    assert relerr(dense_of(H, perm), A) < 1e-6
    check_solves(H, complex_, perm=perm, cols=(3,))


@pytest.mark.parametrize("complex_", [False, True])
@pytest.mark.parametrize("kind", ["random", "mixed"])
def test_hss_ldiv_full_rank_nodes(hs, kind, complex_):
    """Non-root nodes that keep full rank (r == m) eliminate nothing: the walk only moves their rows, in all three directions.
    "random": a dense random matrix, every non-root node is such a node.  "mixed": a smooth matrix with one dense random block row and
    column at 1e-13, where the 12-point leaves keep full rank and nodes above them compress, so both kinds share the launches of a level."""
    n = 96
    rng = np.random.default_rng(3)
    R = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if complex_ else 0)
    if kind == "random":
        A = R + n * np.eye(n)
    else:
        A = kernel_matrix(n, complex_)
        A[:12, :] += 0.1 * R[:12, :]
        A[:, :12] += 0.1 * R[:, :12]
    H = hs.hss.compress(A, leafsize=16, atol=1e-13, rtol=1e-13, kest=32)
    info = [H._info(i) for i in range(1, H.num_nodes)]
    print(f"{kind} complex={complex_}: (m, r) of the non-root nodes {[(d['m'], d['r']) for d in info]}")
    assert H.num_nodes >= 7 and any(d["r"] == d["m"] for d in info)
    if kind == "random":
        assert all(d["r"] == d["m"] for d in info)
    else:
        assert any(d["r"] < d["m"] for d in info)
    check_solves(H, complex_)


@pytest.mark.parametrize("complex_", [False, True])
def test_hss_ldiv_t_device_pointer_and_arguments(hs, complex_):
    """where = 1 agrees bitwise with where = 0; trans outside 0..2 is refused with B untouched."""
    import torch

    n, q = 500, 5
    L = hs._lib.lib()
    H = hs.hss.compress(kernel_matrix(n, complex_), leafsize=40, atol=1e-8, rtol=1e-8, kest=32)
    X = rhs(n, q, complex_)
    for t, name in ((1, "T"), (2, "C"), (0, "N")):
        host = H.ldiv(X, trans=name)
        dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()  # column-major bytes of X
        hs._lib.check(L.hs_hss_ldiv_t(H._h, t, C.c_void_p(dX.data_ptr()), n, q, 1))
        assert np.array_equal(dX.cpu().numpy().T, host)
    B = np.asfortranarray(X.copy())
    for bad in (3, -1):
        assert L.hs_hss_ldiv_t(H._h, bad, B.ctypes.data_as(C.c_void_p), n, q, 0) == hs._lib.HS_ERR_ARGUMENT
        assert np.array_equal(B, X)
    assert L.hs_hss_ldiv_t(H._h, 1, None, n, q, 0) == hs._lib.HS_ERR_ARGUMENT
    assert L.hs_hss_ldiv_t(H._h, 1, B.ctypes.data_as(C.c_void_p), n, 0, 0) == 0
    with pytest.raises(ValueError):
        H.ldiv(X, trans="X")


# ---- solver handles: hs_ldiv_ulv_* ---------------------------------------------------------------------------------------------------------
import scipy.sparse.linalg as spla  # noqa: E402

from helpers import prepare  # noqa: E402

NCOL = 35  # one full chunk of 32 columns and a ragged one
# Defect of the adjoint identity  Y^op B = W^op X  (X = F^-1 B by hs.ldiv, Y = op(F)^-1 W by the block solve), relative to |W|_F |X|_F,
# measured with the EXISTING hs.ldiv_block_t on the "mf-dense-D" configuration of tests/test_ldiv_block_t_gpu.py (convdiff_helmholtz 24^3,
# mf=True): 2.71e-17 (transpose) and 3.13e-17 (adjoint) -- DESIGN.md, "Transposed and adjoint ULV solves".  The bound is 10 times the larger one.
ADJOINT_BASELINE = 3.13e-17
ADJOINT_BOUND = 10 * ADJOINT_BASELINE

# the option sets tests/test_ldiv_block_t_gpu.py::test_refusals (and the refusal tests of the other solves) prove to contain HSS fronts
HANDLES = {
    "hss_d": ("convdiff", (32, 32, 32), 512, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, hss_min=1024)),
    "mf2": ("convdiff", (24, 24, 24), 300, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)),
    "mf3": ("convdiff", (24, 24, 24), 300, dict(swlevel=3, swsize=8, atol=1e-6, rtol=1e-6, mf=3, leafsize=128)),
    "mf2-complex": ("convdiff_helmholtz", (24, 24, 24), 300, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)),
}
_H = {}


@pytest.fixture(scope="module", autouse=True)
def _free_handles():
    yield
    for P, F, lu, x0 in _H.values():
        F.free()
    _H.clear()


def handle(hs, label):
    """(problem, factorization, SuperLU factors, hs.ldiv(F, b) taken before anything else ran on the handle)"""
    if label not in _H:
        kind, shape, nmax, kw = HANDLES[label]
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        F = hs.factor(P["A"], P["nd"], P["nd_loc"], **kw)
        flow = (C.c_int64 * 8)()
        hs._lib.check(hs._lib.lib().hs_flow_info(F._h, flow))
        if label == "hss_d":
            assert flow[4] > 0, list(flow)  # fronts with an HSS D
        else:
            assert flow[0] in (2, 3) and flow[1] > 0, list(flow)  # matrix-free fronts, their D one HSS matrix / the 2 x 2 block form
        b = P["b"].astype(F.dtype)
        _H[label] = (P, F, spla.splu(P["A"].tocsc()), hs.ldiv(F, b))
    return _H[label]


def _block(n, k, cplx, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    return B + 1j * rng.standard_normal((n, k)) if cplx else B


def _op(hs, F, trans):
    return F if trans == 0 else (hs.adjoint(F) if trans == 2 else hs.transpose(F))


def _worst_col(X, R):
    return max(relerr(X[:, j], R[:, j]) for j in range(X.shape[1]))


@pytest.mark.parametrize("label", list(HANDLES))
def test_handle_forward_block_against_looped(hs, label):
    P, F, lu, x0 = handle(hs, label)
    n = P["A"].shape[0]
    B = _block(n, NCOL, F.dtype.kind == "c", 3)
    X = hs.ldiv_ulv(F, B)
    Xl = hs.ldiv(F, B)
    e = _worst_col(X, Xl)
    print(f"{label}: hs.ldiv_ulv(F, B) against the looped hs.ldiv, worst column {e:.2e}")
    assert X.shape == B.shape and e < 1e-10
    assert np.array_equal(X, hs.ldiv_ulv(F, B))
    b = B[:, 0].copy()
    assert hs.ldiv_ulv(F, b).shape == (n,) and np.array_equal(hs.ldiv_ulv(F, b), X[:, 0])


@pytest.mark.parametrize("trans", [1, 2])
@pytest.mark.parametrize("label", list(HANDLES))
def test_handle_adjoint_identity(hs, label, trans):
    P, F, lu, x0 = handle(hs, label)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    B, W = _block(n, NCOL, cplx, 11), _block(n, NCOL, cplx, 12)
    X = hs.ldiv(F, B)
    Y = hs.ldiv_ulv(_op(hs, F, trans), W)
    t = (lambda M: M.conj().T) if trans == 2 else (lambda M: M.T)
    d = np.linalg.norm(t(Y) @ B - t(W) @ X) / (np.linalg.norm(W) * np.linalg.norm(X))
    print(f"{label} trans={trans}: defect of the adjoint identity {d:.2e} (bound {ADJOINT_BOUND:.1e})")
    assert d <= ADJOINT_BOUND
    assert np.array_equal(Y, hs.ldiv_ulv(_op(hs, F, trans), W))


@pytest.mark.parametrize("trans", [1, 2])
@pytest.mark.parametrize("label", list(HANDLES))
def test_handle_against_superlu(hs, label, trans):
    P, F, lu, x0 = handle(hs, label)
    b = P["b"].astype(F.dtype)
    e0 = relerr(hs.ldiv(F, b), lu.solve(b))
    et = relerr(hs.ldiv_ulv(_op(hs, F, trans), b), lu.solve(b, trans="TH"[trans - 1]))
    print(f"{label} trans={trans}: against SuperLU {et:.2e}; the forward hs.ldiv of the same handle {e0:.2e}")
    assert et <= 10 * e0


@pytest.mark.parametrize("label", ["hss_d", "mf2-complex"])
def test_handle_device_entry_point_and_refusals(hs, label):
    import torch

    P, F, lu, x0 = handle(hs, label)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    L = hs._lib.lib()
    fn = L.hs_ldiv_ulv_z if cplx else L.hs_ldiv_ulv_d
    fdev = L.hs_ldiv_ulv_dev_z if cplx else L.hs_ldiv_ulv_dev_d
    pf = hs._lib.p_f64
    B = _block(n, NCOL, cplx, 21)
    for trans in (0, 1, 2):
        ref = hs.ldiv_ulv(_op(hs, F, trans), B)
        dB = torch.from_numpy(np.asfortranarray(B).T.copy()).cuda()  # column-major n x k, ld n
        dC = torch.empty_like(dB)
        hs._lib.check(fdev(F._h, trans, C.c_void_p(dC.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, NCOL, None))
        torch.cuda.synchronize()
        assert np.array_equal(dC.cpu().numpy().T, ref)
    Bm = np.asfortranarray(B[:, :3])
    for bad in (3, -1):
        Cm = np.full((n, 3), 42.0, dtype=F.dtype, order="F")
        assert fn(F._h, bad, Cm.ctypes.data_as(pf), n, Bm.ctypes.data_as(pf), n, n, 3) == hs._lib.HS_ERR_ARGUMENT
        assert np.all(Cm == 42.0)


HANDLES_PLAIN = [
    ("exact", "convdiff_helmholtz", (30, 27), 40, dict(swlevel=0)),
    ("tol1e-4", "convdiff_helmholtz", (24, 24, 24), 300, dict(swlevel=2, swsize=8, atol=1e-4, rtol=1e-4)),
]


@pytest.mark.parametrize("label,kind,shape,nmax,kw", HANDLES_PLAIN, ids=[c[0] for c in HANDLES_PLAIN])
def test_handles_without_hss_fronts_return_the_bits_of_ldiv_block_t(hs, label, kind, shape, nmax, kw):
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], **kw)
    try:
        B = _block(P["A"].shape[0], NCOL, F.dtype.kind == "c", 31)
        for trans in (0, 1, 2):
            Ft = _op(hs, F, trans)
            assert np.array_equal(hs.ldiv_ulv(Ft, B), hs.ldiv_block_t(Ft, B))
    finally:
        F.free()


def test_guard_one_block_call_is_not_slower_than_the_looped_solves(hs):
    """32 columns on the mf = 2 handle: the block call reads the factors once where the loop reads them 32 times."""
    import time

    P, F, lu, x0 = handle(hs, "mf2")
    B = _block(P["A"].shape[0], 32, False, 41)
    hs.ldiv_ulv(F, B)
    hs.ldiv(F, B)
    t0 = time.perf_counter()
    hs.ldiv_ulv(F, B)
    t1 = time.perf_counter()
    hs.ldiv(F, B)
    t2 = time.perf_counter()
    print(f"mf2, 32 columns: one hs.ldiv_ulv call {1e3 * (t1 - t0):.1f} ms, 32 hs.ldiv calls {1e3 * (t2 - t1):.1f} ms")
    assert t1 - t0 <= t2 - t1


def test_zz_stored_factors_are_unchanged(hs):
    """After everything above: hs.ldiv(F, b) on every handle still returns the bits it returned first."""
    for label in HANDLES:
        P, F, lu, x0 = handle(hs, label)
        assert np.array_equal(hs.ldiv(F, P["b"].astype(F.dtype)), x0), label
