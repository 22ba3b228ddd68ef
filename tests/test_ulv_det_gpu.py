"""hs_hss_logabsdet on the device: the per-node reduction kernel alone on exact data (hsk_ulv_det_*, csrc/kernels_selinv.hip), and
H.logabsdet() against numpy.linalg.slogdet of the expanded matrix on the matrices of tests/test_ulv_t_gpu.py.  The formula itself is pinned
on the CPU in tests/test_ulv_det_host.py."""
import ctypes as C

import numpy as np
import pytest

from test_ulv_t_gpu import dense_of, kernel_matrix

pytestmark = pytest.mark.gpu


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------------

def perm_with_parity(rng, n, odd):
    """A random permutation of 0..n-1 of the wanted parity (n >= 2), with long cycles: the walk of the cycle count has work to do."""
    p = rng.permutation(n)
    seen, cycles = np.zeros(n, bool), 0
    for i in range(n):
        if not seen[i]:
            cycles += 1
            j = i
            while not seen[j]:
                seen[j] = True
                j = p[j]
    if ((n - cycles) & 1) != int(odd):
        p[[0, 1]] = p[[1, 0]]  # one more transposition
    return p.astype(np.int32)


# node sizes around the 64 lanes of the wave and its 32-lane halves, more than one pass of the lanes (70), one entry, and an empty node
# inside the launch; (size, odd permutation)
UNIT = np.array([1.0, 1j, -1.0, -1j])  # quarter turns, exact
NODES = [(1, False), (31, True), (0, False), (32, False), (33, True), (70, False), (70, True), (2, True)]


@pytest.mark.parametrize("cplx", [False, True])
def test_kernel_on_powers_of_two(hs, cplx):
    """Diagonals +-2^k (ComplexF64: 2^k times 1, i, -1, -i): log|u| is k log 2 up to the rounding of one logarithm each and the phase a
    multiple of pi / 2, so the sign of the folded product is exact in Float64 and exact to the rounding of cos / sin in ComplexF64; the
    counts of negative pivots and the parity of every permutation are integers and are checked exactly.  Everything off the diagonal is
    filled with values that would show if the kernel read them."""
    L = hs._lib.lib()
    fn = L.hsk_ulv_det_z if cplx else L.hsk_ulv_det_d
    rng = np.random.default_rng(5 + cplx)
    ni = np.array([n for n, _ in NODES], dtype=np.int64)
    ld = np.array([max(n, 1) + (k % 3) for k, (n, _) in enumerate(NODES)], dtype=np.int64)  # padded leading dimensions
    blocks, perms, expect = [], [], []
    for (n, odd), l in zip(NODES, ld):
        A = np.full((l, n), 777.0, dtype=np.complex128 if cplx else np.float64)
        k = rng.integers(-8, 9, size=n)
        q = rng.integers(0, 4, size=n) if cplx else 2 * rng.integers(0, 2, size=n)  # the phase in quarter turns
        for i in range(n):
            A[i, i] = 2.0 ** k[i] * (UNIT[int(q[i])] if cplx else UNIT[int(q[i])].real)
        p = perm_with_parity(rng, n, odd) if n >= 2 else np.arange(n, dtype=np.int32)
        blocks.append(A.ravel(order="F"))
        perms.append(p)
        expect.append((int(k.sum()), q, odd))
    LU = np.ascontiguousarray(np.concatenate(blocks))
    rp = np.ascontiguousarray(np.concatenate(perms), dtype=np.int32)
    out2 = np.full(2 * len(NODES), np.nan)
    fl = np.full(3 * len(NODES), -7, dtype=np.int32)
    res = np.full(3, np.nan)
    pi32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    pf = lambda a: a.ctypes.data_as(hs._lib.p_f64)
    args = (len(NODES), ni.ctypes.data_as(hs._lib.p_i64), ld.ctypes.data_as(hs._lib.p_i64), pf(LU), pi32(rp))
    hs._lib.check(fn(*args, pf(out2), pi32(fl), pf(res)))
    ksum, quarter, flips = 0, 0, 0
    for j, ((n, odd), (ks, q, _)) in enumerate(zip(NODES, expect)):
        # at most n roundings of log (each |k| log 2 <= 8 log 2 < 6, within 1 ulp = 2^-50) and n additions of sums below 6 n
        assert abs(out2[2 * j] - ks * np.log(2.0)) <= 2.0 * n * (6.0 * n) * 2.0 ** -52, (j, out2[2 * j], ks)
        assert fl[3 * j + 1] == int(odd) and fl[3 * j + 2] == 0, (j, fl[3 * j:3 * j + 3])
        if cplx:
            assert abs(out2[2 * j + 1] - float(np.sum(np.angle(UNIT[q])))) <= 4.0 * n * n * 2.0 ** -52, (j, out2[2 * j + 1])
            quarter += int(q.sum())
        else:
            assert out2[2 * j + 1] == 0.0 and fl[3 * j] == int(np.count_nonzero(q)), (j, fl[3 * j])
            flips += int(np.count_nonzero(q))
        ksum += ks
        flips += int(odd)
    ntot = int(ni.sum())
    assert abs(res[0] - ksum * np.log(2.0)) <= 2.0 * ntot * (6.0 * ntot) * 2.0 ** -52
    if cplx:
        want = UNIT[quarter % 4] * (-1.0) ** flips
        assert abs(complex(res[1], res[2]) - want) <= 1e-12, (res, want)
    else:
        assert res[1] == (-1.0) ** flips and res[2] == 0.0, res
    # two calls: the same bits
    out2b, flb, resb = np.empty_like(out2), np.empty_like(fl), np.empty_like(res)
    hs._lib.check(fn(*args, pf(out2b), pi32(flb), pf(resb)))
    assert np.array_equal(out2, out2b) and np.array_equal(fl, flb) and np.array_equal(res, resb)


def test_kernel_sees_a_zero_pivot_and_the_hook_refuses_bad_input(hs):
    L = hs._lib.lib()
    ni = np.array([3, 2], dtype=np.int64)
    ld = np.array([3, 2], dtype=np.int64)
    LU = np.concatenate([np.diag([2.0, 0.0, 4.0]).ravel(order="F"), np.diag([1.0, -1.0]).ravel(order="F")])
    rp = np.array([0, 1, 2, 0, 1], dtype=np.int32)
    out2, fl, res = np.zeros(4), np.zeros(6, dtype=np.int32), np.zeros(3)
    pi32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    pf = lambda a: a.ctypes.data_as(hs._lib.p_f64)
    pl = lambda a: a.ctypes.data_as(hs._lib.p_i64)
    hs._lib.check(L.hsk_ulv_det_d(2, pl(ni), pl(ld), pf(LU), pi32(rp), pf(out2), pi32(fl), pf(res)))
    assert fl[2] == 1 and fl[5] == 0 and fl[3] == 1
    assert res[0] == -np.inf and res[1] == 0.0 and res[2] == 0.0
    bad = np.array([0, 0, 2, 0, 1], dtype=np.int32)  # not a permutation
    assert L.hsk_ulv_det_d(2, pl(ni), pl(ld), pf(LU), pi32(bad), pf(out2), pi32(fl), pf(res)) == hs._lib.HS_ERR_ARGUMENT
    small = np.array([2, 2], dtype=np.int64)  # ld < ni
    assert L.hsk_ulv_det_d(2, pl(ni), pl(small), pf(LU), pi32(rp), pf(out2), pi32(fl), pf(res)) == hs._lib.HS_ERR_ARGUMENT


# ---- the HSS module ------------------------------------------------------------------------------------------------------------------------

def check_logabsdet(H, complex_, perm=None):
    """The comparison and the tolerance of _check_logabsdet in tests/test_selinv_gpu.py, against the matrix H itself represents."""
    sref, lref = np.linalg.slogdet(dense_of(H, perm))
    sign, la = H.logabsdet()
    print(f"n={H.shape[0]} nodes={H.num_nodes} complex={complex_}: log|det| {la:.12g} (ref {lref:.12g}, rel {abs(la - lref) / max(1.0, abs(lref)):.1e}), "
          f"sign {sign} (ref {sref}, diff {abs(sign - sref):.1e})")
    assert abs(la - lref) <= 1e-11 * max(1.0, abs(lref)), (la, lref)
    assert abs(sign - sref) <= 1e-10, (sign, sref)
    assert isinstance(sign, complex) == complex_
    assert H.logabsdet() == (sign, la)  # a fixed order of additions: the same bits


@pytest.mark.parametrize("complex_", [False, True])
@pytest.mark.parametrize("n,leaf,tol", [(500, 40, 1e-4), (1200, 64, 1e-8), (70, 16, 1e-6)])
def test_hss_logabsdet_against_slogdet(hs, complex_, n, leaf, tol):
    H = hs.hss.compress(kernel_matrix(n, complex_), leafsize=leaf, atol=tol, rtol=tol, kest=32)
    assert H.num_nodes >= 3
    check_logabsdet(H, complex_)


@pytest.mark.parametrize("complex_", [False, True])
def test_hss_logabsdet_single_leaf_uneven_split_permuted_and_negative(hs, complex_):
    H = hs.hss.compress(kernel_matrix(48, complex_), leafsize=64)
    assert H.num_nodes == 1
    check_logabsdet(H, complex_)
    H = hs.hss.compress(kernel_matrix(300, complex_), hs.hss.bisection_cluster((100, 300), leafsize=50), atol=1e-8, rtol=1e-8)
    check_logabsdet(H, complex_)
    n = 400
    perm = np.random.default_rng(11).permutation(n)
    A = np.zeros((n, n), dtype=np.complex128 if complex_ else np.float64)
    A[np.ix_(perm, perm)] = kernel_matrix(n, complex_)
    H = hs.hss.compress(A, leafsize=40, atol=1e-8, rtol=1e-8, kest=32, perm=perm)
    check_logabsdet(H, complex_, perm=perm)
    # one row negated: a negative (complex: rotated by pi) determinant
    A = kernel_matrix(70, complex_)
    A[0] = -A[0]
    H = hs.hss.compress(A, leafsize=16, atol=1e-10, rtol=1e-10, kest=32)
    if not complex_:
        assert np.linalg.slogdet(H.expand())[0] == -1.0
    check_logabsdet(H, complex_)


def test_hss_logabsdet_refuses_a_matrix_that_is_not_eliminated(hs):
    H = hs.hss.compress(kernel_matrix(70), leafsize=16, atol=1e-6, rtol=1e-6, kest=32)
    la, sr, si = C.c_double(7.0), C.c_double(7.0), C.c_double(7.0)
    L = hs._lib.lib()
    assert L.hs_hss_logabsdet(H._h, C.byref(la), C.byref(sr), C.byref(si)) == hs._lib.HS_ERR_ARGUMENT
    assert b"not eliminated" in L.hs_last_error() and (la.value, sr.value, si.value) == (7.0, 7.0, 7.0)
