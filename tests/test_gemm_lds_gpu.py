"""gemm_op_lds_kernel -- the plain Float64 update with both operands loaded straight into LDS (kernels_gemm.hip, gemm_tile_d_lds) -- against
the register-staged gemm_op_kernel and against NumPy, through hsk_gemm_op_d: one launch of Sched::gemm, routed as a factorization routes it.

The two kernels issue the same MFMAs on the same operands in the same order, so their results must be EQUAL (np.array_equal).  Against
float64 `A @ B` the bound is componentwise 2 gamma_K (|A| |B|), gamma_K = K u / (1 - K u), u = 2^-53: one gamma_K for the kernel's sum of K
products in whatever order, one for NumPy's (Higham, Accuracy and Stability, section 3.5); C starts at zero there, so C = 0 - acc is exact."""
import ctypes as C

import numpy as np
import pytest

from helpers import prepare

pytestmark = pytest.mark.gpu

SIZES = [128, 130, 254, 257, 2]
P_F64 = C.POINTER(C.c_double)
P_I64 = C.POINTER(C.c_int64)


def gemm_op(hs, A, B, C0, lds, koff=0, roff=0):
    """C0[f] - A[f] @ B[f] for the fronts f of one launch, with gemm_op_lds_kernel allowed (lds) or not; returns (list of C, launches routed
    to gemm_op_lds_kernel)."""
    L = hs._lib.lib()
    K = A[0].shape[1]
    M = np.array([a.shape[0] for a in A], dtype=np.int64)
    N = np.array([b.shape[1] for b in B], dtype=np.int64)
    assert all(a.shape[1] == K and b.shape[0] == K for a, b in zip(A, B))
    pack = lambda xs: np.ascontiguousarray(np.concatenate([np.asfortranarray(x).ravel(order="F") for x in xs]))
    a, b, c = pack(A), pack(B), pack(C0)
    routed = C.c_int64(-1)
    prev = L.hsk_gemm_lds_enable(1 if lds else 0)
    try:
        hs._lib.check(L.hsk_gemm_op_d(len(A), M.ctypes.data_as(P_I64), N.ctypes.data_as(P_I64), K, koff, roff, a.ctypes.data_as(P_F64),
                                      b.ctypes.data_as(P_F64), c.ctypes.data_as(P_F64), C.byref(routed), 0, None))
    finally:
        L.hsk_gemm_lds_enable(prev)
    out, o = [], 0
    for m, n in zip(M, N):
        out.append(c[o:o + m * n].reshape((m, n), order="F"))
        o += m * n
    return out, routed.value


def _operands(rng, M, N, K):
    return rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))


def _check_numpy(A, B, negC, K):
    """negC = A @ B as the kernel computed it (C started at zero)"""
    u = 2.0 ** -53
    gamma = K * u / (1.0 - K * u)
    err = np.abs(negC - A @ B)
    bound = 2.0 * gamma * (np.abs(A) @ np.abs(B))
    worst = float(np.max(err / np.maximum(bound, np.finfo(float).tiny)))
    assert np.all(err <= bound), (A.shape, B.shape, worst)
    return worst


@pytest.mark.parametrize("K", [16, 32, 48, 1040])
def test_bits_and_numpy(hs, K):
    """every (M, N) of SIZES^2, one front per launch: the new kernel takes the launch, equals the old one bit for bit, and meets the bound"""
    rng = np.random.default_rng(K)
    worst = 0.0
    for M in SIZES:
        for N in SIZES:
            A, B, C0 = _operands(rng, M, N, K)
            (c1,), r1 = gemm_op(hs, [A], [B], [C0], True)
            (c0,), r0 = gemm_op(hs, [A], [B], [C0], False)
            assert (r1, r0) == (1, 0), (M, N, K, r1, r0)
            assert np.array_equal(c1, c0), (M, N, K, float(np.max(np.abs(c1 - c0))))
            (z1,), r1 = gemm_op(hs, [A], [B], [np.zeros((M, N))], True)
            assert r1 == 1
            worst = max(worst, _check_numpy(A, B, -z1, K))
    print(f"[gemm lds] K={K}: largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("K", [16, 1040])
def test_batch_of_two_fronts(hs, K):
    """two fronts of different size in one launch: 3 x 3 tiles of the bounding box, so gridDim.x = 9 is no multiple of 8 and the second front
    runs the XCD remap with a shift; the smaller front has ragged edge tiles in m and n and whole tiles that fall outside it"""
    rng = np.random.default_rng(100 + K)
    shapes = [(257, 257), (130, 254)]
    ops = [_operands(rng, M, N, K) for M, N in shapes]
    A, B, C0 = [o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops]
    c1, r1 = gemm_op(hs, A, B, C0, True)
    c0, r0 = gemm_op(hs, A, B, C0, False)
    assert (r1, r0) == (1, 0)
    for f in range(2):
        assert np.array_equal(c1[f], c0[f]), (f, K)
    z1, _ = gemm_op(hs, A, B, [np.zeros(s) for s in shapes], True)
    for f in range(2):
        _check_numpy(A[f], B[f], -z1[f], K)


@pytest.mark.parametrize("K,koff,roff", [(40, 0, 0), (48, 1, 0), (48, 0, 1), (48, 1, 1)])
def test_routing(hs, K, koff, roff):
    """K = 40 is no whole number of 16-column steps; koff / roff = 1 put B / A one double off a 16-byte boundary: such launches stay on
    gemm_op_kernel (the hook counts the launches that took the new kernel) and are still right"""
    rng = np.random.default_rng(7 + K + 2 * koff + roff)
    M, N = 257, 130
    A, B, C0 = _operands(rng, M, N, K)
    (c1,), r1 = gemm_op(hs, [A], [B], [C0], True, koff, roff)
    (c0,), r0 = gemm_op(hs, [A], [B], [C0], False, koff, roff)
    assert (r1, r0) == (0, 0)
    assert np.array_equal(c1, c0)
    (z1,), _ = gemm_op(hs, [A], [B], [np.zeros((M, N))], True, koff, roff)
    _check_numpy(A, B, -z1, K)


def test_routing_takes_aligned_launch(hs):
    """the counterpart: the same shape with K = 48 and no offsets does run the new kernel"""
    rng = np.random.default_rng(8)
    A, B, C0 = _operands(rng, 257, 130, 48)
    _, r1 = gemm_op(hs, [A], [B], [C0], True)
    assert r1 == 1


def test_swizzle_single_entry(hs):
    """B is zero except B[k, n]: column n of C must be exactly -A[:, k] * B[k, n] (one product, rounded once) and every other column zero.
    The position runs over all (n mod 16, k mod 16) -- every slot of the swizzled [n][16] image of B and every lane of the operand read --
    with n spread over the eight 16-column blocks of the tile.  A wrong chunk permutation picks another k, i.e. another column of A."""
    rng = np.random.default_rng(9)
    M, N, K = 128, 128, 16
    A = rng.standard_normal((M, K))
    for n16 in range(16):
        for k in range(16):
            n = n16 + 16 * ((n16 + k) % 8)
            B = np.zeros((K, N))
            B[k, n] = rng.standard_normal()
            (c,), r = gemm_op(hs, [A], [B], [np.zeros((M, N))], True)
            assert r == 1
            want = np.zeros((M, N))
            want[:, n] = -(A[:, k] * B[k, n])
            assert np.array_equal(c, want), (n, k)


def test_end_to_end_on_equals_off(hs):
    """poisson3d_32, exact: the solution with the direct-to-LDS updates equals the one without, the flop count too, and launches did go to
    the new kernel"""
    L = hs._lib.lib()
    P = prepare(hs, "poisson3d_32", rhs="randn")
    xs, flops, routed = [], [], []
    for on in (1, 0):
        prev = L.hsk_gemm_lds_enable(on)
        try:
            L.hsk_gemm_lds_launches(1)
            F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
            xs.append(hs.ldiv(F, P["b"]))
            routed.append(L.hsk_gemm_lds_launches(1))
            flops.append(F.stats()["gemm_flops"])
            F.free()
        finally:
            L.hsk_gemm_lds_enable(prev)
    print(f"[gemm lds] poisson3d_32: launches of gemm_op_lds_kernel on {routed[0]} off {routed[1]}, gemm_flops {flops[0]:.6e}")
    assert routed[0] > 0 and routed[1] == 0
    assert np.all(np.isfinite(xs[0]))
    assert np.array_equal(xs[0], xs[1])
    assert flops[0] == flops[1]
