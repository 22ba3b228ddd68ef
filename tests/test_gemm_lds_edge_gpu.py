"""gemm_op_lds_edge_kernel / gemm_op_env_lds_kernel -- the direct-to-LDS Float64 update for a K that is no multiple of 16 and for an A at an
odd row (kernels_gemm.hip, gemm_tile_d_lds<true>) -- against the register-staged gemm_op_kernel / gemm_op_env_kernel and against NumPy.

The edge tile zero-fills the last, partial K-step as gemm_tile_d does and runs a front with an odd row offset one row higher, so every
entry of C takes the same MFMAs on the same operands in the same order: results must be EQUAL (np.array_equal).  Against float64 `A @ B`
the bound is componentwise 2 gamma_K (|A| |B|) as in test_gemm_lds_gpu.py (gamma_K = K u / (1 - K u), u = 2^-53)."""
import ctypes as C

import numpy as np
import pytest

from helpers import prepare
from test_gemm_lds_gpu import P_F64, P_I64, SIZES, _check_numpy, _operands, gemm_op

pytestmark = pytest.mark.gpu


def edge_op(hs, A, B, C0, lds, roff):
    """gemm_op plus the launches the call sent to the edge kernels"""
    L = hs._lib.lib()
    L.hsk_gemm_lds_edge_launches(1)
    out, routed = gemm_op(hs, A, B, C0, lds, 0, roff)
    return out, routed, L.hsk_gemm_lds_edge_launches(1)


def _one_case(hs, rng, M, N, K, roff):
    A, B, C0 = _operands(rng, M, N, K)
    (c1,), r1, e1 = edge_op(hs, [A], [B], [C0], True, roff)
    (c0,), r0, e0 = edge_op(hs, [A], [B], [C0], False, roff)
    assert (r1, e1, r0, e0) == (0, 1, 0, 0), (M, N, K, roff, r1, e1, r0, e0)
    assert np.array_equal(c1, c0), (M, N, K, roff, float(np.max(np.abs(c1 - c0))))
    (z1,), _, e1 = edge_op(hs, [A], [B], [np.zeros((M, N))], True, roff)
    assert e1 == 1
    return _check_numpy(A, B, -z1, K)


@pytest.mark.parametrize("roff", [0, 1])
@pytest.mark.parametrize("K", [1, 15, 17, 40, 1041])
def test_tail_and_offset_sweep(hs, K, roff):
    """K: a tail only, a tail with the odd straddle, one full step plus one column, an even tail, a long K; roff = 1 puts A at an odd row.
    Every (M, N) of SIZES^2, one front per launch: the edge kernel takes it when allowed, equals the old kernel, meets the bound"""
    rng = np.random.default_rng(1000 * roff + K)
    worst = 0.0
    for M in SIZES:
        for N in SIZES:
            worst = max(worst, _one_case(hs, rng, M, N, K, roff))
    print(f"[gemm lds edge] K={K} roff={roff}: largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("K", [17, 48])
@pytest.mark.parametrize("M", [1, 127, 128, 129])
def test_shift_opens_a_tile_row(hs, M, K):
    """an odd row offset runs the front with M + 1 rows: at M = 128 that is a second tile row (K = 48: the shift alone, no tail)"""
    rng = np.random.default_rng(50 * K + M)
    _one_case(hs, rng, M, 130, K, 1)


def test_single_entry_in_the_tail(hs):
    """B is zero except B[k, n], k in the partial K-step 16..22 of K = 23 (22 is the straddling chunk's only row): column n of C must be
    exactly -A[:, k] * B[k, n] and every other column zero, for every n mod 16"""
    rng = np.random.default_rng(23)
    M, N, K = 128, 128, 23
    A = rng.standard_normal((M, K))
    for k in range(16, K):
        for n16 in range(16):
            n = n16 + 16 * ((n16 + k) % 8)
            B = np.zeros((K, N))
            B[k, n] = rng.standard_normal()
            (c,), r, e = edge_op(hs, [A], [B], [np.zeros((M, N))], True, 0)
            assert (r, e) == (0, 1)
            want = np.zeros((M, N))
            want[:, n] = -(A[:, k] * B[k, n])
            assert np.array_equal(c, want), (n, k)


SCHUR_FRONTS = [(33, 130), (48, 257), (62, 2), (225, 128)]  # (ni, nb): odd and even ni, one fully qualifying front, 3 x 3 tiles of the box


def schur(hs, A, B, C0, lds, env):
    """SB - LF[ni.., :] @ UR for the fronts of one launch through hsk_gemm_schur_d; returns (list of C, launches of gemm_op_lds_kernel, of the
    edge kernels)"""
    L = hs._lib.lib()
    ni = np.array([a.shape[1] for a in A], dtype=np.int64)
    nb = np.array([a.shape[0] for a in A], dtype=np.int64)
    pack = lambda xs: np.ascontiguousarray(np.concatenate([np.asfortranarray(x).ravel(order="F") for x in xs]))
    a, b, c = pack(A), pack(B), pack(C0)
    r_lds, r_edge = C.c_int64(-1), C.c_int64(-1)
    prev = L.hsk_gemm_lds_enable(1 if lds else 0)
    try:
        hs._lib.check(L.hsk_gemm_schur_d(len(A), ni.ctypes.data_as(P_I64), nb.ctypes.data_as(P_I64), a.ctypes.data_as(P_F64), b.ctypes.data_as(P_F64),
                                         c.ctypes.data_as(P_F64), 1 if env else 0, C.byref(r_lds), C.byref(r_edge), 0, None))
    finally:
        L.hsk_gemm_lds_enable(prev)
    out, o = [], 0
    for n in nb:
        out.append(c[o:o + n * n].reshape((n, n), order="F"))
        o += n * n
    return out, r_lds.value, r_edge.value


@pytest.mark.parametrize("env", [0, 1])
def test_schur_form(hs, env):
    """one launch over fronts with their own ni and nb: K = ni and A's row offset ni differ from front to front.  env: the operands get a
    staircase of leading zeros per 32-block (some rows of A wholly zero) and the launch is enveloped -- tiles start their K loop late or
    do not run"""
    rng = np.random.default_rng(77 + env)
    A, B, C0 = [], [], []
    for ni, nb in SCHUR_FRONTS:
        a, b, c = _operands(rng, nb, nb, ni)
        if env:
            for r in range(nb):
                a[r, :32 * ((r // 32) % 4)] = 0.0
            for col in range(nb):
                b[:32 * (((col // 32) + 1) % 3), col] = 0.0
        A.append(a), B.append(b), C0.append(c)
    c1, l1, e1 = schur(hs, A, B, C0, True, env)
    c0, l0, e0 = schur(hs, A, B, C0, False, env)
    assert (l1, e1, l0, e0) == (0, 1, 0, 0)
    for f in range(len(A)):
        assert np.array_equal(c1[f], c0[f]), (f, SCHUR_FRONTS[f], float(np.max(np.abs(c1[f] - c0[f]))))
    z1, _, _ = schur(hs, A, B, [np.zeros_like(c) for c in C0], True, env)
    for f, (ni, nb) in enumerate(SCHUR_FRONTS):
        _check_numpy(A[f], B[f], -z1[f], ni)


def test_end_to_end_on_equals_off(hs):
    """poisson3d_32, exact: solution and flop count are equal with the direct-to-LDS updates on and off; with them on, launches go to the
    edge kernels and no plain Float64 update is left on the register-staged ones"""
    L = hs._lib.lib()
    P = prepare(hs, "poisson3d_32", rhs="randn")
    xs, flops, edge, reg, lds = [], [], [], [], []
    for on in (1, 0):
        prev = L.hsk_gemm_lds_enable(on)
        try:
            L.hsk_gemm_lds_launches(1), L.hsk_gemm_lds_edge_launches(1), L.hsk_gemm_reg_launches(1)
            F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
            xs.append(hs.ldiv(F, P["b"]))
            lds.append(L.hsk_gemm_lds_launches(1)), edge.append(L.hsk_gemm_lds_edge_launches(1)), reg.append(L.hsk_gemm_reg_launches(1))
            flops.append(F.stats()["gemm_flops"])
            F.free()
        finally:
            L.hsk_gemm_lds_enable(prev)
    print(f"[gemm lds edge] poisson3d_32: on: lds {lds[0]} edge {edge[0]} reg {reg[0]}   off: lds {lds[1]} edge {edge[1]} reg {reg[1]}   gemm_flops {flops[0]:.6e}")
    assert edge[0] > 0 and reg[0] == 0
    assert lds[1] == 0 and edge[1] == 0 and reg[1] == lds[0] + edge[0]
    assert np.all(np.isfinite(xs[0]))
    assert np.array_equal(xs[0], xs[1])
    assert flops[0] == flops[1]
