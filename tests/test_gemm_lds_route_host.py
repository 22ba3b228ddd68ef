"""hsk_gemm_lds_route -- which kernel a plain Float64 update of one front may run (hs_common.h, hs_gemm_lds_route) -- on the host, no GPU:
0 register-staged gemm_op_kernel, 1 gemm_op_lds_kernel, 2 gemm_op_lds_edge_kernel.  The direct-to-LDS kernels need an even k0 (B 16-byte
aligned); gemm_op_lds_kernel on top of that whole 16-column K-steps and an even row offset of A, which is r0, plus ni when C is SB."""
import itertools

import pytest

LF, UR, SB = 0, 1, 2
REG, LDS, EDGE = 0, 1, 2


@pytest.fixture(scope="module")
def route(hs):
    return hs._lib.lib().hsk_gemm_lds_route


@pytest.mark.parametrize("cmat", [LF, UR, SB])
def test_every_combination(route, cmat):
    """K mod 16 in {0, 8, 15} x k0 parity x r0 parity x ni parity, with k1 inside the front and with k1 clipped by ni"""
    seen = set()
    for kmod, k0, r0, nipar in itertools.product((0, 8, 15), (32, 33), (64, 65), (0, 1)):
        K = 48 + kmod
        for clipped in (False, True):
            # clipped: k1 is "everything" and K = ni - k0; else k1 = k0 + K lies inside a longer front
            ni = k0 + K if clipped else k0 + K + 100
            ni += (ni & 1) ^ nipar
            if clipped:
                K = ni - k0
            k1 = (1 << 30) if clipped else k0 + K
            arow = r0 + (ni if cmat == SB else 0)
            want = REG if k0 & 1 else (LDS if K % 16 == 0 and arow % 2 == 0 else EDGE)
            got = route(cmat, r0, k0, k1, ni)
            assert got == want, (cmat, r0, k0, k1, ni, K, got, want)
            seen.add(want)
    assert seen == {REG, LDS, EDGE}


def test_named_cases(route):
    """the launches of a factorization the rule was written for"""
    big = 1 << 30
    assert route(SB, 0, 0, big, 7938) == EDGE   # Schur update, K = ni = 7938: a K tail, even offset
    assert route(SB, 0, 0, big, 961) == EDGE    # ragged K and an odd row offset ni
    assert route(SB, 0, 0, big, 4096) == LDS    # whole K-steps, even ni
    assert route(SB, 0, 0, big, 4097) == EDGE   # K = 4097
    assert route(UR, 256, 0, 256, 3375) == LDS  # U12 update inside an odd front: r0 and K are what count, not ni
    assert route(UR, 257, 0, 256, 3375) == EDGE
    assert route(LF, 256, 1, 257, 3375) == REG  # an odd k0 stays on the register-staged kernel
    assert route(UR, 0, 64, 64, 100) == REG     # nothing to do
    assert route(UR, 0, 128, big, 100) == REG


def test_ni_counts_toward_the_row_offset_only_under_sb(route):
    """written out by hand: with C in LF or UR the row offset of A is r0 alone, whatever the parity of ni; with C in SB it is r0 + ni"""
    big = 1 << 30
    # odd ni = 3375, K = 256 (whole steps), even k0
    assert route(LF, 512, 256, 512, 3375) == LDS    # r0 even: ni must not count
    assert route(UR, 512, 256, 512, 3375) == LDS
    assert route(SB, 512, 256, 512, 3375) == EDGE   # 512 + 3375 is odd
    assert route(LF, 513, 256, 512, 3375) == EDGE   # r0 odd
    assert route(UR, 513, 256, 512, 3375) == EDGE
    assert route(SB, 513, 256, 512, 3375) == LDS    # 513 + 3375 is even
    # even ni = 2944 = 184 * 16: nothing changes between the three
    for cmat in (LF, UR, SB):
        assert route(cmat, 512, 256, 512, 2944) == LDS
        assert route(cmat, 513, 256, 512, 2944) == EDGE
    # k1 clipped by an odd ni: K = 3375 - 3328 = 47, a tail whatever the offsets
    for cmat in (LF, UR, SB):
        assert route(cmat, 3328, 3328, big, 3375) == EDGE
    # odd k0 wins over everything
    for cmat in (LF, UR, SB):
        assert route(cmat, 512, 255, 511, 3375) == REG
