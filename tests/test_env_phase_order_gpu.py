"""The K-sorted tile order of the enveloped plain updates (GemmOp::order 2, csrc/kernels_gemm.hip; DESIGN.md section 4 "K-sorted order") on
the device: the kernel that writes its tables against NumPy, and factorizations under order 2 against the same process under order 0 --
the order changes which workgroup runs a tile, never the tile, so every stored block and the solution must be EQUAL, not close."""
import ctypes as C

import numpy as np
import pytest

from helpers import prepare
from test_env_tile_order_gpu import _batch, _odd_cube, _two_block_front

pytestmark = pytest.mark.gpu

BIG = 1 << 30  # HS_BIG / HS_ENV_NONE
LF, UR, SB = 0, 1, 2


class env_order:
    """with env_order(hs, order): ... -- leaf and branch envelopes on, the tile order 0 / 1 / 2; the previous settings come back afterwards"""

    def __init__(self, hs, order):
        self.L, self.order = hs._lib.lib(), order

    def __enter__(self):
        self.prev_leaf = self.L.hsk_envelope_enable(1)
        self.prev_branch = self.L.hsk_branch_envelope_enable(1)
        self.prev = self.L.hsk_env_order_enable(self.order)

    def __exit__(self, *a):
        assert self.L.hsk_env_order_enable(self.prev) == self.order  # the switch returns what was set
        self.L.hsk_branch_envelope_enable(self.prev_branch)
        self.L.hsk_envelope_enable(self.prev_leaf)


@pytest.fixture(autouse=True)
def every_front_takes_order_2(hs):
    """production leaves fronts of fewer than 2048 tiles on the balanced order (hsk_env_perm_min_tiles); the fronts here are smaller"""
    L = hs._lib.lib()
    prev = L.hsk_env_perm_min_tiles(0)
    yield
    assert L.hsk_env_perm_min_tiles(prev) == 0


def test_small_fronts_keep_the_balanced_order_by_default(hs, edge_batch):
    """with the default limit every front of the batch (441 tiles at most) is flagged and runs order 1: the same bits again"""
    Fs, envs, nis = edge_batch
    L = hs._lib.lib()
    assert L.hsk_env_perm_min_tiles(-1) == 0
    try:
        small = _run_orders(hs, Fs, nis, envs, (2,), sorted_expected=False)[0]  # no launch of the batch reaches the limit: no table is written
    finally:
        L.hsk_env_perm_min_tiles(0)
    ref = _run_orders(hs, Fs, nis, envs, (0,))[0]
    for name in ("LF", "UR", "SB", "rperm"):
        assert np.array_equal(small[name], ref[name]), name


# ---- the permutation kernel against a stable argsort --------------------------------------------------------------------------------------


def _stride(slot):
    return (2 + 2 * slot * slot + 2 * slot + (slot // 8) ** 2 + 1) & ~1


def _env_min(first, ni, lo, hi):
    blk = lambda p: p >> 5 if p < ni else ((ni + 31) >> 5) + ((p - ni) >> 5)  # noqa: E731  (hs_env_block)
    return min(int(first[b]) for b in range(blk(lo), blk(hi - 1) + 1))


def _keys(ni, nb, env, op, bm, bn, edge):
    """K starts of the tile rows / columns of a plain update, by the rules of resolve_op and hs_env_kstart restated: (kr, kc, kend)"""
    cmat, bmat, r0, r1, c0, c1, k0, k1 = op
    m = ni + nb
    crows, ccols = {LF: (m, ni), UR: (ni, nb), SB: (nb, nb)}[cmat]
    M, N, K = min(r1, crows) - r0, min(c1, ccols) - c0, min(k1, ni) - k0
    row0, col0 = r0 + (ni if cmat == SB else 0), c0 + (0 if cmat == LF else ni)
    if edge and row0 % 2:  # the edge tile runs a front whose A sits at an odd row from one row higher
        row0, M = row0 - 1, M + 1
    nblk = (ni + 31) // 32 + (nb + 31) // 32
    fL, fU = env[:nblk], env[nblk:]
    kend = k0 + K
    kr = [min(max(_env_min(fL, ni, row0 + lo, row0 + min(lo + bm, M)), k0), kend) for lo in range(0, M, bm)]
    kc = [min(max(_env_min(fU, ni, col0 + lo, col0 + min(lo + bn, N)), k0), kend) for lo in range(0, N, bn)]
    return np.asarray(kr, dtype=np.int32), np.asarray(kc, dtype=np.int32), kend


def _two_block_tables(ni, nb, ni1, nb1):
    first = [0 if b0 < ni1 else (ni1 // 32) * 32 for b0 in range(0, ni, 32)] + [0 if b0 < nb1 else (ni1 // 32) * 32 for b0 in range(0, nb, 32)]
    return np.asarray(first + first, dtype=np.int32)


def _banded_tables(ni, nb, seed):
    """leaf-like: every interior block starts a few blocks left of its diagonal, every boundary block somewhere in the interior or nowhere"""
    rng = np.random.default_rng(seed)
    nI, nB = (ni + 31) // 32, (nb + 31) // 32
    out = []
    for _ in range(2):
        inner = [32 * max(0, b - int(rng.integers(0, 4))) for b in range(nI)]
        outer = [BIG if rng.random() < 0.2 else 32 * int(rng.integers(0, nI)) for _ in range(nB)]
        out += inner + outer
    return np.asarray(out, dtype=np.int32)


PERM_CASES = {
    # name: (complex, ni, nb, tables, op (cmat, bmat, r0, r1, c0, c1, k0, k1), edge)
    "two_block_schur": (0, 1024, 2600, _two_block_tables(1024, 2600, 512, 1300), (SB, UR, 0, BIG, 0, BIG, 0, BIG), 1),
    "two_block_trailing": (0, 2048, 1500, _two_block_tables(2048, 1500, 1056, 700), (LF, LF, 1024, BIG, 1024, BIG, 0, 1024), 1),
    "banded_leaf": (0, 700, 1900, _banded_tables(700, 1900, 5), (SB, UR, 0, BIG, 0, BIG, 0, BIG), 0),
    "shifted_odd_ni": (0, 1023, 2450, _two_block_tables(1023, 2450, 500, 1200), (SB, UR, 0, BIG, 0, BIG, 0, BIG), 1),
    "complex": (1, 640, 1500, _banded_tables(640, 1500, 6), (SB, UR, 0, BIG, 0, BIG, 0, BIG), 0),
    "complex_two_block_ur": (1, 1024, 1200, _two_block_tables(1024, 1200, 480, 600), (UR, UR, 512, BIG, 0, BIG, 0, 512), 0),
}


@pytest.mark.parametrize("name", list(PERM_CASES))
def test_permutation_kernel_against_numpy(hs, name):
    is_complex, ni, nb, env, op, edge = PERM_CASES[name]
    L = hs._lib.lib()
    bm, bn = 128, (64 if is_complex else 128)
    kr, kc, kend = _keys(ni, nb, env, op, bm, bn, edge and not is_complex)
    tiles_m, tiles_n = kr.size, kc.size
    slot = (max(tiles_m, tiles_n) + 7) // 8 * 8
    out = np.zeros(_stride(slot), dtype=np.uint16)
    p32 = C.POINTER(C.c_int32)
    assert L.hsk_env_perm(is_complex, ni, nb, env.ctypes.data_as(p32), *op, edge, slot, out.ctypes.data_as(C.POINTER(C.c_uint16))) == 0
    assert out[0] == 1
    tail = out[2 + 2 * slot * slot :]
    assert np.array_equal(tail[:tiles_m], np.argsort(kr, kind="stable")), (kr, tail[:tiles_m])
    assert np.array_equal(tail[slot : slot + tiles_n], np.argsort(kc, kind="stable")), (kc, tail[slot : slot + tiles_n])
    assert np.unique(kr).size > 1 or np.unique(kc).size > 1  # the case sorts something
    # the unit order: stable by the summed K starts of a unit's 64 tiles
    skr, skc = np.sort(kr, kind="stable").astype(np.int64), np.sort(kc, kind="stable").astype(np.int64)
    gm, gn = tiles_m // 8, tiles_n // 8
    usum = [np.maximum.outer(skr[8 * g : 8 * g + 8], skc[8 * c : 8 * c + 8]).sum() for g in range(gm) for c in range(gn)]
    assert np.array_equal(tail[2 * slot : 2 * slot + gm * gn], np.argsort(np.asarray(usum), kind="stable"))
    # and the table the update reads is the host's map for the same keys (first front of a launch: shift 0)
    n = tiles_m * tiles_n
    tm, tn = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    assert L.hsk_env_phase_order(tiles_m, tiles_n, kr.ctypes.data_as(p32), kc.ctypes.data_as(p32), 0, tm.ctypes.data_as(p32), tn.ctypes.data_as(p32), None) == 0
    table = out[2 : 2 + 2 * n].reshape(n, 2)
    assert np.array_equal(table[:, 0], tm) and np.array_equal(table[:, 1], tn)


def test_a_front_that_does_not_fit_its_slot_is_flagged(hs):
    _, ni, nb, env, op, edge = PERM_CASES["two_block_schur"]  # 21 tile rows
    L = hs._lib.lib()
    out = np.full(_stride(16), 7, dtype=np.uint16)
    assert L.hsk_env_perm(0, ni, nb, env.ctypes.data_as(C.POINTER(C.c_int32)), *op, edge, 16, out.ctypes.data_as(C.POINTER(C.c_uint16))) == 0
    assert out[0] == 0


# ---- factorizations: order 2 against order 0 -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["poisson3d_32", "odd_cube", "helmholtz3d_32"])
def test_order_2_equals_order_0_bitwise(hs, name):
    """poisson3d_32: the root (ni = 2048) on the look-ahead schedule -- main and side stream write their tables side by side --, level 2 on
    the recursive one; odd_cube: the shifted edge route; helmholtz3d_32: ComplexF64, which keeps the balanced order.  The launches route as before."""
    P = _odd_cube(hs) if name == "odd_cube" else prepare(hs, name, rhs="randn")
    L = hs._lib.lib()
    Fs, routes = [], []
    sorted_launches = []
    for order in (2, 0):
        L.hsk_gemm_lds_launches(1), L.hsk_gemm_lds_edge_launches(1), L.hsk_gemm_reg_launches(1), L.hsk_env_perm_launches(1)
        with env_order(hs, order):
            Fs.append(hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0, keep_schur=True))
        routes.append((L.hsk_gemm_lds_launches(1), L.hsk_gemm_lds_edge_launches(1), L.hsk_gemm_reg_launches(1)))
        sorted_launches.append(L.hsk_env_perm_launches(1))
    F2, F0 = Fs
    assert routes[0] == routes[1], routes
    assert sorted_launches[1] == 0
    if name != "helmholtz3d_32":
        assert routes[0][1] > 0, routes  # enveloped Float64 updates ran
        assert 0 < sorted_launches[0] <= routes[0][1], (sorted_launches, routes)  # ... and some of them in the K-sorted order
    else:
        assert sorted_launches[0] == 0  # ComplexF64 runs the register-staged kernel, which holds no K-sorted order: setting 2 must change nothing
    assert F2.nnodes == F0.nnodes
    for k in range(F2.nnodes):
        b2, b0 = F2.node_blocks(k, with_schur=True), F0.node_blocks(k, with_schur=True)
        for blk in ("LU", "Lbi", "Uib", "S", "rperm"):
            assert np.array_equal(b2[blk], b0[blk]), (k, blk, F2.node_info(k))
    x2, x0 = hs.ldiv(F2, P["b"]), hs.ldiv(F0, P["b"])
    assert np.array_equal(x2, x0)
    assert np.all(np.isfinite(x2))
    F2.free()
    F0.free()
    # the kernels' own count of the K-steps they ran is still the host's with the switch at 2.  (A counted launch runs the register-staged
    # kernel, which holds no K-sorted order: these launches run the balanced order, and the counter below says so.)
    L.hsk_env_perm_launches(1)
    Fc, dev = _factor_counted_order2(hs, P)
    host = Fc.stats()["gemm_flops"]
    print(f"[env phase order] {name}: gemm_flops host {host:.17g} device {dev:.17g}")
    assert dev == host
    assert L.hsk_env_perm_launches(1) == 0
    Fc.free()


def _factor_counted_order2(hs, P):
    L = hs._lib.lib()
    with env_order(hs, 2):
        assert L.hsk_op_flops_mode(1) == 0
        try:
            F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
            out = C.c_double()
            assert L.hsk_op_flops(C.byref(out)) == 0
        finally:
            L.hsk_op_flops_mode(0)
    return F, out.value


# ---- synthetic batches with caller-made tables -------------------------------------------------------------------------------------------------


def _front_from_tables(ni, nb, first, seed):
    """a front whose entries sit inside the block envelope `first` (one table for firstL and firstU: symmetric pattern), strongly diagonally
    dominant"""
    rng = np.random.default_rng(seed)
    m = ni + nb
    blk = np.where(np.arange(m) < ni, np.arange(m) >> 5, ((ni + 31) >> 5) + ((np.arange(m) - ni) >> 5))
    start = first[blk].astype(np.int64)  # first interior column of a row = first interior row of a column
    c = np.arange(m)
    ok_row = (c[None, :] >= ni) | (c[None, :] >= start[:, None])
    ok = ok_row & ok_row.T
    F = np.where(ok, rng.standard_normal((m, m)), 0.0)
    F[c, c] += 4.0 * m
    return F, np.concatenate([first, first]).astype(np.int32)


def _increasing_front(seed):
    """[int1; int2 | bnd1; bnd2] with ni1 = 256 of ni = 512: block b of int2 starts at column 32 (b - 8), so the keys of the trailing updates
    are not two-valued"""
    ni, nb = 512, 1200
    first = [0] * 8 + [32 * (b - 8) for b in range(8, 16)] + [0 if b0 < 600 else 256 for b0 in range(0, nb, 32)]
    return _front_from_tables(ni, nb, np.asarray(first, dtype=np.int32), seed)


SHAPES = [(256, 2600), (256, 2450), (256, 1100), (256, 300)]


@pytest.fixture(scope="module")
def edge_batch():
    """the Schur tilings 21, 20, 9, 3 of tests/test_env_tile_order_gpu.py plus a front with a strictly increasing table"""
    fronts = [_two_block_front(ni, nb, 200 + nb) for ni, nb in SHAPES] + [_increasing_front(9)]
    return [f for f, _ in fronts], [e for _, e in fronts], [ni for ni, _ in SHAPES] + [512]


def _run_orders(hs, Fs, nis, envs, orders, sorted_expected=True):
    """the batch under every order of `orders`; the launches of the table kernel say whether the K-sorted order really ran"""
    L = hs._lib.lib()
    res = []
    for order in orders:
        L.hsk_gemm_lds_edge_launches(1), L.hsk_env_perm_launches(1)
        with env_order(hs, order):
            res.append(_batch(hs, Fs, nis, envs))
        assert L.hsk_gemm_lds_edge_launches(1) > 0  # the clipped updates ran the enveloped kernel
        n = L.hsk_env_perm_launches(1)
        assert (n > 0) if (order == 2 and sorted_expected) else (n == 0), (order, n)
    return res


def test_synthetic_batch_orders_2_1_0(hs, edge_batch):
    Fs, envs, nis = edge_batch
    res = _run_orders(hs, Fs, nis, envs, (2, 1, 0))
    for other in res[1:]:
        for name in ("LF", "UR", "SB", "rperm"):
            assert np.array_equal(res[0][name], other[name]), name
    # and the Schur complement is the Schur complement: a tile skipped by every order would keep F's own block
    k = 2  # the 9 x 9 front
    ni, nb = SHAPES[k]
    off = sum(n * n for _, n in SHAPES[:k])
    S = res[0]["SB"][off : off + nb * nb].reshape((nb, nb), order="F")
    F = Fs[k]
    Sref = F[ni:, ni:] - F[ni:, :ni] @ np.linalg.solve(F[:ni, :ni], F[:ni, ni:])
    assert np.max(np.abs(S - Sref)) <= 1e-12 * np.max(np.abs(Sref))


def test_fronts_that_do_not_fit_their_slot_take_the_fallback(hs, edge_batch):
    """slots of 8 tile rows / columns: every front of the batch but the 3 x 3 one has more and runs the balanced order, decided on the device
    (the table kernel is launched and flags them: test_a_front_that_does_not_fit_its_slot_is_flagged reads such a flag)"""
    Fs, envs, nis = edge_batch
    L = hs._lib.lib()
    prev = L.hsk_env_perm_slot_limit(8)
    try:
        small = _run_orders(hs, Fs, nis, envs, (2,))[0]
    finally:
        assert L.hsk_env_perm_slot_limit(prev) == 8
    ref = _run_orders(hs, Fs, nis, envs, (0,))[0]
    for name in ("LF", "UR", "SB", "rperm"):
        assert np.array_equal(small[name], ref[name]), name


def test_walking_launch(hs):
    """40 fronts with ni = 256, nb = 1400: 11 x 11 tiles x 40 >= 4096.  Boundary rows and columns from 512 on have nothing in the interior
    (7 of the 11 tile rows and columns are empty and sort last), so the launch walks: 24 workgroups per front for 121 virtual block ids"""
    ni, nb, count = 256, 1400, 40
    first = np.asarray([0] * 8 + [0 if b0 < 512 else BIG for b0 in range(0, nb, 32)], dtype=np.int32)
    F, env = _front_from_tables(ni, nb, np.minimum(first, ni), 31)  # (entries: a start at ni leaves no interior column)
    env = np.concatenate([first, first])
    Fs, envs, nis = [F] * count, [env] * count, [ni] * count
    res = _run_orders(hs, Fs, nis, envs, (2, 1, 0))
    for other in res[1:]:
        for name in ("LF", "UR", "SB", "rperm"):
            assert np.array_equal(res[0][name], other[name]), name
    off = (count - 1) * nb * nb  # the last front
    S = res[0]["SB"][off : off + nb * nb].reshape((nb, nb), order="F")
    Sref = F[ni:, ni:] - F[ni:, :ni] @ np.linalg.solve(F[:ni, :ni], F[:ni, ni:])
    assert np.max(np.abs(S - Sref)) <= 1e-12 * np.max(np.abs(Sref))
