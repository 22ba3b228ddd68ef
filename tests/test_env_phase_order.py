"""hsk_env_phase_order -- which tile a block id of an enveloped plain update runs under the K-sorted order (GemmOp::order 2,
csrc/kernels_gemm.hip: env_rank, env_unit_key, env_phase_pos, env_phase_coords; DESIGN.md section 4 "K-sorted order") -- on the host, no
GPU, by the functions the kernels call.

The sequence of positions the block ids are dealt from starts with the whole units: unit u < (tiles_m // 8) * (tiles_n // 8) is the 64
positions [64 u, 64 u + 64).  Those are the "complete units" below.  (The rest of the sequence walks the right strip of fewer than 8 tile
columns and the bottom strip of fewer than 8 tile rows: 64 consecutive positions there cannot be 8 rows x 8 columns -- on 19 x 21 tiles no
order at all puts 6 x 64 of the 399 tiles into 8 x 8 windows, only 2 x 2 of them exist.)

Checked: the map is a bijection onto the tile grid for every tiling, shift and key profile (a tile skipped is a block of the front left
without its update); complete units hold 8 tile rows x 8 tile columns and, for a two-block front, one K start; the XCDs get the same summed
K length to within 10 % under the two-block cost, the bound tests/test_env_tile_order.py sets for the balanced order; and no fewer tiles
than under the balanced order run beside tiles of their own K start only."""
import ctypes as C

import numpy as np
import pytest

XCDS = 8
TILINGS = [(1, 1), (3, 3), (8, 8), (9, 9), (19, 21), (21, 20), (95, 95), (128, 128), (256, 3), (3, 256)]
KEND = 4096  # K end of the launch: a tile row or column whose key is KEND has nothing left


def _keys(n, profile):
    """K starts of n tile rows (or columns): what env_perm_kernel computes from a front's tables"""
    i = np.arange(n)
    if profile == "constant":
        k = np.zeros(n)
    elif profile.startswith("two_block"):  # child 1 = the first n1 tile rows, full K; child 2 starts at ni1 = KEND / 2
        num, den = {"two_block_1_3": (1, 3), "two_block_1_2": (1, 2), "two_block_2_3": (2, 3)}[profile]
        k = np.where(i < (n * num) // den, 0, KEND // 2)
    elif profile == "increasing":  # the triangular profile of int2 rows: every tile row starts 32 columns later
        k = 32 * i
    elif profile == "empty":  # two-block with every third row of child 2 empty, and the first row
        k = np.where(i < n // 2, 0, KEND // 2)
        k = np.where((i % 3 == 0) & ((i >= n // 2) | (i == 0)), KEND, k)
    else:
        raise ValueError(profile)
    return np.ascontiguousarray(k, dtype=np.int32)


PROFILES = ["constant", "two_block_1_3", "two_block_1_2", "two_block_2_3", "increasing", "empty"]


def _order2(hs, tiles_m, tiles_n, kr, kc, shift):
    L = hs._lib.lib()
    n = tiles_m * tiles_n
    tm, tn, pos = (np.full(n, -1, dtype=np.int32) for _ in range(3))
    p32 = C.POINTER(C.c_int32)
    assert L.hsk_env_phase_order(tiles_m, tiles_n, kr.ctypes.data_as(p32), kc.ctypes.data_as(p32), shift, tm.ctypes.data_as(p32),
                                 tn.ctypes.data_as(p32), pos.ctypes.data_as(p32)) == 0
    return tm, tn, pos


def _order01(hs, tiles_m, tiles_n, order):
    L = hs._lib.lib()
    tm = np.full(tiles_m * tiles_n, -1, dtype=np.int32)
    tn = np.full(tiles_m * tiles_n, -1, dtype=np.int32)
    p32 = C.POINTER(C.c_int32)
    assert L.hsk_env_tile_order(tiles_m, tiles_n, order, tm.ctypes.data_as(p32), tn.ctypes.data_as(p32)) == 0
    return tm, tn


def _assert_bijection(tm, tn, tiles_m, tiles_n, what):
    assert tm.min() >= 0 and tm.max() < tiles_m and tn.min() >= 0 and tn.max() < tiles_n, what
    seen = np.bincount(tm.astype(np.int64) * tiles_n + tn, minlength=tiles_m * tiles_n)
    assert seen.size == tiles_m * tiles_n and np.all(seen == 1), what


@pytest.mark.parametrize("shape", TILINGS)
def test_bijection_and_units(hs, shape):
    tiles_m, tiles_n = shape
    nfull = (tiles_m // 8) * (tiles_n // 8)
    for prof_m in PROFILES:
        for prof_n in (prof_m, "constant"):
            kr, kc = _keys(tiles_m, prof_m), _keys(tiles_n, prof_n)
            for shift in range(8):
                what = (shape, prof_m, prof_n, shift)
                tm, tn, pos = _order2(hs, tiles_m, tiles_n, kr, kc, shift)
                _assert_bijection(tm, tn, tiles_m, tiles_n, what)
                assert np.array_equal(np.sort(pos), np.arange(tiles_m * tiles_n)), what  # block id -> position is one too
                by_pos = np.argsort(pos)
                start = np.maximum(kr[tm], kc[tn])[by_pos]
                um, un = tm[by_pos][: 64 * nfull].reshape(nfull, 64), tn[by_pos][: 64 * nfull].reshape(nfull, 64)
                for u in range(nfull):  # a complete unit: 8 tile rows x 8 tile columns, each pair once
                    assert np.unique(um[u]).size == 8 and np.unique(un[u]).size == 8, (what, u)
                # heavy units first: the summed K starts of the complete units do not fall along the sequence
                sums = start[: 64 * nfull].reshape(nfull, 64).sum(axis=1)
                assert np.all(np.diff(sums) >= 0), what
                # the first 64 F block ids of an XCD, F = whole rounds of 8 units, run F complete units one after the other: the 64 workgroups
                # an XCD holds at a time are one unit
                F = nfull // 8
                for x in range(XCDS):
                    mine = np.flatnonzero((np.arange(tm.size) + shift) % XCDS == x)[: 64 * F]
                    assert np.all(pos[mine].reshape(F, 64) // 64 == (pos[mine].reshape(F, 64) // 64)[:, :1]), (what, x)


def test_two_block_units_have_one_k_start(hs):
    """128 x 128 tiles, child 1 = the first 64 tile rows and columns: the split falls on a unit boundary, so every complete unit (all 256
    of them) has exactly one K start"""
    T = 128
    k = np.ascontiguousarray(np.where(np.arange(T) < 64, 0, KEND // 2), dtype=np.int32)
    for shift in range(8):
        tm, tn, pos = _order2(hs, T, T, k, k, shift)
        start = np.maximum(k[tm], k[tn])[np.argsort(pos)].reshape(-1, 64)
        assert start.shape[0] == 256
        assert np.all(start == start[:, :1]), shift


def _heaviest_over_mean(tm, tn, n1m, n1n, shift):
    """the two-block cost of tests/test_env_tile_order.py: bnd1 x bnd1 runs all of K, every other tile half of it; block id bid of a front
    at XCD shift `shift` sits on XCD (bid + shift) & 7"""
    cost = np.where((tm < n1m) & (tn < n1n), 1.0, 0.5)
    per_xcd = np.bincount((np.arange(cost.size) + shift) & (XCDS - 1), weights=cost, minlength=XCDS)
    return per_xcd.max() / per_xcd.mean()


def _two_block(n, n1):
    return np.ascontiguousarray(np.where(np.arange(n) < n1, 0, KEND // 2), dtype=np.int32)


BALANCE = [(T, T, n1) for T, n1 in [(62, 31), (94, 47), (95, 47), (127, 63), (128, 64), (256, 128), (95, 32), (95, 63)]]  # those of the balanced order's test
BALANCE += [(tm_, tn_, None) for tm_, tn_ in TILINGS if min(tm_, tn_) >= 19]  # and the tilings above with T >= 19, nb1 at 1/3, 1/2, 2/3


@pytest.mark.parametrize("tiles_m,tiles_n,n1", BALANCE)
def test_balance(hs, tiles_m, tiles_n, n1):
    splits = [(n1, n1)] if n1 is not None else [((tiles_m * a) // b, (tiles_n * a) // b) for a, b in ((1, 3), (1, 2), (2, 3))]
    for n1m, n1n in splits:
        kr, kc = _two_block(tiles_m, n1m), _two_block(tiles_n, n1n)
        worst = 0.0
        for shift in range(8):
            tm, tn, _ = _order2(hs, tiles_m, tiles_n, kr, kc, shift)
            worst = max(worst, _heaviest_over_mean(tm, tn, n1m, n1n, shift))
        one = _heaviest_over_mean(*_order01(hs, tiles_m, tiles_n, 1), n1m, n1n, 0)
        print(f"[env phase order] {tiles_m} x {tiles_n} split {n1m}, {n1n}: heaviest XCD / mean: balanced order {one:.3f}, K-sorted order {worst:.3f} (worst shift)")
        assert worst <= 1.10


def _single_start_share(tm, tn, kr, kc, shift=0):
    """share of the tiles that run beside tiles of their own K start only: the block ids of an XCD, in rising order, 64 at a time (the
    workgroups it holds at once when they start and finish together)"""
    start = np.maximum(kr[tm], kc[tn])
    good = 0
    for x in range(XCDS):
        mine = np.flatnonzero((np.arange(tm.size) + shift) % XCDS == x)
        for lo in range(0, mine.size, 64):
            s = start[mine[lo : lo + 64]]
            good += s.size if np.all(s == s[0]) else 0
    return good / tm.size


@pytest.mark.parametrize("shape", TILINGS)
def test_single_start_share_is_no_lower_than_the_balanced_order(hs, shape):
    tiles_m, tiles_n = shape
    for prof in PROFILES:
        kr, kc = _keys(tiles_m, prof), _keys(tiles_n, prof)
        s1 = _single_start_share(*_order01(hs, tiles_m, tiles_n, 1), kr, kc)
        s0 = _single_start_share(*_order01(hs, tiles_m, tiles_n, 0), kr, kc)
        tm, tn, _ = _order2(hs, tiles_m, tiles_n, kr, kc, 0)
        s2 = _single_start_share(tm, tn, kr, kc)
        print(f"[env phase order] {tiles_m} x {tiles_n} {prof}: single-start share: dense order {s0:.3f}, balanced {s1:.3f}, K-sorted {s2:.3f}")
        assert s2 >= s1


def test_constant_keys_walk_the_grid_unit_by_unit(hs):
    """a front without tables: the sorts are the identity, unit u is the 8 x 8 block (u // gn, u % gn) of the grid itself"""
    tiles_m, tiles_n = 24, 16
    z = np.zeros(24, dtype=np.int32)
    tm, tn, pos = _order2(hs, tiles_m, tiles_n, z, z[:16].copy(), 0)
    by_pos = np.argsort(pos)
    q = np.arange(64)
    for u in range(6):
        assert np.array_equal(tm[by_pos][64 * u : 64 * u + 64], 8 * (u // 2) + q % 8)
        assert np.array_equal(tn[by_pos][64 * u : 64 * u + 64], 8 * (u % 2) + q // 8)


def test_bad_arguments(hs):
    L = hs._lib.lib()
    buf = (C.c_int32 * 16)()
    assert L.hsk_env_phase_order(0, 2, buf, buf, 0, buf, buf, None) == -1
    assert L.hsk_env_phase_order(2, 513, buf, buf, 0, buf, buf, None) == -1
    assert L.hsk_env_phase_order(2, 2, None, buf, 0, buf, buf, None) == -1
    assert L.hsk_env_phase_order(2, 2, buf, buf, 8, buf, buf, None) == -1
    assert L.hsk_env_phase_order(2, 2, buf, buf, 0, buf, buf, None) == 0
