"""hsk_env_tile_order -- which tile a block id of an enveloped plain update runs (csrc/kernels_gemm.hip: xcd_remap_shift, tile_coords,
env_order_stride; DESIGN.md section 4 "Branch fronts") -- on the host, no GPU.  Both orders must be bijections onto the tile grid (a
tile skipped is a block of the front left without its update, a tile row out of range a store outside the front); order 0 is the order
of the dense launches; and the balanced order must give every XCD about the same summed K length under the two-block cost of a branch
front, where the dense order leaves the first XCDs 20-33 % above the mean."""
import ctypes as C

import numpy as np
import pytest

XCDS = 8
BIG = [(95, 95), (128, 128), (256, 256), (127, 3), (1, 200), (200, 1), (9, 9), (20, 20)]


def _order(hs, tiles_m, tiles_n, order):
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


@pytest.mark.parametrize("order", [0, 1])
def test_bijection_small(hs, order):
    for tiles_m in range(1, 41):
        for tiles_n in range(1, 41):
            tm, tn = _order(hs, tiles_m, tiles_n, order)
            _assert_bijection(tm, tn, tiles_m, tiles_n, (tiles_m, tiles_n, order))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("shape", BIG)
def test_bijection_big(hs, shape, order):
    tm, tn = _order(hs, *shape, order)
    _assert_bijection(tm, tn, *shape, (shape, order))


def _parent_order(tiles_m, tiles_n):
    """xcd_remap + tile_coords restated: XCD x = bid & 7 owns a contiguous chunk of tile ids; tile ids walk groups of 8 tile rows, column
    after column inside a group"""
    nwg = tiles_m * tiles_n
    bid = np.arange(nwg, dtype=np.int64)
    q, r, x, o = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    t = np.where(x < r, x * (q + 1), r * (q + 1) + (x - r) * q) + o
    per_group = 8 * tiles_n
    g = t // per_group
    gm = np.minimum(tiles_m - 8 * g, 8)
    in_g = t - g * per_group
    return 8 * g + in_g % gm, in_g // gm


@pytest.mark.parametrize("shape", BIG + [(1, 1), (7, 13), (8, 8), (13, 7), (33, 40)])
def test_order_0_is_the_dense_order(hs, shape):
    tm, tn = _order(hs, *shape, 0)
    rm, rn = _parent_order(*shape)
    assert np.array_equal(tm, rm) and np.array_equal(tn, rn)


def test_at_most_8_tile_rows_and_columns_keep_the_dense_order(hs):
    for shape in [(8, 8), (3, 5), (1, 1), (8, 2)]:
        for a, b in zip(_order(hs, *shape, 1), _order(hs, *shape, 0)):
            assert np.array_equal(a, b), shape


def _heaviest_over_mean(tm, tn, n1):
    """Schur launch of a branch front whose child 1 holds the first n1 tile rows and columns: bnd1 x bnd1 runs all of K, every other tile
    half of it.  Blocks bid, bid + 8, ... share an XCD."""
    cost = np.where((tm < n1) & (tn < n1), 1.0, 0.5)
    per_xcd = np.bincount(np.arange(cost.size) & (XCDS - 1), weights=cost, minlength=XCDS)
    return per_xcd.max() / per_xcd.mean()


@pytest.mark.parametrize("T,n1", [(62, 31), (94, 47), (95, 47), (127, 63), (128, 64), (256, 128), (95, 32), (95, 63)])
def test_balance(hs, T, n1):
    new = _heaviest_over_mean(*_order(hs, T, T, 1), n1)
    old = _heaviest_over_mean(*_order(hs, T, T, 0), n1)
    print(f"[env tile order] T {T} n1 {n1}: heaviest XCD / mean: dense order {old:.3f}, balanced order {new:.3f}")
    assert new <= 1.10
    assert old >= 1.19


def test_bad_arguments(hs):
    L = hs._lib.lib()
    buf = (C.c_int32 * 4)()
    assert L.hsk_env_tile_order(0, 2, 1, buf, buf) == -1
    assert L.hsk_env_tile_order(2, -1, 1, buf, buf) == -1
    assert L.hsk_env_tile_order(2, 2, 1, None, buf) == -1
    assert L.hsk_env_tile_order(32769, 1, 1, buf, buf) == -1
