"""trsm_strip_kernel (kernels_trsm.hip) -- the 256-row TRSM base case X <- inv256L * X of a level in one launch, a workgroup per strip of
NS = 32 columns -- against the two half products on the GEMM tile it replaces (GemmOp::ainv 3 then 4) and against NumPy.

Every output element takes the same MFMA chain over the same k in the same order on either path, so the results must be EQUAL
(np.array_equal), and everything outside the block X[r0 : r0 + wl, c0 : c1) must be what it was.

Against float64 `inv @ X` the bound is componentwise: a sum of K <= 256 products accumulated in any order carries an error of at most
gamma_K (|inv| |X|), gamma_K = K u / (1 - K u), u = 2^-53 (Higham, Accuracy and Stability, section 3.1; the fused multiply-adds of the MFMA
only drop roundings).  The kernel and NumPy each stay inside it, so they differ by at most 2 gamma_256 (|inv| |X|): the constant is 2."""
import ctypes as C

import numpy as np
import pytest

from helpers import prepare

pytestmark = pytest.mark.gpu

P_F64 = C.POINTER(C.c_double)
P_I64 = C.POINTER(C.c_int64)
NS = 32
U = 2.0 ** -53
GAMMA = 2.0 * (256 * U / (1.0 - 256 * U))
BIG = 1 << 30


def make_inv(rng, wl):
    """a lower-triangular 256 x 256 block; NaN wherever no path may read a value that reaches a stored result: the rows and columns past
    wl and the block [0:128, 128:256] (rows 0..127 take k < 128 only)"""
    inv = np.tril(rng.standard_normal((256, 256)))
    inv[wl:, :] = np.nan
    inv[:, wl:] = np.nan
    inv[:128, 128:] = np.nan
    return inv


def trsm(hs, ni, nb, r0, c0, c1, inv, X, on, ldpad=0, shift=0, env=0):
    """the base case through hsk_trsm_inv_d; returns (list of X after, launches of the strip kernel, of the half products)"""
    L = hs._lib.lib()
    ni_a, nb_a = np.array(ni, dtype=np.int64), np.array(nb, dtype=np.int64)
    x = np.ascontiguousarray(np.concatenate([np.asfortranarray(v).ravel(order="F") for v in X]))
    iv = np.ascontiguousarray(np.concatenate([np.asfortranarray(v).ravel(order="F") for v in inv]))
    strips = C.c_int64(-1)
    prev = L.hsk_trsm_strip_enable(1 if on else 0)
    try:
        L.hsk_trsm_half_launches(1)
        hs._lib.check(L.hsk_trsm_inv_d(len(ni), ni_a.ctypes.data_as(P_I64), nb_a.ctypes.data_as(P_I64), r0, c0, c1, ldpad, shift,
                                       iv.ctypes.data_as(P_F64), x.ctypes.data_as(P_F64), env, C.byref(strips)))
        halves = L.hsk_trsm_half_launches(1)
    finally:
        L.hsk_trsm_strip_enable(prev)
    out, o = [], 0
    for a, b in zip(ni, nb):
        out.append(x[o:o + a * b].reshape((a, b), order="F"))
        o += a * b
    return out, strips.value, halves


def check_front(X0, Xon, Xoff, inv, ni, nb, r0, c0, c1, what):
    """on == off; outside the block untouched; inside within the bound of inv @ X"""
    assert np.array_equal(Xon, Xoff), (what, float(np.nanmax(np.abs(Xon - Xoff))))
    wl, ce = min(256, ni - r0), min(c1, nb)
    mask = np.zeros(X0.shape, dtype=bool)
    if wl > 0 and ce > c0:
        mask[r0:r0 + wl, c0:ce] = True
    assert np.array_equal(Xon[~mask], X0[~mask]), what
    if not mask.any():
        return 0.0
    B = X0[r0:r0 + wl, c0:ce]
    V = np.nan_to_num(inv[:wl, :wl], nan=0.0)  # (lower triangular: the NaN block above the diagonal stands for zeros nobody reads)
    want, bound = V @ B, GAMMA * (np.abs(V) @ np.abs(B))
    got = Xon[r0:r0 + wl, c0:ce]
    assert np.all(np.isfinite(got)), what
    err = np.abs(got - want)
    assert np.all(err <= bound), (what, float(np.max(err / np.maximum(bound, 1e-300))))
    return float(np.max(err / np.maximum(bound, 1e-300)))


@pytest.mark.parametrize("r0", [0, 256])
@pytest.mark.parametrize("wl", [1, 127, 128, 129, 255, 256])
def test_block_height_and_strip_sweep(hs, wl, r0):
    """wl: one row, either side of the half at 128, a ragged and a whole block; the column extent: one column, either side of a strip,
    two strips and a bit, many strips.  One front per launch, r0 = 0 and r0 = 256"""
    rng = np.random.default_rng(10 * wl + r0)
    worst = 0.0
    for N in (1, NS - 1, NS, NS + 1, 2 * NS + 5, 300):
        ni = r0 + wl
        inv, X0 = make_inv(rng, wl), rng.standard_normal((ni, N))
        (x1,), s1, h1 = trsm(hs, [ni], [N], r0, 0, BIG, [inv], [X0], True)
        (x0,), s0, h0 = trsm(hs, [ni], [N], r0, 0, BIG, [inv], [X0], False)
        assert (s1, h1, s0, h0) == (1, 0, 0, 2), (wl, N, s1, h1, s0, h0)
        worst = max(worst, check_front(X0, x1, x0, inv, ni, N, r0, 0, BIG, (wl, N, r0)))
    print(f"[trsm strip] wl={wl} r0={r0}: largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("c0,c1", [(0, BIG), (5, 200), (33, 64)])
def test_three_fronts_one_launch(hs, c0, c1):
    """fronts of their own ni and nb in one launch at r0 = 256: a ragged block, a whole one inside a larger front, and a front that ends
    before r0 and must be left alone; a column window that starts and ends inside strips"""
    rng = np.random.default_rng(c0 + 7)
    r0 = 256
    fronts = [(256 + 129, 70), (256 + 256 + 40, 300), (200, 50)]
    ni, nb = [f[0] for f in fronts], [f[1] for f in fronts]
    inv = [make_inv(rng, max(1, min(256, a - r0))) for a in ni]
    X0 = [rng.standard_normal(f) for f in fronts]
    x1, s1, h1 = trsm(hs, ni, nb, r0, c0, c1, inv, X0, True)
    x0, s0, h0 = trsm(hs, ni, nb, r0, c0, c1, inv, X0, False)
    assert (s1, h1, s0, h0) == (1, 0, 0, 2)
    for f in range(3):
        check_front(X0[f], x1[f], x0[f], inv[f], ni[f], nb[f], r0, c0, c1, (f, c0, c1))
    assert np.array_equal(x1[2], X0[2])


@pytest.mark.parametrize("ldpad,shift", [(1, 0), (0, 1), (1, 1), (3, 1)])
@pytest.mark.parametrize("ni", [256 + 255, 256 + 256, 256 + 77])
def test_unaligned_operands_run_natively(hs, ni, ldpad, shift):
    """an odd leading dimension and / or a base 8 bytes off a 16-byte boundary, with an odd and an even block height: the strip kernel takes
    them itself (its 16-byte loads need 8-byte alignment only) -- the counter says so"""
    rng = np.random.default_rng(ni + 10 * ldpad + shift)
    r0, N = 256, 2 * NS + 5
    inv, X0 = make_inv(rng, ni - r0), rng.standard_normal((ni, N))
    (x1,), s1, h1 = trsm(hs, [ni], [N], r0, 0, BIG, [inv], [X0], True, ldpad, shift)
    (x0,), s0, h0 = trsm(hs, [ni], [N], r0, 0, BIG, [inv], [X0], False, ldpad, shift)
    assert (s1, h1, s0, h0) == (1, 0, 0, 2)
    check_front(X0, x1, x0, inv, ni, N, r0, 0, BIG, (ni, ldpad, shift))


def test_enveloped_staircase(hs):
    """an enveloped launch: the columns of X carry a staircase of leading zeros per 32-column block, as the U12 of a leaf front does --
    strips that start their K loop late, strips whose first 128 rows are all zeros (not stored), strips that are zero over the whole
    block or over the whole front (not run), next to a dense front (no envelope clip at all when its columns are full)"""
    rng = np.random.default_rng(99)
    r0 = 256
    fronts = [(600, 330), (256 + 100, 70), (256 + 256, 64)]
    steps = [0, 9, 12, 16, 8, 20, 3, 17, 13, 11, 4]  # first non-zero row of a 32-column block, in units of 32 rows
    ni, nb = [f[0] for f in fronts], [f[1] for f in fronts]
    inv = [make_inv(rng, min(256, a - r0)) for a in ni]
    X0 = []
    for f, (a, b) in enumerate(fronts):
        x = rng.standard_normal((a, b))
        if f < 2:
            for c in range(b):
                x[:min(a, 32 * steps[(c // 32 + f) % len(steps)]), c] = 0.0
        X0.append(x)
    x1, s1, h1 = trsm(hs, ni, nb, r0, 0, BIG, inv, X0, True, env=1)
    x0, s0, h0 = trsm(hs, ni, nb, r0, 0, BIG, inv, X0, False, env=1)
    xd, sd, hd = trsm(hs, ni, nb, r0, 0, BIG, inv, X0, True, env=0)
    assert (s1, h1, s0, h0, sd, hd) == (1, 0, 0, 2, 1, 0)
    for f in range(3):
        check_front(X0[f], x1[f], x0[f], inv[f], ni[f], nb[f], r0, 0, BIG, ("env", f))
        assert np.array_equal(x1[f], xd[f]), f  # the clip leaves out exact zeros only


def test_end_to_end_on_equals_off(hs):
    """poisson3d_32, exact: solution and flop count are equal with the strip kernel on and off; with it on, no Float64 lower half product
    is left, and every strip launch stands for the pair of half products the run without it makes"""
    L = hs._lib.lib()
    P = prepare(hs, "poisson3d_32", rhs="randn")
    xs, flops, strips, halves = [], [], [], []
    for on in (1, 0):
        prev = L.hsk_trsm_strip_enable(on)
        try:
            L.hsk_trsm_strip_launches(1), L.hsk_trsm_half_launches(1)
            F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
            xs.append(hs.ldiv(F, P["b"]))
            strips.append(L.hsk_trsm_strip_launches(1)), halves.append(L.hsk_trsm_half_launches(1))
            flops.append(F.stats()["gemm_flops"])
            F.free()
        finally:
            L.hsk_trsm_strip_enable(prev)
    print(f"[trsm strip] poisson3d_32: on: strips {strips[0]} halves {halves[0]}   off: strips {strips[1]} halves {halves[1]}")
    assert strips[0] > 0 and halves[0] == 0
    assert strips[1] == 0 and halves[1] == 2 * strips[0]
    assert np.all(np.isfinite(xs[0]))
    assert np.array_equal(xs[0], xs[1])
    assert flops[0] == flops[1]
