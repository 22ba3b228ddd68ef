"""The look-ahead LU schedule (Sched::factor_fronts_lookahead, csrc/hs_sched.h) held to tests/lu_mirror.py, as production runs it.

Fronts with maxni >= 1536 (Float64, block columns of 1024) or >= 1200 (ComplexF64, block columns of 512) are eliminated block column by
block column on two streams: the main stream swaps, solves and updates with block column j while the side stream factors block column
j + 1, and the left swaps are applied once at the end.  tests/test_lu_paths_gpu.py stops at ni = 1000, so all of it runs the recursive
schedule; this file runs hsk_front_batch_{d,z} where the schedule looks ahead, and asserts with hsk_lookahead_runs that it did.

  a  production defaults, in process: two to four block columns, partial and one-column last block columns, lone fronts and mixed batches,
     modes 1 and 2, and Float64 in mode 2 | 4 (Sched::aligned16, the routing of the plain updates hs_numeric runs with)
  b  many short block columns (HS_LA_MIN=257 HS_LA_NB=256, read once per process: a child), down to a second block column of one column
  c  the growth flag by position across block columns: a planted multiplier of 8 raises it, 2.9 does not, a NaN does, huge Abi rows do not
  d  tournament pivoting under look-ahead (modes 0 and 3): backward errors, pivots taken from a later block column, info of singular fronts
  e  Float64: the direct-to-LDS routing and the strip TRSM change no bit of a whole elimination
  f  a look-ahead block below 256 with solve descriptors takes the recursive schedule, so the 256 x 256 inverses exist

Fronts are drawn with default_rng(7000 + 1000 * cplx + ni) and built once per process; nothing modifies them.  The bounds are those of
test_lu_paths_gpu.py (check_against_mirror: pivots exact, factors within 1e-12; check_inverses) and of test_tournament_with_descriptors /
front_check in test_kernels_gpu.py (1e-13 backward errors, Schur complement within 1e-13 max(cond, 10)).

The 1e-12 of check_against_mirror had only been met up to ni = 1000.  Measured on an MI355X for the lone fronts of part a, relative Frobenius
distance device <-> float64 mirror, largest over the modes: L 1.3e-14 (1537, 0), U 1.5e-15, Lbi 7.2e-14 (2049, 300); pivots equal
everywhere.  The bound holds with a factor of ten to spare, so no other reference was needed and none is used."""
import functools
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

from lu_mirror import find_good_front, optimistic_lu
from test_lu_paths_gpu import _plant, check_against_mirror, check_inverses, front_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LA_NB = {False: 1024, True: 512}  # the block columns of Sched::factor_fronts (Float64, ComplexF64)
ALIGNED = 4                       # bit 2 of hsk_front_batch's mode: Sched::aligned16


@functools.lru_cache(maxsize=None)
def big_front(ni, nb, cplx):
    """(F, mirror) of one front, built once per process and shared: callers must not modify either."""
    return find_good_front(np.random.default_rng(7000 + 1000 * cplx + ni), ni, nb, cplx)


def modes_of(cplx):
    return (1, 2) if cplx else (1, 2, 2 | ALIGNED)


def counted_batch(hs, Fs, nis, mode, inverses=False, expect=1):
    """front_batch, asserting that Sched::factor_fronts sent exactly `expect` batches to the look-ahead schedule."""
    L = hs._lib.lib()
    before = L.hsk_lookahead_runs(0)
    res = front_batch(hs, Fs, nis, mode, inverses=inverses)
    assert L.hsk_lookahead_runs(0) - before == expect, (mode, nis, L.hsk_lookahead_runs(0) - before, expect)
    return res


def check_shapes(hs, shapes, cplx, what):
    """Every mode on the fronts `shapes` in ONE call per mode: mirror, inverses (descriptor modes), look-ahead counter."""
    fronts = [big_front(ni, nb, cplx) for ni, nb in shapes]
    nis = [ni for ni, _ in shapes]
    for mode in modes_of(cplx):
        res = counted_batch(hs, [F for F, _ in fronts], nis, mode, inverses=bool(mode & 2))
        for (F, mir), r, (ni, nb) in zip(fronts, res, shapes):
            check_against_mirror(F, ni, r, mir, (what, mode, ni, nb, cplx))
            if mode & 2:
                check_inverses(r, (what, mode, ni, nb, cplx))
    assert all(np.any(mir["rperm"] != np.arange(ni)) for (_, mir), ni in zip(fronts, nis))  # every front pivots


# ---- a. production defaults, in process --------------------------------------------------------------------------------------------------

DEFAULT_SHAPES = [
    (False, 1536, 37),   # two block columns, 1024 + 512
    (False, 1537, 0),    # the second block column ends in a one-column group
    (False, 2049, 300),  # three block columns, the last one column wide
    (True, 1200, 37),    # block columns 512 + 512 + 176
    (True, 1537, 1),     # four block columns: reaches the ev_iter wait of the host
]
MIXED_SHAPES = {False: [(2049, 300), (700, 40), (1537, 0)], True: [(1537, 1), (500, 40), (1200, 37)]}


@pytest.mark.parametrize("cplx,ni,nb", DEFAULT_SHAPES)
def test_lookahead_matches_mirror(hs, cplx, ni, nb):
    """A lone front at the production switches (no environment set): modes 1, 2 and, Float64, 2 | 4."""
    check_shapes(hs, [(ni, nb)], cplx, "lone")


@pytest.mark.parametrize("cplx", [False, True])
def test_lookahead_mixed_batch(hs, cplx):
    """One call: the smaller fronts are clipped out of the later block columns, and every front keeps its own flag."""
    check_shapes(hs, MIXED_SHAPES[cplx], cplx, "mixed")


# ---- c (in process). a growth flag raised by a row in a later block column than its column ------------------------------------------------

# (row, column) per scalar type.  ComplexF64 (1200, 37), block columns of 512: the plants (899, 17) and (600, 300) of the child below have their
# rows in block column 1 and their columns in block column 0, and (1199, 17) is the last interior row.  Float64 (1537, 0), block columns of
# 1024: the same two plants lie inside block column 0, so they are joined by their images with the row in block column 1, the last interior
# row (1536, 17) and (1100, 300).
PLANTS_DEFAULT = {False: (1537, 0, [(899, 17), (600, 300), (1536, 17), (1100, 300)]), True: (1200, 37, [(899, 17), (600, 300), (1199, 17)])}


@pytest.mark.parametrize("cplx", [False, True])
def test_growth_flag_across_block_columns(hs, cplx):
    ni, nb, plants = PLANTS_DEFAULT[cplx]
    F0, mir0 = big_front(ni, nb, cplx)
    fronts = [F0] + [_plant(F0, mir0, row, col, 8.0) for row, col in plants]
    assert any(row // LA_NB[cplx] > col // LA_NB[cplx] for row, col in plants)
    for mode in (1, 2):
        res = counted_batch(hs, fronts, [ni] * len(fronts), mode)
        assert [r["growth"] for r in res] == [0] + [1] * len(plants), (mode, [r["growth"] for r in res])
        assert all(r["info"] == 0 for r in res)
        check_against_mirror(F0, ni, res[0], mir0, (mode, "clean"))


# ---- d. tournament pivoting under look-ahead -----------------------------------------------------------------------------------------------

def gaussian_front(rng, ni, nb, cplx):
    """Gaussian with a zero diagonal: the diagonal blocks alone do not suffice, the tournament must reach below them."""
    m = ni + nb
    F = rng.standard_normal((m, m)) + (1j * rng.standard_normal((m, m)) if cplx else 0)
    F[np.arange(ni), np.arange(ni)] = 0.0
    return F


def check_tournament(F, ni, r, nbcol, inverses, what):
    """The bounds of test_tournament_with_descriptors and front_check (test_kernels_gpu.py), and a pivot from a later block column."""
    nb = F.shape[0] - ni
    assert r["info"] == 0 and r["growth"] == 0, (what, r["info"], r["growth"])
    rp = r["rperm"]
    assert sorted(rp.tolist()) == list(range(ni)), what
    # a row that started in a later block column than the position it ended in: only the left swaps applied at the end put its multipliers right
    assert np.any(rp // nbcol > np.arange(ni) // nbcol), what
    lf = r["LF"]
    L = np.tril(lf[:ni], -1) + np.eye(ni)
    U = np.triu(lf[:ni])
    Aii, Aib, Abi, Abb = F[:ni, :ni], F[:ni, ni:], F[ni:, :ni], F[ni:, ni:]
    nrm = np.linalg.norm(F)
    e1 = np.linalg.norm(L @ U - Aii[rp]) / np.linalg.norm(Aii)
    assert e1 <= 1e-13, (what, "L U - P Aii", e1)
    if nb:
        e2 = np.linalg.norm(lf[ni:] @ U - Abi) / nrm
        e3 = np.linalg.norm(L @ r["UR"] - Aib[rp]) / nrm
        assert e2 <= 1e-13 and e3 <= 1e-13, (what, "Lbi U - Abi, L UR - P Aib", e2, e3)
        Sref = Abb - Abi @ np.linalg.solve(Aii, Aib)
        e4 = np.linalg.norm(r["SB"] - Sref) / np.linalg.norm(Sref)
        cond = np.linalg.cond(Aii)
        assert e4 <= 1e-13 * max(cond, 10.0), (what, "Schur", e4, cond)
    if inverses:
        check_inverses(r, what)


def run_tournament(hs, batches, cplx, nbcol, seed):
    """Modes 0 and 3 on every batch (a list of (ni, nb)) of Gaussian zero-diagonal fronts."""
    rng = np.random.default_rng(seed)
    for shapes in batches:
        Fs = [gaussian_front(rng, ni, nb, cplx) for ni, nb in shapes]
        nis = [ni for ni, _ in shapes]
        for mode in (0, 3):
            res = counted_batch(hs, Fs, nis, mode, inverses=(mode == 3))
            for F, r, (ni, nb) in zip(Fs, res, shapes):
                check_tournament(F, ni, r, nbcol, mode == 3, ("tournament", mode, ni, nb, cplx))


@pytest.mark.parametrize("cplx,ni,nb", [(False, 1537, 37), (True, 1200, 9)])
def test_tournament_under_lookahead(hs, cplx, ni, nb):
    """A lone front (the reserved-CU stream pair and, in these modes, the capped concurrent update) at the production block columns."""
    run_tournament(hs, [[(ni, nb)]], cplx, LA_NB[cplx], 7200 + cplx)


# ---- e. routing and strip switches change no bit -------------------------------------------------------------------------------------------

BIT_KEYS = ("LF", "UR", "SB", "rperm", "invL", "invU", "inv256L", "inv256U")
# (1537, 37) alone, the mixed batch of a, and small fronts on the recursive schedule: odd row offsets and K tails, hence edge-kernel launches
BIT_BATCHES = [([(1537, 37)], 1), (MIXED_SHAPES[False], 1), ([(257, 7), (513, 129), (1000, 1)], 0)]


def _bit_runs(hs, mode):
    out = []
    for shapes, la in BIT_BATCHES:
        fronts = [big_front(ni, nb, False) for ni, nb in shapes]
        res = counted_batch(hs, [F for F, _ in fronts], [ni for ni, _ in shapes], mode, inverses=True, expect=la)
        assert all(r["info"] == 0 and r["growth"] == 0 for r in res)
        out += res
    return out


def _assert_same_bits(a, b, what):
    for k, (ra, rb) in enumerate(zip(a, b)):
        for key in BIT_KEYS:
            assert np.array_equal(ra[key], rb[key]), (what, k, ra["ni"], key)


def test_gemm_routing_changes_no_bit(hs):
    """Mode 2 | 4 with the direct-to-LDS kernels on, the same with them off, and plain mode 2 (no aligned16: register-staged): whole
    eliminations equal bit for bit, and only the first sends launches to gemm_op_lds_kernel and the edge kernels."""
    L = hs._lib.lib()
    runs, lds, edge = [], [], []
    prev = L.hsk_gemm_lds_enable(1)
    try:
        for mode, on in ((2 | ALIGNED, 1), (2 | ALIGNED, 0), (2, 1)):
            L.hsk_gemm_lds_enable(on)
            L.hsk_gemm_lds_launches(1), L.hsk_gemm_lds_edge_launches(1)
            runs.append(_bit_runs(hs, mode))
            lds.append(L.hsk_gemm_lds_launches(1)), edge.append(L.hsk_gemm_lds_edge_launches(1))
    finally:
        L.hsk_gemm_lds_enable(prev)
    print(f"[lookahead routing] launches lds {lds} edge {edge}")
    assert lds[0] > 0 and edge[0] > 0 and lds[1:] == [0, 0] and edge[1:] == [0, 0], (lds, edge)
    _assert_same_bits(runs[0], runs[1], "lds on / off")
    _assert_same_bits(runs[0], runs[2], "aligned16 / plain")


def test_trsm_strip_changes_no_bit(hs):
    """The strip TRSM between block columns (LF and UR) against the two half products it replaces, over whole eliminations."""
    L = hs._lib.lib()
    runs, strips, halves = [], [], []
    prev = L.hsk_trsm_strip_enable(1)
    try:
        for on in (1, 0):
            L.hsk_trsm_strip_enable(on)
            L.hsk_trsm_strip_launches(1), L.hsk_trsm_half_launches(1)
            runs.append(_bit_runs(hs, 2 | ALIGNED))
            strips.append(L.hsk_trsm_strip_launches(1)), halves.append(L.hsk_trsm_half_launches(1))
    finally:
        L.hsk_trsm_strip_enable(prev)
    print(f"[lookahead strip] strips {strips} halves {halves}")
    assert strips[0] > 0 and halves[0] == 0 and strips[1] == 0 and halves[1] == 2 * strips[0], (strips, halves)
    _assert_same_bits(runs[0], runs[1], "strip on / off")


def test_aligned_bit_argument_checks(hs):
    """Modes 0..7 are hsk_front_batch's; hsk_sweep_level keeps refusing everything outside 2..3, the aligned bit included."""
    from test_lu_paths_gpu import _pd, _pi

    L = hs._lib.lib()
    ni = np.array([4], dtype=np.int64)
    nb = np.array([0], dtype=np.int64)
    F = np.eye(4)
    none = (None,) * 11
    for mode in (4, 7):
        assert L.hsk_front_batch_d(1, _pi(ni), _pi(nb), mode, _pd(F), *none) == 0
        assert L.hsk_front_batch_z(1, _pi(ni), _pi(nb), mode, _pd(np.eye(4, dtype=np.complex128)), *none) == 0
    for mode in (-1, 8, 12):
        assert L.hsk_front_batch_d(1, _pi(ni), _pi(nb), mode, _pd(F), *none) != 0
    inv = np.zeros(1024)
    assert L.hsk_front_batch_d(1, _pi(ni), _pi(nb), 1 | ALIGNED, _pd(F), None, None, None, None, None, None, _pd(inv), None, None, None, None) != 0
    fidx = np.arange(4, dtype=np.int64)
    b = np.ones(4)
    for mode in (1, 2 | ALIGNED, 3 | ALIGNED):
        assert L.hsk_sweep_level_d(1, _pi(ni), _pi(nb), mode, _pd(F), None, 4, _pi(fidx), _pd(b), 0, 0, -1, *((None,) * 14)) != 0


# ---- b, c, d in a child: many short block columns (HS_LA_MIN, HS_LA_NB are read once per process) -------------------------------------------

SHORT_NB = 256
SHORT_SHAPES = [(257, 300), (513, 1), (769, 37), (1000, 0), (1025, 300)]  # 257: a second block column of ONE column; 769: four block columns
                                                                         # and the host throttle; 1000: a partial last block column
PLANTS_8 = [(300, 17), (899, 17), (600, 300), (899, 600), (880, 800), (767, 255)]  # columns in block columns 0, 0, 1, 2, 3 (partial), 0; rows just
PLANTS_LOW = [(300, 31), (600, 287), (899, 767), (880, 831)]                       # below the group, in the next block column, the last interior row


def child_short_columns(hs, cplx):
    assert all(ni >= SHORT_NB + 1 for ni, _ in SHORT_SHAPES)
    for shape in SHORT_SHAPES:
        check_shapes(hs, [shape], cplx, "short")
    check_shapes(hs, [SHORT_SHAPES[4], SHORT_SHAPES[0], SHORT_SHAPES[2]], cplx, "short mixed")


def child_growth_flags(hs, cplx):
    """ni = 900 in block columns of 256: 0..255, 256..511, 512..767 and the partial 768..899."""
    ni, nb = 900, 20
    F0, mir0 = find_good_front(np.random.default_rng(7100 + cplx), ni, nb, cplx, lmax_max=2.0)
    fronts = [F0] + [_plant(F0, mir0, row, col, 8.0) for row, col in PLANTS_8]
    lows = []
    for row, col in PLANTS_LOW:
        G = _plant(F0, mir0, row, col, 2.9)
        mir = optimistic_lu(G, ni)
        assert 2.8 <= mir["lmax"] <= 3.0 and mir["gap"] >= 1e-10, (row, col, mir["lmax"], mir["gap"])
        fronts.append(G)
        lows.append((G, mir))
    expect = [0] + [1] * len(PLANTS_8) + [0] * len(PLANTS_LOW)
    # a NaN below the group of its column, in the last block column; huge entries in the Abi rows (rows >= ni) must not raise the flag
    nan_below = F0.copy()
    nan_below[880, 10] = np.nan
    abi = F0.copy()
    abi[ni + 3, 7] = 1e8
    abi[ni + nb - 1, 890] = -1e8
    mir_abi = optimistic_lu(abi, ni)
    assert not mir_abi["flag"]
    for mode in (1, 2):
        res = counted_batch(hs, fronts, [ni] * len(fronts), mode)
        got = [r["growth"] for r in res]
        assert got == expect, (mode, cplx, got)
        assert all(r["info"] == 0 for r in res)
        check_against_mirror(F0, ni, res[0], mir0, (mode, "clean"))
        for (G, mir), r in zip(lows, res[-len(lows):]):
            check_against_mirror(G, ni, r, mir, (mode, "planted 2.9"))
        res = counted_batch(hs, [nan_below, F0, abi], [ni] * 3, mode)
        assert [r["growth"] for r in res] == [1, 0, 0], (mode, cplx, [r["growth"] for r in res])
        check_against_mirror(F0, ni, res[1], mir0, (mode, "clean beside NaN"))
        check_against_mirror(abi, ni, res[2], mir_abi, (mode, "abi"))


def child_tournament(hs, cplx):
    run_tournament(hs, [[(769, 37)], [(1000, 0), (1025, 300), (257, 9)]], cplx, SHORT_NB, 7300 + cplx)
    # singular fronts: the FIRST exactly zero column k is reported as info = k + 1 -- k in block column 1, and in the (partial) last one
    rng = np.random.default_rng(7400 + cplx)
    sing = []
    for ni, nb, k in ((600, 10, 300), (1000, 8, 900)):
        F = gaussian_front(rng, ni, nb, cplx)
        F[:ni, k] = 0.0
        F[:ni, k + 3] = 0.0
        sing.append((F, ni, k))
    for mode in (0, 3):
        res = counted_batch(hs, [s[0] for s in sing], [s[1] for s in sing], mode)
        assert [r["info"] for r in res] == [k + 1 for _, _, k in sing], (mode, [r["info"] for r in res])


def child_small_block(hs, cplx):
    """HS_LA_NB = 128 with solve descriptors: no range of the look-ahead loop is 256 columns wide, so nothing in it would leave inv256L /
    inv256U behind.  Sched::factor_fronts sends such a batch to the recursive schedule (counter 0); without descriptors it looks ahead."""
    ni, nb = 600, 40
    F, mir = big_front(ni, nb, cplx)
    r = counted_batch(hs, [F], [ni], 2, inverses=True, expect=0)[0]
    check_against_mirror(F, ni, r, mir, ("small block", 2, cplx))
    check_inverses(r, ("small block", 2, cplx))
    r = counted_batch(hs, [F], [ni], 1, expect=1)[0]
    check_against_mirror(F, ni, r, mir, ("small block", 1, cplx))


CHILD_PARTS = {"short": child_short_columns, "growth": child_growth_flags, "tournament": child_tournament, "small": child_small_block}


def child_main(parts, cplx):
    """Runs in the child: every part on its own, one marker line each.  A part that fails reports and the next one still runs -- unless the
    failure is the device's, after which nothing more is started on it."""
    import hsamd

    hs = hsamd.load()
    L = hs._lib.lib()
    for part in parts:
        before = L.hsk_lookahead_runs(0)
        try:
            CHILD_PARTS[part](hs, cplx)
        except AssertionError:
            print(f"LOOKAHEAD {part} {int(cplx)} FAILED\n{traceback.format_exc()}", flush=True)
            continue
        except BaseException:
            print(f"LOOKAHEAD {part} {int(cplx)} ERROR\n{traceback.format_exc()}", flush=True)
            raise
        print(f"LOOKAHEAD {part} {int(cplx)} OK runs {L.hsk_lookahead_runs(0) - before}", flush=True)


_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_lu_lookahead_gpu as T
T.child_main(%r, %r)
"""


@functools.lru_cache(maxsize=None)
def _child_output(parts, cplx, la_min, la_nb):
    """One child per scalar type and pair of switches, shared by the tests that read its marker lines."""
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), parts, cplx)
    env = dict(os.environ, HS_LA_MIN=str(la_min), HS_LA_NB=str(la_nb))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    return r.returncode, r.stdout, r.stderr


def _assert_part(part, cplx, la_min, la_nb, parts):
    rc, out, err = _child_output(parts, cplx, la_min, la_nb)
    lines = [ln for ln in out.splitlines() if ln.startswith(f"LOOKAHEAD {part} {int(cplx)} OK runs ")]
    assert rc == 0 and len(lines) == 1, (rc, out[-4000:], err[-3000:])
    return int(lines[0].split()[-1])


SHORT_PARTS = ("short", "growth", "tournament")


@pytest.mark.parametrize("cplx", [False, True])
def test_short_block_columns_match_mirror(cplx):
    """b: block columns of 256 from ni = 257 on.  Every call of the part looked ahead (counted_batch); the total is what that adds up to."""
    runs = _assert_part("short", cplx, SHORT_NB + 1, SHORT_NB, SHORT_PARTS)
    assert runs == (len(SHORT_SHAPES) + 1) * len(modes_of(cplx)), runs


@pytest.mark.parametrize("cplx", [False, True])
def test_growth_flag_by_position_across_block_columns(cplx):
    """c: a multiplier of 8 raises the flag of its own front wherever its column's block column and its row lie; 2.9 does not."""
    assert _assert_part("growth", cplx, SHORT_NB + 1, SHORT_NB, SHORT_PARTS) == 4


@pytest.mark.parametrize("cplx", [False, True])
def test_tournament_short_block_columns(cplx):
    """d: modes 0 and 3, a lone front and a batch, and the info of singular fronts."""
    assert _assert_part("tournament", cplx, SHORT_NB + 1, SHORT_NB, SHORT_PARTS) == 6


@pytest.mark.parametrize("cplx", [False, True])
def test_lookahead_block_below_256_with_descriptors(cplx):
    """f: HS_LA_MIN=129 HS_LA_NB=128.  Mode 2 runs the recursive schedule and its stored inverses invert their blocks; mode 1 looks ahead."""
    assert _assert_part("small", cplx, 129, 128, ("small",)) == 1
