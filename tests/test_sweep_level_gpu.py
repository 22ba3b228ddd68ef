"""The sweep kernels of ldiv! -- kernels_solve_wide.hip (flow_sweep_kernel, fwd_wide / bwd_wide, wide_first), kernels_solve.hip (gather, the
32-column steps, the interior update, scatter), kernels_solve_t.hip (t_flow, t_diag / t_update, t_int_update, t_gather / t_scatter) -- one tree
level at a time through hsk_sweep_level_{d,z} (include/hs_kernels.h), held to the local recurrence of tests/sweep_mirror.py.

The hook factors a batch of fronts the way a level is factored (mode 2: the default optimistic path, mode 3: tournament pivoting), so the
stored inverses and their padding are the production ones, and runs the level's forward and backward sweeps on a global vector through
the per-level driver the level loops of ldiv! call (sweep_level_fwd / sweep_level_bwd, csrc/hs_sweep.h).  The batches sit on the tile edges of every implementation: HS_PB = 32,
HS_SW = 256, the dataflow tiles FB = 64 / 32 (transposed 32 / 16) rows, the tall boundary tiles FBB = 256 / 128 rows by CT = 64 columns,
UPD_CS = 512 and HS_TCH = 1024 boundary entries per chunk, and 1..4 column blocks for the odd and the even round counts.  Every entry of
every front is held to the mirror's bound or required bitwise unchanged (blank fronts, fronts without interior DOFs, the boundary of a
compressed front, the entries of b no front names)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sweep_mirror as sm
from lu_mirror import find_good_front, good_front

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPRESSED, BLANK = 1, 2

# (ni, nb, flags)
SMALL = [(1, 0, 0), (31, 1, 0), (32, 31, 0), (33, 63, 0), (63, 64, 0), (64, 65, 0), (65, 0, 0), (255, 129, 0), (256, 127, 0), (257, 255, 0),
         (300, 37, 0), (0, 37, 0), (256, 300, COMPRESSED), (128, 40, BLANK)]
LARGE = [(511, 256, 0), (512, 257, 0), (513, 511, 0), (769, 1025, 0), (1000, 513, 0), (600, 128, 0), (40, 1025, 0)]
SPECS = {"small": SMALL, "large": LARGE}

_batches = {}


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None


def make_batch(spec, cplx, seed):
    """Seeded Gaussian fronts (lu_mirror.good_front: the diagonal 32-blocks scaled so that optimistic pivoting succeeds and still swaps rows;
    beyond one 32-block find_good_front keeps only fronts whose largest multiplier stays below 3, so the growth flag of mode 2 stays down; no
    NaN anywhere -- all bits set is the sweeps' sentinel), disjoint random global ids out of about 1.3 times as many, a Gaussian b."""
    rng = np.random.default_rng(seed)
    sizes = [(ni, nb) for ni, nb, _ in spec]
    Fs = [find_good_front(rng, ni, nb, cplx)[0] if ni > 32 else good_front(rng, ni, nb, cplx) for ni, nb in sizes]
    n, ids = sm.make_ids(rng, sizes)
    b0 = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
    return dict(cplx=cplx, sizes=sizes, flags=[fl for _, _, fl in spec], Fs=Fs, n=n, ids=ids, b0=b0)


def batch(name, cplx):
    """Built once per (batch, type) and shared: nothing changes it."""
    if (name, cplx) not in _batches:
        _batches[(name, cplx)] = make_batch(SPECS[name], cplx, 100 + 2 * list(SPECS).index(name) + cplx)
    return _batches[(name, cplx)]


def run_hook(hs, B, mode, path, trans, tall=-1, fill=0.0, fidx=None, n=None):
    """One hsk_sweep_level call; returns (return code, raw output arrays)."""
    cplx = B["cplx"]
    dt = np.complex128 if cplx else np.float64
    ni = np.asarray([s[0] for s in B["sizes"]], dtype=np.int64)
    nb = np.asarray([s[1] for s in B["sizes"]], dtype=np.int64)
    m = ni + nb
    n = B["n"] if n is None else n
    Fp = np.concatenate([np.asarray(F, dtype=dt).ravel(order="F") for F in B["Fs"]])
    flags = np.asarray(B["flags"], dtype=np.int64)
    fidx = np.ascontiguousarray(np.concatenate(B["ids"]) if fidx is None else fidx, dtype=np.int64)
    b0 = np.ascontiguousarray(B["b0"], dtype=dt)
    n32 = (ni + 31) // 32 * 1024
    n256 = (ni + 255) // 256 * 65536
    raw = dict(LF=np.full(int((m * ni).sum()) + 1, fill, dtype=dt), UR=np.full(int((ni * nb).sum()) + 1, fill, dtype=dt),
               rperm=np.full(int(ni.sum()) + 1, int(fill), dtype=np.int64), info=np.full(len(ni), int(fill), dtype=np.int64),
               growth=np.full(len(ni), int(fill), dtype=np.int64),
               invL=np.full(int(n32.sum()) + 1, fill, dtype=dt), invU=np.full(int(n32.sum()) + 1, fill, dtype=dt),
               inv256L=np.full(int(n256.sum()) + 1, fill, dtype=dt), inv256U=np.full(int(n256.sum()) + 1, fill, dtype=dt),
               y=np.full(int(ni.sum()) + 1, fill, dtype=dt), b_fwd=np.full(n, fill, dtype=dt), x=np.full(int(ni.sum()) + 1, fill, dtype=dt),
               b_bwd=np.full(n, fill, dtype=dt))
    tall_used = C.c_int(-7)
    L = hs._lib.lib()
    fn = L.hsk_sweep_level_z if cplx else L.hsk_sweep_level_d
    rc = fn(len(ni), _pi(ni), _pi(nb), mode, _pd(Fp), _pi(flags), n, _pi(fidx), _pd(b0), path, trans, tall, _pd(raw["LF"]), _pd(raw["UR"]),
            _pi(raw["rperm"]), _pi(raw["info"]), _pi(raw["growth"]), _pd(raw["invL"]), _pd(raw["invU"]), _pd(raw["inv256L"]), _pd(raw["inv256U"]),
            _pd(raw["y"]), _pd(raw["b_fwd"]), _pd(raw["x"]), _pd(raw["b_bwd"]), C.byref(tall_used))
    raw["tall_used"] = np.asarray([tall_used.value], dtype=np.int64)
    return rc, raw


def assemble(B, raw):
    """(level, outputs) in the form sweep_mirror.check_level takes, from the packed arrays of the hook."""
    fronts, ys, xs = [], [], []
    o = dict(lf=0, ur=0, rp=0, i32=0, i256=0)
    for k, (ni, nb) in enumerate(B["sizes"]):
        m = ni + nb
        n32, n256 = (ni + 31) // 32 * 1024, (ni + 255) // 256 * 65536
        blocks = lambda a, off, cnt, bs: a[off:off + cnt].reshape((-1, bs, bs)).transpose(0, 2, 1)  # block: column-major bs x bs
        fronts.append(dict(ni=ni, nb=nb, fidx=B["ids"][k], LF=raw["LF"][o["lf"]:o["lf"] + m * ni].reshape((m, ni), order="F"),
                           UR=raw["UR"][o["ur"]:o["ur"] + ni * nb].reshape((ni, nb), order="F"), rperm=raw["rperm"][o["rp"]:o["rp"] + ni],
                           compressed=bool(B["flags"][k] & COMPRESSED), blank=bool(B["flags"][k] & BLANK),
                           inv={32: (blocks(raw["invL"], o["i32"], n32, 32), blocks(raw["invU"], o["i32"], n32, 32)),
                                256: (blocks(raw["inv256L"], o["i256"], n256, 256), blocks(raw["inv256U"], o["i256"], n256, 256))}))
        ys.append(raw["y"][o["rp"]:o["rp"] + ni])
        xs.append(raw["x"][o["rp"]:o["rp"] + ni])
        o["lf"] += m * ni; o["ur"] += ni * nb; o["rp"] += ni; o["i32"] += n32; o["i256"] += n256
    return dict(n=B["n"], b0=B["b0"], fronts=fronts), dict(y=ys, x=xs, b_fwd=raw["b_fwd"], b_bwd=raw["b_bwd"])


def check(hs, B, rc, raw, trans, path, what):
    """What every case asserts: the return code, info == 0 and growth == 0, the mirror's bound on y (z), the forward b[bnd] and x for every
    entry of every live front, and the bitwise conditions on everything else."""
    assert rc == 0, (what, rc, hs._lib.lib().hs_last_error())
    assert not raw["info"].any() and not raw["growth"].any(), (what, raw["info"], raw["growth"])
    level, out = assemble(B, raw)
    rep = sm.check_level(level, out, trans, 32 if path == 2 else 256)
    print(what, {k: "%.2e" % v for k, v in rep.worst.items()})
    rep.assert_ok(what)
    assert rep.entries == sm.covered_entries(level)
    return level, out


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("name", ["small", "large"])
def test_sweeps_n(hs, name, path, cplx):
    """ldiv!: dataflow (0), 256 columns per launch (1), 32 columns per launch on invL / invU (2: HS_SOLVE_FLOW=0 HS_SOLVE_WIDE=0)."""
    B = batch(name, cplx)
    rc, raw = run_hook(hs, B, 2, path, 0)
    check(hs, B, rc, raw, 0, path, ("N", name, path, cplx))
    assert raw["tall_used"][0] == 0  # neither batch reaches the rule's 1536 boundary blocks


@pytest.mark.parametrize("cplx,trans", [(False, 1), (True, 1), (True, 2)])
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("name", ["small", "large"])
def test_sweeps_t_and_h(hs, name, path, cplx, trans):
    B = batch(name, cplx)
    rc, raw = run_hook(hs, B, 2, path, trans)
    check(hs, B, rc, raw, trans, path, ("TH"[trans - 1], name, path, cplx))


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("tall", [1, 0])
@pytest.mark.parametrize("name", ["small", "large"])
def test_forward_dataflow_tall_and_short_boundary_tiles(hs, name, tall, cplx):
    """The tall boundary tiles (FBB rows x 64 columns per round, their own loads and reduction) at shapes of our choosing: boundary blocks of
    1, 31, 63 .. 1025 rows against FBB = 256 / 128, and 1 .. 16 rounds of 64 columns (odd and even counts, ragged last rounds)."""
    B = batch(name, cplx)
    rc, raw = run_hook(hs, B, 2, 0, 0, tall=tall)
    check(hs, B, rc, raw, 0, 0, ("tall", tall, name, cplx))
    assert raw["tall_used"][0] == tall


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("trans", [0, 1])
def test_tournament_pivots_reach_the_gather_and_scatter(hs, trans, cplx):
    """Factor mode 3 (a redone level): rows are swapped across whole panels, and the sweeps must follow rperm."""
    B = batch("small", cplx)
    rc, raw = run_hook(hs, B, 3, 0, trans)
    level, _ = check(hs, B, rc, raw, trans, 0, ("mode 3", trans, cplx))
    assert any(not np.array_equal(fr["rperm"], np.arange(fr["ni"])) for fr in level["fronts"])


def test_production_tall_rule(hs):
    """1536 fronts with boundary blocks: launch_fwd_flow takes the tall tiles by its own rule; one front fewer and it does not."""
    nis, nbs = (1, 2, 5, 17, 33, 64), (1, 3, 64, 65)
    spec = [(nis[k % 6], nbs[k % 4], 0) for k in range(1536)]
    B = make_batch(spec, False, 7)
    rule = hs._lib.lib().hsk_flow_tall_rule
    assert rule(0, 1536, 65) == 1 and rule(0, 1535, 65) == 0
    rc, raw = run_hook(hs, B, 2, 0, 0)
    check(hs, B, rc, raw, 0, 0, "1536 fronts")
    assert raw["tall_used"][0] == 1


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("trans", [0, 1])
def test_dataflow_sweeps_are_bitwise_reproducible(hs, trans, cplx):
    """DESIGN.md section 4a' and the header of kernels_solve_t.hip: no atomics on values, fixed reduction order -- the same call twice gives
    the same bits whatever order the workgroups ran in."""
    B = batch("small", cplx)
    rc1, r1 = run_hook(hs, B, 2, 0, trans)
    rc2, r2 = run_hook(hs, B, 2, 0, trans)
    assert rc1 == 0 and rc2 == 0
    for k in r1:
        assert np.array_equal(r1[k].view(np.uint64) if r1[k].dtype != np.int64 else r1[k],
                              r2[k].view(np.uint64) if r2[k].dtype != np.int64 else r2[k]), k
    check(hs, B, rc1, r1, trans, 0, ("twice", trans, cplx))


# ---- HS_SOLVE_FIRST=0 (read once per process): fwd_wide / bwd_wide compute the first block's product themselves -----------------------

_FIRST_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, hsamd
import test_sweep_level_gpu as T
hs = hsamd.load()
rc, raw = T.run_hook(hs, T.batch("small", False), 2, 1, 0)
assert rc == 0, rc
np.savez(%r, **raw)
print("FIRST OK")
"""


def test_wide_sweeps_without_the_first_block_kernel(hs, tmp_path):
    out = str(tmp_path / "first0.npz")
    code = _FIRST_CHILD % (ROOT, os.path.join(ROOT, "tests"), out)
    env = dict(os.environ, HS_SOLVE_FIRST="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FIRST OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    with np.load(out) as z:
        raw = {k: z[k] for k in z.files}
    check(hs, batch("small", False), 0, raw, 0, 1, "HS_SOLVE_FIRST=0")


def test_hook_argument_checks(hs):
    """Every refusal comes before any device work and leaves the outputs alone."""
    B = make_batch([(5, 3, 0), (4, 0, 0)], False, 9)
    ids = np.concatenate(B["ids"])
    dup, low, high = ids.copy(), ids.copy(), ids.copy()
    dup[-1] = dup[0]
    low[3] = -1
    high[3] = B["n"]
    cases = [dict(path=3), dict(path=-1), dict(trans=3), dict(trans=-1), dict(tall=2), dict(tall=-2), dict(path=2, trans=1), dict(trans=2),
             dict(mode=1), dict(mode=4), dict(fidx=dup), dict(fidx=low), dict(fidx=high)]
    for kw in cases:
        a = dict(mode=2, path=0, trans=0, tall=-1, fidx=None)
        a.update(kw)
        rc, raw = run_hook(hs, B, a["mode"], a["path"], a["trans"], tall=a["tall"], fill=7.0, fidx=a["fidx"])
        assert rc != 0, kw
        assert raw["tall_used"][0] == -7, kw
        for k, v in raw.items():
            if k != "tall_used":
                assert (v == 7).all(), (kw, k)
    Bz = make_batch([(5, 3, 0)], True, 9)
    rc, raw = run_hook(hs, Bz, 2, 2, 2, fill=7.0)  # the 32-column sweeps have no adjoint either
    assert rc != 0 and (raw["x"] == 7).all()
    rc, raw = run_hook(hs, B, 2, 0, 0)
    check(hs, B, rc, raw, 0, 0, "accepted")
