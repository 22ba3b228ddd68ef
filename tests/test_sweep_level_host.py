"""tests/sweep_mirror.py guards itself (no GPU): a float64 NumPy implementation of one level's sweeps -- SciPy LU factors, NumPy inverses of the
diagonal blocks -- passes check_level for both block sizes, N / T / H, real and complex, and the same implementation with ONE planted defect
fails it.  The conditions on what the check leaves out live here too, and the one place that maps HS_SOLVE_FLOW / HS_SOLVE_WIDE to the
`path` of the sweeps (hs_sweep_path, csrc/hs_sweep.h)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sweep_mirror as sm

# (ni, nb): the shapes the bound was reasoned about, one front per ragged / full last block, and the descriptors without a bound
SIZES = [(300, 129), (769, 300), (0, 37), (33, 5), (1000, 513)]
SPECIAL = [(256, 300, "compressed"), (128, 40, "blank")]

_levels = {}


def level(cplx):
    if cplx not in _levels:
        rng = np.random.default_rng(20 + cplx)
        sizes = SIZES[:-1] + [(ni, nb) for ni, nb, _ in SPECIAL] + SIZES[-1:]  # the largest front last: the defects go there
        n, ids = sm.make_ids(rng, sizes)
        fronts = [sm.host_front(rng, ni, nb, cplx, ids[k]) for k, (ni, nb) in enumerate(sizes)]
        for k, (_, _, what) in enumerate(SPECIAL):
            fronts[len(SIZES) - 1 + k][what] = True
        b0 = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
        _levels[cplx] = dict(n=n, b0=b0, fronts=fronts)
    return _levels[cplx]


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("trans", [0, 1, 2])
@pytest.mark.parametrize("bs", [32, 256])
def test_float64_sweeps_pass_the_mirror(cplx, trans, bs):
    """Worst |got - mirror| / bound over the twelve cases, measured: 8.5e-4 (Float64, T, the forward z; N: 7.7e-4), ComplexF64 at most
    2.8e-4 -- the same for both block sizes to within a factor of two."""
    lv = level(cplx)
    out = sm.host_sweeps(lv, trans, bs)
    rep = sm.check_level(lv, out, trans, bs)
    print("clean", cplx, trans, bs, rep.worst)
    rep.assert_ok((cplx, trans, bs))
    assert rep.ratio() <= 0.05, rep.worst  # a float64 evaluation sits far inside a bound that is not fitted to it


DEFECTS = [("zero_entry", 0), ("zero_entry", 1), ("skip_column", 0), ("skip_column", 2), ("no_conj", 2), ("rperm_side", 0), ("rperm_side", 1)]
# (Float64 has no conjugate to miss)
DEFECT_CASES = [(d, t, bs, c) for d, t in DEFECTS for bs in (32, 256) for c in (False, True) if c or d != "no_conj"]


@pytest.mark.parametrize("defect,trans,bs,cplx", DEFECT_CASES)
def test_one_planted_defect_fails_the_mirror(defect, trans, bs, cplx):
    """Largest |got - mirror| / bound a defect leaves, the smallest over all cases, measured: 1.1e6 (one zeroed entry, Float64, N, 256-column
    blocks; the other zeroed entries 3.7e6 .. 5e8), a skipped column 1.1e9 .. 8.6e10, a missing conjugate 1.6e10, the permutation on the
    wrong side of the gather 6.6e11 .. 5.5e12; on the wrong side of the scatter it breaks b[fidx[rperm]] == x bitwise."""
    lv = level(cplx)
    out = sm.host_sweeps(lv, trans, bs, defect=defect)
    rep = sm.check_level(lv, out, trans, bs)
    print("defect", defect, cplx, trans, bs, rep.ratio(), rep.fails[:2])
    assert rep.fails, (defect, rep.worst)
    last = len(lv["fronts"]) - 1
    assert all(f[1] in (last, -1) for f in rep.fails), rep.fails  # the check is local: only the front with the defect fails
    finite = [f[3] for f in rep.fails if np.isfinite(f[3])]
    if defect in ("zero_entry", "skip_column", "no_conj"):
        assert finite and max(finite) >= 1e4, rep.fails  # far beyond the bound, not a near miss


def test_every_entry_is_bounded_or_bitwise():
    """Nothing is sampled or skipped: check_level holds 2 ni + nb entries of every live front to the bound (a compressed front: 2 ni, its
    boundary must stay bitwise), and the only fronts without a bound are the blank one and the one without interior DOFs -- which it
    requires bitwise unchanged, as it does every entry of b that no front names."""
    lv = level(False)
    out = sm.host_sweeps(lv, 0, 256)
    rep = sm.check_level(lv, out, 0, 256)
    live = [fr for fr in lv["fronts"] if fr["ni"] and not fr.get("blank")]
    assert rep.entries == sm.covered_entries(lv) == sum(2 * fr["ni"] + (0 if fr.get("compressed") else fr["nb"]) for fr in live)
    assert len(live) == len(lv["fronts"]) - 2
    used = np.concatenate([fr["fidx"] for fr in lv["fronts"]])
    unused = np.setdiff1d(np.arange(lv["n"]), used)
    assert unused.size > 0.2 * used.size
    comp = next(fr for fr in lv["fronts"] if fr.get("compressed"))
    blank = next(fr for fr in lv["fronts"] if fr.get("blank"))
    empty = next(fr for fr in lv["fronts"] if fr["ni"] == 0)
    for ids, what in ((unused[:1], "unused"), (blank["fidx"][:1], "blank interior"), (blank["fidx"][-1:], "blank boundary"),
                      (empty["fidx"][:1], "boundary of a front without interior"), (comp["fidx"][-1:], "compressed boundary")):
        for key in ("b_fwd", "b_bwd"):
            bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}
            bad[key][ids] = np.nextafter(bad[key][ids], np.inf)  # one ulp
            if key == "b_fwd":
                bad["b_bwd"][ids] = bad["b_fwd"][ids]
            r = sm.check_level(lv, bad, 0, 256)
            assert any(f[0] in ("fwd b elsewhere", "bwd b") for f in r.fails), (what, key, r.fails)
    # one ulp on an interior entry of b after the backward sweep breaks b[fidx[:ni]] == x bitwise
    bad = dict(out, b_bwd=out["b_bwd"].copy())
    i = live[0]["fidx"][:1]
    bad["b_bwd"][i] = np.nextafter(bad["b_bwd"][i], np.inf)
    assert any(f[0] == "bwd b" for f in sm.check_level(lv, bad, 0, 256).fails)
    # a NaN never passes
    bad = dict(out, y=[v.copy() for v in out["y"]])
    bad["y"][0][7] = np.nan
    assert sm.check_level(lv, bad, 0, 256).fails


# ---- hs_sweep_path: the switches are read once per process, so every setting is asked of a fresh child process ------------------------
# (the child loads the library alone, without the package: nothing here touches a device)
_PATH_CHILD = "import ctypes, sys; print('PATH', ctypes.CDLL(sys.argv[1]).hsk_sweep_path())"


@pytest.mark.parametrize("env,want", [({}, 0), ({"HS_SOLVE_FLOW": "0"}, 1), ({"HS_SOLVE_FLOW": "0", "HS_SOLVE_WIDE": "0"}, 2),
                                      ({"HS_SOLVE_WIDE": "0"}, 0)])
def test_sweep_path_from_the_environment(hs, env, want):
    """0: dataflow, whatever HS_SOLVE_WIDE says; HS_SOLVE_FLOW=0: 1 (256 columns per launch), with HS_SOLVE_WIDE=0 on top: 2 (32 columns)."""
    base = {k: v for k, v in os.environ.items() if k not in ("HS_SOLVE_FLOW", "HS_SOLVE_WIDE")}
    r = subprocess.run([sys.executable, "-c", _PATH_CHILD, hs._lib.LIB_PATH], env=dict(base, **env), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split() == ["PATH", str(want)], (env, r.returncode, r.stdout[-500:], r.stderr[-2000:])
