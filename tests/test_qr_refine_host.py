"""The mirror of the rank-revealing orthogonalisation (tests/qr_mirror.py) against independent references, and the conditions under which
tests/test_qr_refine_gpu.py may compare the device with it decision by decision -- all on the CPU:

  * with a window of one row, theta = 1 and no conditioning cut-off the norm-ordered mirror is a column-pivoted QR on gap inputs (residual
    norms a factor > sqrt(2) apart): it reproduces the order and the |R_jj| of scipy's qr(M^H, pivoting=True);
  * the float64 and the extended-precision run agree on every decision for every input of the GPU tests, the smallest decision margin of
    every such input is at least 1e-6, the designed ranks come out, and the scaled distances between the two precisions stay within the
    recorded MEASURED_D / MEASURED_T (the GPU tests allow the device 16 times those);
  * the mirror's T is the least-squares interpolation M[p_R] pinv(M[p_S]);
  * the selection is a stable partition."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import qr_mirror as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("hsk_qr_params", "hsk_qr_chol_d", "hsk_qr_chol_z", "hsk_qr_select", "hsk_qr_refine_d", "hsk_qr_refine_z")


def test_hooks_are_declared_exported_and_bound(hs):
    ktxt = open(os.path.join(ROOT, "include", "hs_kernels.h")).read()
    lib = hs._lib.lib()
    for name in HOOKS:
        assert re.search(r"\bint\s+%s\s*\(" % name, ktxt), name
        assert name in hs._lib.EXPORTS and getattr(lib, name).argtypes is not None
    P = Q.params(hs)
    assert P["W"] == 64 and 0.0 < P["cond"] < 1.0 and 0.0 < P["theta"] <= 1.0 and 0.0 < P["noise_rel"] < 1e-8
    # argument errors need no device
    E = hs._lib.HS_ERR_ARGUMENT
    assert lib.hsk_qr_params(None) == E
    assert lib.hsk_qr_select(1, None, None, None, None, None, None) == E
    for f in (lib.hsk_qr_chol_d, lib.hsk_qr_chol_z):
        assert f(1, *([None] * 12)) == E
    for f in (lib.hsk_qr_refine_d, lib.hsk_qr_refine_z):
        assert f(1, None, None, None, None, None, None, None, 0, 0.0, 0.0, 0.0, None, None, None, None, None, None, None) == E


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("lo", [1e-6, 1e-9])
def test_window_of_one_is_scipys_pivoted_qr(cplx, lo):
    """Gap inputs: every residual norm a factor > sqrt(2) above the next, so bucket 0 of the selection (within a factor 2 in norm^2 of the
    largest) holds one row and the window of one is the greedy choice.  The rows come in a random order."""
    import scipy.linalg as sla

    P1 = {"W": 1, "cond": 0.0, "theta": 1.0, "noise_rel": 0.0}
    m, q = 30, 41
    M = Q.lq_input(m, q, Q.graded(m, 1.0, lo), "weak", cplx, 3 + cplx)[np.random.default_rng(5).permutation(m)]
    R, piv = sla.qr(M.conj().T, mode="r", pivoting=True)
    dref = np.abs(np.diag(R))[:m]
    assert np.min(dref[:-1] / dref[1:]) > 1.5  # the order is unambiguous, for the selection's buckets too
    for prec in (np.float64, np.longdouble):
        out = Q.refine(M, np.arange(m), m, 0.0, 0.0, 0.0, P1, norm_select=True, prec=prec)
        assert out["r"] == m and out["windows"] == m and out["blocks"] == [(j, 1) for j in range(m)]
        assert list(out["p"]) == list(piv)
        assert np.max(np.abs(out["d"] - dref) / dref) < 1e-9
        assert abs(out["top"] - dref[0]) < 1e-12 * dref[0]


@pytest.fixture(scope="module")
def runs(hs):
    """Both precisions on every (case, order) of the GPU tests, once."""
    P = Q.params(hs)
    out = {}
    for cplx in (False, True):
        for c in Q.refine_cases(cplx):
            for o in c["orders"]:
                out[(cplx, c["name"], o)] = (c, Q.run_case(c, o, P), Q.run_case(c, o, P, np.longdouble))
    return out


def test_the_two_precisions_agree_on_every_decision_with_a_margin(runs):
    worst, wd, wt = (np.inf, None), 0.0, 0.0
    for key, (c, a, b) in runs.items():
        assert a["decisions"] == b["decisions"] and a["r"] == b["r"] and a["blocks"] == b["blocks"] and np.array_equal(a["p"], b["p"]), key
        assert (a["windows"], a["refreshes"]) == (b["windows"], b["refreshes"]), key
        if c["rank"] is not None:
            assert a["r"] == c["rank"], (key, a["r"])
        mg = min(a["margin"].min, b["margin"].min)
        assert mg >= 1e-6, (key, a["margin"].where, b["margin"].where)
        if mg < worst[0]:
            worst = (mg, key)
        dd, dt = Q.scaled_distances(c["M"], b, a["d"], a["T"])
        wd, wt = max(wd, dd), max(wt, dt)
    print(f"smallest decision margin {worst[0]:.2e} at {worst[1]}; float64 against extended: d {wd:.3e}, T {wt:.3e}")
    assert wd <= Q.MEASURED_D and wt <= Q.MEASURED_T, (wd, wt)
    assert Q.BOUND_D == 16 * Q.MEASURED_D and Q.BOUND_T == 16 * Q.MEASURED_T


def test_the_designed_cases_do_what_their_names_say(runs):
    g = lambda name, o, cplx=False: runs[(cplx, name, o)][2]
    for cplx in (False, True):
        assert g("refresh", 1, cplx)["refreshes"] >= 1
        for o in (0, 1):
            assert len(g("conditioning cut in one window", o, cplx)["blocks"]) >= 2
            w = g("second window accepts nothing", o, cplx)
            assert w["blocks"][-1][0] + w["blocks"][-1][1] == 64 and w["decisions"][-1][3] == 0
            z = g("zero matrix", o, cplx)
            assert z["r"] == 0 and z["top"] == 0.0 and z["windows"] == 1
            assert g("rmax = 0", o, cplx)["windows"] == 0
        # three chunks of the selection, and a selection that really re-orders
        assert any(d[0] == "window" and list(d[2]) != sorted(d[2]) for d in g("m700 strong", 1, cplx)["decisions"])


@pytest.mark.parametrize("cplx", [False, True])
def test_T_is_the_least_squares_interpolation(runs, cplx):
    n = 0
    for (cx, name, o), (c, a, b) in runs.items():
        r = b["r"]
        if cx != cplx or r == 0 or r == c["M"].shape[0]:
            continue
        Ms, Mr = c["M"][b["p"][:r]], c["M"][b["p"][r:]]
        cnd = np.linalg.cond(Ms)
        if cnd > 1e8:
            continue
        Tp = Mr @ np.linalg.pinv(Ms, rcond=1e-15)
        T = np.asarray(b["T"], dtype=Tp.dtype)
        # pinv in float64: eps * cond(M_S), a factor 64 for the sizes
        assert np.max(np.abs(T - Tp)) <= 64 * 2.3e-16 * cnd * max(1.0, np.max(np.abs(Tp))), (name, o, cnd)
        n += 1
    assert n >= 20


def test_chol_cases_have_a_margin_and_their_designed_counts(hs):
    P = Q.params(hs)
    for cplx in (False, True):
        for c in Q.chol_cases(cplx, P):
            ma, mb = Q.Margin(), Q.Margin()
            a, b = Q.run_chol_case(c, P, np.float64, ma), Q.run_chol_case(c, P, np.longdouble, mb)
            assert a["na"] == b["na"] and a["perm"] == b["perm"], c["name"]
            if c["nacc"] is not None:
                assert a["na"] == c["nacc"], (c["name"], a["na"])
            assert min(ma.min, mb.min) >= 1e-6, (c["name"], ma.where, mb.where)


def test_the_selection_of_the_mirror_is_a_stable_partition():
    for name, m, done, want, p0, res2 in Q.select_cases():
        p1, om = Q.select(p0, done, m, want, res2)
        Q.check_selection(name, m, done, want, p0, res2, np.asarray(p1), [float(om[0]), float(om[1])])
