"""Lockstep refined solves for a block of right-hand sides on the CPU: the NumPy statement of the schedule (tests/refine_block_mirror.py)
against a column-by-column loop of the single-column xGERFS and estimator mirrors, the new entry points of the C ABI, and the refusals a
host-side plan can name.  The device implementation (csrc/hs_refine_block.hip) is checked in tests/test_refine_block_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import normest_mirror as M
import refine_block_mirror as RB
from helpers import prepare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hs_ldiv_refine_block_d", "hs_ldiv_refine_block_z", "hs_ldiv_refine_block_dev_d", "hs_ldiv_refine_block_dev_z", "hs_ldiv_refine_block_info")


def _dense_solver(Ad):
    """An "F" with a fixed relative perturbation of 1e-6, whose columns do not depend on each other (one matrix-vector product per column):
    a single-column call and a block call return the same bits for a column."""
    rng = np.random.default_rng(7)
    Fd = Ad * (1.0 + 1e-6 * rng.standard_normal(Ad.shape))
    inv = {"N": np.linalg.inv(Fd), "T": np.linalg.inv(Fd.T), "C": np.linalg.inv(Fd.conj().T)}
    calls = []

    def solve(X, tr):
        calls.append(X.shape[1])
        return np.stack([inv[tr] @ X[:, j] for j in range(X.shape[1])], axis=1)

    return solve, calls


def _rhs(n, k, cplx, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    if cplx:
        B = B + 1j * rng.standard_normal((n, k))
    B[:, 2] = 0.0          # a zero column: berr = 1 by the safe1 guard, one correction
    B[:, 4] = B[:, 1]      # a copy
    return B


@pytest.mark.parametrize("trans", [0, 1, 2])
@pytest.mark.parametrize("kind", ["convdiff", "convdiff_helmholtz"])
def test_lockstep_mirror_equals_the_column_loop(hs, kind, trans):
    P = prepare(hs, (9, 9), kind=kind, nmax=10, rhs="randn")
    A = P["A"].tocsr()
    n = A.shape[0]
    cplx = np.iscomplexobj(A.data)
    opA = (A, A.T, A.conj().T)[trans].tocsr()
    nz = int(np.diff(opA.indptr).max()) + 1
    solve, calls = _dense_solver(A.toarray())
    nrhs = 7
    B = _rhs(n, nrhs, cplx, 3)
    Xs, bs, fs, ss = RB.refine_single(solve, opA, B, nz, trans=trans)
    assert ss.max() >= 1 and np.all(bs[[0, 1, 3, 5, 6]] <= 10 * np.finfo(float).eps)
    assert len(set(ss.tolist())) >= 2, ss  # columns freeze at different corrections: compaction is exercised
    ref = None
    for G in (None, 1, 2, nrhs):
        st = {}
        del calls[:]
        X, be, fe, steps = RB.refine_block(solve, opA, B, nz, trans=trans, group=G, chunk=4, stats=st)
        assert np.array_equal(steps, ss), (G, steps, ss)
        np.testing.assert_allclose(be, bs, rtol=1e-13, atol=0)
        np.testing.assert_allclose(fe, fs, rtol=1e-13, atol=0)
        np.testing.assert_allclose(X, Xs, rtol=0, atol=1e-13 * np.abs(Xs).max())
        assert np.array_equal(X[:, 4], X[:, 1]) and be[4] == be[1] and fe[4] == fe[1] and steps[4] == steps[1]
        assert fe[2] >= 0 and np.all(X[:, 2] == 0)
        # block applications of the refinement: the first solve and one per lockstep correction, per group
        width = G or nrhs
        want = sum(1 + steps[g0:g0 + width].max() for g0 in range(0, nrhs, width))
        assert st["refine_solves"] == want, (G, st, steps)
        assert st["groups"] == -(-nrhs // width) and st["max_active"] == min(width, nrhs)
        assert len(calls) == st["refine_solves"] + st["est_solves"] and sum(calls) == st["col_apps"]
        # the estimators share one application per half-step: far fewer applications than the loop's 2 per iteration and column
        assert st["est_solves"] <= 2 * (RB.EST_ITMAX + 1) * st["groups"]
        if ref is None:
            ref = (X, be, fe, steps)
        else:  # the group width changes nothing
            assert np.array_equal(X, ref[0]) and np.array_equal(be, ref[1]) and np.array_equal(fe, ref[2]) and np.array_equal(steps, ref[3])
    # a permutation and a subset of the columns give the same columns
    perm = np.array([5, 0, 3, 6, 1, 4, 2])
    Xp, bp, fp, sp_ = RB.refine_block(solve, opA, B[:, perm], nz, trans=trans, chunk=4)
    assert np.array_equal(Xp, ref[0][:, perm]) and np.array_equal(bp, ref[1][perm]) and np.array_equal(fp, ref[2][perm]) and np.array_equal(sp_, ref[3][perm])
    sub = [6, 2, 3]
    Xq, bq, fq, sq = RB.refine_block(solve, opA, B[:, sub], nz, trans=trans, group=2, chunk=4)
    assert np.array_equal(Xq, ref[0][:, sub]) and np.array_equal(bq, ref[1][sub]) and np.array_equal(fq, ref[2][sub]) and np.array_equal(sq, ref[3][sub])
    # without ferr and without corrections: the plain block solve
    X0, b0, f0, s0 = RB.refine_block(solve, opA, B, nz, trans=trans, itmax=0, ferr=False)
    assert f0 is None and np.all(s0 == 0) and np.array_equal(X0, solve(B, "NTC"[trans]))
    # ferr is an upper bound of the true forward error of the refined columns (dense inverse: the estimator's lower-bound slack is small)
    xt = np.linalg.solve(opA.toarray(), B)
    for c in (0, 1, 3, 5, 6):
        assert ref[2][c] >= np.abs(ref[0][:, c] - xt[:, c]).max() / M.cabs1(ref[0][:, c]).max()


def test_new_entry_points_are_declared_exported_and_bound(hs):
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    lib = hs._lib.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    assert callable(hs.ldiv_refine_block) and callable(hs.ldiv_refine_block_info)
    out = np.full(8, -1.0)
    assert lib.hs_ldiv_refine_block_info(out.ctypes.data_as(hs._lib.p_f64)) == 0 and np.all(out >= 0)
    assert lib.hs_ldiv_refine_block_info(None) == hs._lib.HS_ERR_ARGUMENT
    assert set(hs.ldiv_refine_block_info()) == {"seconds", "block_solves", "column_applications", "residual_launches", "max_active", "groups",
                                                "workspace_bytes", "estimator_column_applications"}


def test_refusals_need_no_device(hs):
    """Every refusal comes before any device work: a null handle and host-side plans (hs_plan) name them, and X stays untouched."""
    L = hs._lib.lib()
    f64, i64p = hs._lib.p_f64, hs._lib.p_i64
    P = prepare(hs, (20, 12), kind="convdiff", nmax=10)
    n = P["A"].shape[0]
    b = np.asfortranarray(np.ones((n, 2)))
    x = np.full((n, 2), 7.0, order="F")
    berr, ferr, steps = np.zeros(2), np.zeros(2), np.zeros(2, dtype=np.int64)
    pb, px = b.ctypes.data_as(f64), x.ctypes.data_as(f64)

    def call(h, fn=L.hs_ldiv_refine_block_d, trans=0, X=px, ldx=n, B=pb, ldb=n, nn=n, nrhs=2, itmax=5, be=berr.ctypes.data_as(f64), st=steps.ctypes.data_as(i64p)):
        return fn(h, trans, X, ldx, B, ldb, nn, nrhs, itmax, be, ferr.ctypes.data_as(f64), st)

    def call_dev(h, fn=L.hs_ldiv_refine_block_dev_d, trans=0, X=C.c_void_p(x.ctypes.data), B=C.c_void_p(b.ctypes.data), itmax=5):
        return fn(h, trans, X, n, B, n, n, 2, itmax, berr.ctypes.data_as(f64), ferr.ctypes.data_as(f64), steps.ctypes.data_as(i64p), None)

    ARG, DIM, UNS = hs._lib.HS_ERR_ARGUMENT, hs._lib.HS_ERR_DIMENSION, hs._lib.HS_ERR_UNSUPPORTED
    for fn in (L.hs_ldiv_refine_block_d, L.hs_ldiv_refine_block_z):
        assert call(None, fn) == ARG and b"null" in L.hs_last_error()
    for fn in (L.hs_ldiv_refine_block_dev_d, L.hs_ldiv_refine_block_dev_z):
        assert call_dev(None, fn) == ARG
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"])
    try:
        assert call(h, trans=3) == ARG and b"trans" in L.hs_last_error()
        assert call(h, trans=-1) == ARG
        assert call(h, itmax=-1) == ARG and b"itmax" in L.hs_last_error()
        assert call(h, L.hs_ldiv_refine_block_z) == ARG and b"MethodError" in L.hs_last_error()
        assert call(h, X=None) == ARG and b"NULL" in L.hs_last_error()
        assert call(h, B=None) == ARG and call(h, be=None) == ARG and call(h, st=None) == ARG
        assert call(h, X=pb) == ARG and b"alias" in L.hs_last_error()
        assert call_dev(h, X=C.c_void_p(b.ctypes.data + 8 * n)) == ARG and b"alias" in L.hs_last_error()  # X = the second column of B
        assert call(h, nn=n - 1) == DIM and call(h, ldx=n - 1) == DIM and call(h, ldb=n - 1) == DIM and call(h, nrhs=-1) == DIM
        # valid arguments: a plan holds no factors
        assert call(h) == ARG and b"plan" in L.hs_last_error()
        assert call_dev(h) == ARG and b"plan" in L.hs_last_error()
        assert call(h, nrhs=0) == ARG  # the handle is checked whatever nrhs is
    finally:
        L.hs_free(h)
    # what the block solve refuses: HS_ERR_UNSUPPORTED whatever trans is (ferr or not), and no fallback
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=2)
    try:
        for trans in (0, 1, 2):
            assert call(h, trans=trans) == UNS and b"ranks" in L.hs_last_error()
    finally:
        L.hs_free(h)
    P3 = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512)
    n3 = P3["A"].shape[0]
    b3 = np.ones(n3)
    x3 = np.full(n3, 7.0)
    h = hs.dist.plan_only(P3["A"], P3["nd"], P3["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    try:
        for trans in (0, 1, 2):
            for fe in (ferr.ctypes.data_as(f64), None):
                st = L.hs_ldiv_refine_block_d(h, trans, x3.ctypes.data_as(f64), n3, b3.ctypes.data_as(f64), n3, n3, 1, 5, berr.ctypes.data_as(f64), fe,
                                              steps.ctypes.data_as(i64p))
                assert st == UNS and b"HSS" in L.hs_last_error()
    finally:
        L.hs_free(h)
    assert np.all(x == 7.0) and np.all(x3 == 7.0) and np.all(b == 1.0)
