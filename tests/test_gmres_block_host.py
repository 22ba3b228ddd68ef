"""Lockstep GMRES on the CPU: the NumPy statement of its schedule (tests/gmres_block_mirror.py: freezing, per-column k_used, compaction,
groups) against a plain single-vector GMRES of the same iteration, column by column, and the new entry points of the C ABI.  The device
implementation (csrc/hs_gmres_block.hip) is checked in tests/test_gmres_block_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import gmres_block_mirror as M
from helpers import prepare, relerr
from oracle import hs_oracle as O, hs_oracle_lr as OL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The shapes of test_ldiv_block_host.py, real and complex.  The 2-D trees are cut deeper (nmax = 40) than there: with nmax = 450 they have two
# levels and boundaries of 27 DOFs, which the oracle's compression leaves exact.  Per problem the options of the loose compressed
# factorization (oracle/hs_oracle_lr.py), chosen so that the columns of `rhs_mix` need different numbers of iterations.
PROBLEMS = [
    ("convdiff", (30, 27), 40, dict(swlevel=4, swsize=4, atol=0.3, rtol=0.3)),
    ("convdiff_helmholtz", (30, 27), 40, dict(swlevel=3, swsize=4, atol=1e-2, rtol=1e-2)),
    ("convdiff", (18, 18, 18), 300, dict(swlevel=2, swsize=8, atol=0.1, rtol=0.1)),
]
NRHS = 9
RESTART, MAXITER = 5, 30


@pytest.mark.parametrize("prec", ["exact", "compressed", "none"])
@pytest.mark.parametrize("kind,shape,nmax,copts", PROBLEMS)
def test_mirror_of_the_lockstep_schedule_matches_single_vector_gmres(hs, kind, shape, nmax, copts, prec):
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    A = P["A"]
    n = A.shape[0]
    cplx = np.iscomplexobj(A.data)
    B = M.rhs_mix(n, NRHS, cplx, seed=1)
    reltol = 1e-8
    if prec == "exact":
        lu = spla.splu(A)
        apply = lu.solve
    elif prec == "compressed":
        F = OL.factor(A, P["ond"], P["ond_loc"], **copts)
        assert O.maxrank(F) > 0
        apply = lambda v: O.ldiv(F, v)  # noqa: E731
    else:
        apply = None
        # unpreconditioned GMRES(5) gets nowhere near 1e-8 in 30 iterations.  On the indefinite problem it stagnates: at 1e-2 every column
        # exhausts maxiter, at 0.3 the point sources finish within the first cycles and the constant vector never does
        reltol = 0.3 if kind == "convdiff_helmholtz" else 1e-2
    # The block preconditioner of the mirror has the property the device block solve has and a NumPy product on a block has not: a column
    # of the result does not depend on the other columns (BLAS sums a block and a vector in different orders, and restarted GMRES(5) on the
    # indefinite problem amplifies that rounding beyond 1e-10 within 30 iterations).  It is still ONE call per step.
    block = None if apply is None else (lambda Z: np.stack([apply(np.ascontiguousarray(Z[:, c])) for c in range(Z.shape[1])], axis=1))
    kw = dict(reltol=reltol, restart=RESTART, maxiter=MAXITER)
    single = [M.gmres_single(A, B[:, c], apply, **kw) for c in range(NRHS)]
    its = [ch["iters"] for _, ch in single]
    print(kind, shape, prec, "single-vector iterations:", its)
    # the reference itself must make the columns finish in different cycles: a spread of at least 2 over the non-zero columns and at least two
    # restart cycles.  Not asked of the exact preconditioner: every column takes one step by construction
    assert its[3] == 0 and single[3][1]["isconverged"] and not np.any(single[3][0])
    nz = [v for c, v in enumerate(its) if c != 3]
    if prec == "exact":
        assert max(nz) <= 2
    else:
        assert max(nz) - min(nz) >= 2 and max(nz) > RESTART, its
    for group in (None, 4):  # one group; groups of 4 columns (chunk width 4 in the mirror), the last one ragged
        st = {}
        X, chs = M.gmres_block(A, B, block, group=group, chunk=4 if group else 32, stats=st, **kw)
        assert st["groups"] == (1 if group is None else 3)
        for c in range(NRHS):
            xs, cs = single[c]
            assert chs[c]["iters"] == cs["iters"] and chs[c]["isconverged"] == cs["isconverged"], (c, chs[c]["iters"], cs["iters"])
            # rtol 1e-10 and nothing else: the mirror does a column's arithmetic with the very NumPy calls of `gmres_single`
            assert np.allclose(chs[c]["resnorm"], cs["resnorm"], rtol=1e-10, atol=0.0), (c, chs[c]["resnorm"], cs["resnorm"])
            assert relerr(X[:, c], xs) < 1e-10, (c, relerr(X[:, c], xs))
        if block is not None and group is None:
            # lockstep: one block application per step and per cycle end, never one per column
            assert st["prec_calls"] <= max(its) + st["cycles"] < sum(its)
            assert st["column_applications"] < st["prec_calls"] * NRHS  # the zero column never enters, finished columns leave
    # a vector is one column
    x, ch = M.gmres_block(A, B[:, 1], block, **kw)
    assert x.shape == (n,) and ch["iters"] == its[1]
    # an initial guess
    X0 = 0.5 * np.stack([s[0] for s in single], axis=1)
    Xg, chg = M.gmres_block(A, B, block, X0=X0, **kw)
    for c in (0, 3, 5):
        xs, cs = M.gmres_single(A, B[:, c], apply, x0=X0[:, c], **kw)
        assert chg[c]["iters"] == cs["iters"] and relerr(Xg[:, c], xs) < 1e-10


def test_new_entry_points_are_declared_exported_and_bound(hs):
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    lib = hs._lib.lib()
    for name in ("hs_gmres_block_d", "hs_gmres_block_z", "hs_gmres_block_info"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    assert callable(hs.gmres_block) and callable(hs.gmres_block_info)
    # argument errors need no device: a null B, X or iters is refused, and nothing is written
    n = 4
    colptr = np.arange(1, n + 2, dtype=np.int64)
    rowval = np.arange(1, n + 1, dtype=np.int64)
    pi = hs._lib.p_i64
    iters = np.full(2, 7, dtype=np.int64)
    conv = np.full(2, 7, dtype=np.int32)
    pc = conv.ctypes.data_as(C.POINTER(C.c_int))
    for fn, dt in ((lib.hs_gmres_block_d, np.float64), (lib.hs_gmres_block_z, np.complex128)):
        nz = np.ones(n, dtype=dt)
        B = np.ones((n, 2), dtype=dt, order="F")
        X = np.full((n, 2), 3.0, dtype=dt, order="F")
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        head = (None, n, colptr.ctypes.data_as(pi), rowval.ctypes.data_as(pi), vp(nz))
        tail = (2, 0, 0, 1e-8, 0.0, 5, 10, None)
        assert fn(*head, None, n, vp(X), n, *tail, iters.ctypes.data_as(pi), pc, None) == hs._lib.HS_ERR_ARGUMENT
        assert fn(*head, vp(B), n, None, n, *tail, iters.ctypes.data_as(pi), pc, None) == hs._lib.HS_ERR_ARGUMENT
        assert fn(*head, vp(B), n, vp(X), n, *tail, None, pc, None) == hs._lib.HS_ERR_ARGUMENT
        assert fn(*head, vp(B), n, vp(B), n, *tail, iters.ctypes.data_as(pi), pc, None) == hs._lib.HS_ERR_ARGUMENT  # X aliasing B
        assert fn(*head, vp(B), n - 1, vp(X), n, *tail, iters.ctypes.data_as(pi), pc, None) == hs._lib.HS_ERR_ARGUMENT
        assert fn(*head, vp(B), n, vp(X), n, 2, 2, 0, 1e-8, 0.0, 5, 10, None, iters.ctypes.data_as(pi), pc, None) == hs._lib.HS_ERR_ARGUMENT  # where
        assert fn(*head, vp(B), n, vp(X), n, 2, 0, 0, 1e-8, 0.0, 1000, 10, None, iters.ctypes.data_as(pi), pc, None) == hs._lib.HS_ERR_ARGUMENT  # restart
        assert b"restart" in lib.hs_last_error()
        assert fn(*head, None, n, None, n, 0, 0, 0, 1e-8, 0.0, 5, 10, None, None, None, None) == hs._lib.HS_OK  # nrhs = 0 touches nothing
        assert np.all(X == 3.0) and np.all(B == 1.0) and np.all(iters == 7) and np.all(conv == 7)
    assert lib.hs_gmres_block_info(None) == hs._lib.HS_ERR_ARGUMENT
    out = (C.c_double * 8)()
    assert lib.hs_gmres_block_info(out) == hs._lib.HS_OK
