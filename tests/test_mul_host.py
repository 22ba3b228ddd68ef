"""The product with the stored factorization on the CPU: the NumPy statement of its schedule (tests/mul_mirror.py) over the oracle's exact
factors against op(A) X, its round trip with the block solve's mirror, and the new entry points of the C ABI (hs_mul_*, hs_mul_info,
hs_factor_error_*, hsk_multi_tri_*) on a null handle and on host-side plans.  The device implementation (csrc/hs_solve_multi.hip:
hs_mul_run, csrc/kernels_solve_multi_mul.hip, csrc/hs_mul.hip) is checked in tests/test_mul_gpu.py.

Round-trip bound: the block solve is backward stable, x = (F + dF)^-1 b with |dF| of the order of eps |F|, so F x - b = -dF x and
|F x - b| / |b| <= eps-order x cond(A).  n eps cond_1(A), cond_1 from numpy.linalg.cond on the dense 2-D matrix, is that bound with the
usual dimension factor; it is derived, not measured (measured here: 3.5e-15 on convdiff 30 x 27, 3.0e-11 on convdiff_helmholtz 30 x 27,
whose cond_1 is 4e6 -- a flat bound would be wrong)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ldiv_block_mirror as M
import mul_mirror as MM
from helpers import prepare, relerr
from oracle import hs_oracle as O
from test_ldiv_block_host import PROBLEMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
_CACHE = {}


def _levels(hs, kind, shape, nmax, lowrank):
    key = (kind, shape, nmax, lowrank)
    if key not in _CACHE:
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        F = O.factor(P["A"], P["ond"], P["ond_loc"], swlevel=0)
        _CACHE[key] = (P["A"], M.fronts_by_level(F, lowrank=lowrank))
    return _CACHE[key]


def _rand(rng, n, k, cplx):
    B = rng.standard_normal((n, k))
    return B + 1j * rng.standard_normal((n, k)) if cplx else B


@pytest.mark.parametrize("lowrank", [False, True], ids=["dense", "lowrank"])
@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_mirror_of_the_schedule_matches_the_matrix(hs, kind, shape, nmax, lowrank):
    A, levels = _levels(hs, kind, shape, nmax, lowrank)
    n = A.shape[0]
    ni = [len(f.int) for fr in levels for f in fr]
    assert max(ni) > 256 and max(ni) % 256 != 0
    assert any(len(f.bnd) and f.lowrank is not None for fr in levels for f in fr) == lowrank
    cplx = np.iscomplexobj(A.data)
    rng = np.random.default_rng(5)
    for trans in (0, 1, 2):
        Aop = MM.op_of(A, trans)
        for k in (1, 17, 40):
            X = _rand(rng, n, k, cplx)
            e = relerr(MM.mul(levels, X, trans=trans, kc=32), Aop @ X)
            print(f"{kind} {shape} lowrank={lowrank} trans={trans} k={k}: {e:.2e}")
            assert e < 1e-11
    x = rng.standard_normal(n)
    assert MM.mul(levels, x).shape == (n,)
    assert np.array_equal(MM.mul(levels, x, trans="T"), MM.mul(levels, x, trans=1))


@pytest.mark.parametrize("kind,shape,nmax", [p for p in PROBLEMS if len(p[1]) == 2])
def test_mirror_round_trip_with_the_block_solve(hs, kind, shape, nmax):
    A, levels = _levels(hs, kind, shape, nmax, False)
    n = A.shape[0]
    bound = n * EPS * float(np.real(np.linalg.cond(A.toarray(), 1)))
    rng = np.random.default_rng(6)
    B = _rand(rng, n, 40, np.iscomplexobj(A.data))
    R = MM.mul(levels, M.ldiv_block(levels, B, kc=32), trans=0, kc=32)
    worst = max(relerr(R[:, j], B[:, j]) for j in range(B.shape[1]))
    print(f"{kind} {shape}: mul(ldiv_block(B)) vs B, worst column {worst:.2e}, bound n eps cond_1 = {bound:.2e}")
    assert worst < bound


def test_new_entry_points_are_declared_exported_and_bound(hs):
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    ktxt = open(os.path.join(ROOT, "include", "hs_kernels.h")).read()
    lib = hs._lib.lib()
    for name in ("hs_mul_d", "hs_mul_z", "hs_mul_dev_d", "hs_mul_dev_z", "hs_mul_info", "hs_factor_error_d", "hs_factor_error_z"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    for name in ("hsk_multi_tri_d", "hsk_multi_tri_z", "hsk_multi_tri_t_d", "hsk_multi_tri_t_z"):
        assert re.search(r"\bint\s+%s\s*\(" % name, ktxt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    assert callable(hs.mul) and callable(hs.mul_info) and callable(hs.factor_error)
    # argument errors need no device: a null handle is refused by every entry point, outputs untouched
    b = np.zeros(4)
    pb = b.ctypes.data_as(hs._lib.p_f64)
    out = np.full(6, 7.0)
    po = out.ctypes.data_as(hs._lib.p_f64)
    for trans in (0, 1, 2):
        for fn in (lib.hs_mul_d, lib.hs_mul_z):
            assert fn(None, trans, pb, 2, pb, 2, 2, 1) == hs._lib.HS_ERR_ARGUMENT
            assert "hs_mul_*" in lib.hs_last_error().decode()
        for fn in (lib.hs_mul_dev_d, lib.hs_mul_dev_z):
            assert fn(None, trans, None, 2, None, 2, 2, 1, None) == hs._lib.HS_ERR_ARGUMENT
        for fn in (lib.hs_factor_error_d, lib.hs_factor_error_z):
            assert fn(None, trans, None, 0, 4, 0, 0, po) == hs._lib.HS_ERR_ARGUMENT
            assert "hs_factor_error_*" in lib.hs_last_error().decode()
    assert lib.hs_mul_info(None, po) == hs._lib.HS_ERR_ARGUMENT
    assert np.all(b == 0) and np.all(out == 7.0)
    # the hooks refuse bad arguments before they look for a device
    for fn in (lib.hsk_multi_tri_d, lib.hsk_multi_tri_z):
        assert fn(4, 4, 1, pb, 4, pb, 4, pb, 4, 0, 3, None) == hs._lib.HS_ERR_ARGUMENT  # tri outside 1, 2
        assert fn(4, 4, 65, pb, 4, pb, 4, pb, 4, 0, 1, None) == hs._lib.HS_ERR_ARGUMENT  # kc > 64
    for fn in (lib.hsk_multi_tri_t_d, lib.hsk_multi_tri_t_z):
        assert fn(4, 4, 1, pb, 4, pb, 4, pb, 4, 0, 0, 0, None) == hs._lib.HS_ERR_ARGUMENT
        assert fn(4, 4, 0, pb, 4, pb, 4, pb, 4, 0, 2, 0, None) == hs._lib.HS_ERR_ARGUMENT  # kc < 1
    # the Python layer refuses the factor objects that are out of scope without touching a handle
    for cls in (hs.ModifiedFactor, hs.DemotedFactor):
        obj = object.__new__(cls)
        obj._h = None
        for call in (lambda: hs.mul(obj, np.zeros(3)), lambda: hs.factor_error(obj), lambda: hs.mul_info(obj)):
            with pytest.raises(hs.UnsupportedError):
                call()
    with pytest.raises(TypeError):
        hs.mul(np.eye(3), np.zeros(3))


def _answer(hs, fn, h, trans, n):
    L = hs._lib.lib()
    b = np.full(n, 3.0)
    c = np.full(n, 5.0)
    st = fn(h, trans, c.ctypes.data_as(hs._lib.p_f64), n, b.ctypes.data_as(hs._lib.p_f64), n, n, 1)
    msg = L.hs_last_error().decode()
    word = next((w for w in ("ranks", "HSS", "not complete", "trans") if w in msg), None)
    assert np.all(c == 5.0) and np.all(b == 3.0)
    return st, word, msg


def test_plan_only_handles_are_refused_as_the_block_solve_refuses_them(hs):
    """On the host-side plans of tests/test_ldiv_transpose_host.py (`single`, `rank0of2`, `mf2`) hs_mul_d returns the status and the
    discriminating word hs_ldiv_block_t_d returns there, before any device work, and its message names hs_mul_*."""
    L = hs._lib.lib()
    P = prepare(hs, (20, 12), kind="convdiff", nmax=10)
    P3 = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512)
    handles = [
        ("single", P, dict()),
        ("rank0of2", P, dict(rank=0, nranks=2)),
        ("mf2", P3, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)),
    ]
    for hname, Pr, kw in handles:
        n = Pr["A"].shape[0]
        h = hs.dist.plan_only(Pr["A"], Pr["nd"], Pr["nd_loc"], **kw)
        try:
            for trans in (-1, 0, 1, 2, 3):
                st0, word0, _ = _answer(hs, L.hs_ldiv_block_t_d, h, trans, n)
                st, word, msg = _answer(hs, L.hs_mul_d, h, trans, n)
                assert (st, word) == (st0, word0), (hname, trans, st, word, st0, word0)
                assert st != 0 and "hs_mul_*" in msg, (hname, trans, msg)
            out = np.full(4, 7.0)
            assert L.hs_factor_error_d(h, 0, None, 0, 4, 0, 0, out.ctypes.data_as(hs._lib.p_f64)) == hs._lib.HS_ERR_ARGUMENT
            assert "hs_factor_error_*" in L.hs_last_error().decode() and "not complete" in L.hs_last_error().decode()
            assert np.all(out == 7.0)
            info = np.full(6, 7.0)
            assert L.hs_mul_info(h, info.ctypes.data_as(hs._lib.p_f64)) == 0 and np.all(info == 0.0)  # no product yet
        finally:
            L.hs_free(h)
