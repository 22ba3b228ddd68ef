"""Float32-stored factors (hs_f32_*, csrc/hs_f32.hip) on the CPU: the new entry points of the C ABI and their bindings, the refusals that
need no device (null arguments, host-side plans), the argument checks of the Python layer, and the demotion rule as a NumPy mirror
(tests/f32_mirror.py).  The device implementation is checked in tests/test_f32_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import f32_mirror as FM
from helpers import prepare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["hs_f32_create", "hs_f32_ldiv_d", "hs_f32_ldiv_z", "hs_f32_ldiv_dev_d", "hs_f32_ldiv_dev_z", "hs_f32_info", "hs_gmres_block_f32_d", "hs_gmres_block_f32_z"]
HOOKS = ["hsk_multi_prob_f32_d", "hsk_multi_prob_f32_z", "hsk_multi_prob_t_f32_d", "hsk_multi_prob_t_f32_z", "hsk_round_factors_f32"]


def test_new_entry_points_are_declared_exported_and_bound(hs):
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    ktxt = open(os.path.join(ROOT, "include", "hs_kernels.h")).read()
    lib = hs._lib.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    assert re.search(r"\bvoid\s+hs_f32_free\s*\(", txt) and "hs_f32_free" in hs._lib.EXPORTS and hasattr(lib, "hs_f32_free")
    for name in HOOKS:
        assert re.search(r"\bint\s+%s\s*\(" % name, ktxt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)


def test_null_arguments_are_refused_by_every_entry_point(hs):
    lib = hs._lib.lib()
    E = hs._lib.HS_ERR_ARGUMENT
    h = C.c_void_p(77)
    b = np.zeros(4)
    pb = b.ctypes.data_as(hs._lib.p_f64)
    vb = b.ctypes.data_as(C.c_void_p)
    one = np.ones(3, dtype=np.int64).ctypes.data_as(hs._lib.p_i64)
    cnt = np.full(2, 42, dtype=np.int64)
    assert lib.hs_f32_create(None, None, C.byref(h)) == E and not h  # null handle: *G = NULL
    assert "null" in lib.hs_last_error().decode()
    assert lib.hs_f32_create(None, None, None) == E  # null output pointer
    for sfx in ("_d", "_z"):
        for trans in (0, 1, 2):
            assert getattr(lib, "hs_f32_ldiv" + sfx)(None, trans, pb, 2, pb, 2, 2, 1) == E
            assert getattr(lib, "hs_f32_ldiv_dev" + sfx)(None, trans, None, 2, None, 2, 2, 1, None) == E
            assert getattr(lib, "hs_gmres_block_f32" + sfx)(None, trans, 2, one, one, vb, vb, 2, vb, 2, 1, 0, 0, -1.0, 0.0, -1, 5, None, one, None, None) == E
        assert getattr(lib, "hs_f32_ldiv" + sfx)(None, 0, pb, 2, pb, 2, 2, 0) == E  # nrhs = 0 still checks
    assert lib.hs_f32_info(None, pb) == E
    assert lib.hsk_round_factors_f32(None, cnt.ctypes.data_as(hs._lib.p_i64)) == E
    lib.hs_f32_free(None)
    # the hooks refuse bad arguments before they look for a device
    for fn in (lib.hsk_multi_prob_f32_d, lib.hsk_multi_prob_f32_z):
        assert fn(0, 1, 1, pb, 1, pb, 1, pb, 1, 0, 0, None) == E
        assert fn(2, 2, 65, pb, 2, pb, 2, pb, 2, 0, 0, None) == E
    for fn in (lib.hsk_multi_prob_t_f32_d, lib.hsk_multi_prob_t_f32_z):
        assert fn(0, 1, 1, pb, 1, pb, 1, pb, 1, 0, 0, 0, None) == E
        assert fn(2, 2, 65, pb, 2, pb, 2, pb, 2, 0, 0, 0, None) == E
    assert np.all(b == 0) and np.all(cnt == 42)


def _create(hs, h):
    lib = hs._lib.lib()
    g = C.c_void_p(77)
    st = lib.hs_f32_create(h, None, C.byref(g))
    return st, lib.hs_last_error().decode(), g


def test_host_side_plans_are_refused_as_the_block_solve_refuses_them(hs):
    """A plan over two ranks and plans whose fronts keep D as an HSS matrix: HS_ERR_UNSUPPORTED naming the reason, as hs_ldiv_block_t_* names
    it on such a factorization (tests/test_ldiv_block_t_gpu.py); a plain plan: the status and the words of the zero-column block solve."""
    lib = hs._lib.lib()
    E = hs._lib
    P = prepare(hs, (20, 12), kind="convdiff", nmax=10)
    n = P["A"].shape[0]
    cnt = np.full(2, 42, dtype=np.int64)
    h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=2)
    try:
        st, msg, g = _create(hs, h)
        assert st == E.HS_ERR_UNSUPPORTED and "ranks" in msg and not g, (st, msg)
    finally:
        lib.hs_free(h)
    P3 = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512)
    for kw in (dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128), dict(swlevel=3, swsize=8, atol=1e-6, rtol=1e-6, mf=3, leafsize=128)):
        h = hs.dist.plan_only(P3["A"], P3["nd"], P3["nd_loc"], **kw)
        try:
            st, msg, g = _create(hs, h)
            assert st == E.HS_ERR_UNSUPPORTED and "HSS" in msg and not g, (kw, st, msg)
        finally:
            lib.hs_free(h)
    # a plan the block solve would serve once it is factored (hss_d is decided by the numeric phase: tests/test_f32_gpu.py): the probe speaks
    for PP, kw in ((P, dict()), (P3, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, hss_min=1024))):
        h = hs.dist.plan_only(PP["A"], PP["nd"], PP["nd_loc"], **kw)
        m = PP["A"].shape[0]
        try:
            want = lib.hs_ldiv_block_dev_t_d(h, 0, None, m, None, m, m, 0, None)
            wmsg = lib.hs_last_error().decode()
            st, msg, g = _create(hs, h)
            assert want != E.HS_OK and (st, msg) == (want, wmsg) and not g
            assert lib.hsk_round_factors_f32(h, cnt.ctypes.data_as(E.p_i64)) == want
        finally:
            lib.hs_free(h)
    assert np.all(cnt == 42) and n == 240


def test_python_argument_checks_need_no_device(hs):
    assert callable(hs.demote) and callable(hs.ldiv_f32) and hs.DemotedFactor is not None
    n = 70
    F = hs.FactorNode(None, np.float64, n, None)  # no handle: every check below comes before the library is called
    with pytest.raises(TypeError):
        hs.demote(hs.transpose(F))
    for bad in (None, 3, np.eye(3), hs.ModifiedFactor(None, F, 0)):
        with pytest.raises(TypeError):
            hs.demote(bad)
    G = hs.DemotedFactor(None, np.float64, n)
    assert (G.n, G.dtype, G.shape) == (n, np.dtype(np.float64), (n, n)) and "Float32" in repr(G)
    with hs.DemotedFactor(None, np.complex128, n) as Gz:
        assert Gz.dtype.kind == "c" and "ComplexF32" in repr(Gz)
    with pytest.raises(TypeError):
        hs.ldiv_f32(F, np.zeros(n))
    with pytest.raises(TypeError):
        hs.ldiv_f32(G)
    with pytest.raises(ValueError, match="trans"):
        hs.ldiv_f32(G, np.zeros(n), trans="X")
    with pytest.raises(hs.DimensionMismatch):
        hs.ldiv_f32(G, np.zeros(n + 1))
    with pytest.raises(hs.DimensionMismatch):
        hs.ldiv_f32(np.zeros(n), G, np.zeros((n - 1, 2)), trans="T")
    with pytest.raises(TypeError, match="MethodError"):
        hs.ldiv_f32(G, np.zeros(n, dtype=complex))
    with pytest.raises(ValueError, match="holds no matrix"):
        hs.gmres_block(None, np.zeros(n), Pr=G)
    with pytest.raises(ValueError, match="trans"):
        hs.gmres_block(sp.eye(n, format="csc"), np.zeros(n), Pr=G, trans="X")
    with pytest.raises(hs.DimensionMismatch):
        hs.gmres_block(sp.eye(n, format="csc"), np.zeros(n + 1), Pr=G)
    G.free()
    G.free()


def test_mirror_of_the_demotion_rule():
    fmax = FM.FLT_MAX
    big = fmax * (1.0 + 2.0**-24)  # 2^128 - 2^80: past the half-way point between FLT_MAX and 2^128
    half = fmax + 2.0**103  # the half-way point itself: the tie goes to the even mantissa, 2^128 = Inf
    assert fmax < half < big < 2.0**128
    x = np.array([big, -big, 1e39, 1e-46, 1e-40, 0.0, -0.0, fmax, np.nextafter(half, 0.0), 1.0 + 2.0**-24, 1.0 + 3 * 2.0**-24, FM.FLT_MIN, np.inf, np.nan, half])
    w, over, flush = FM.demote(x)
    assert over == 4 and flush == 2  # +-big, 1e39 and the tie; 1e-46 (zero) and 1e-40 (subnormal)
    assert np.isposinf(w[0]) and np.isneginf(w[1]) and np.isposinf(w[2])
    assert w[3] == 0.0 and 0.0 < w[4] < FM.FLT_MIN and w[4] == float(np.float32(1e-40))
    assert w[5] == 0.0 and not np.signbit(w[5]) and w[6] == 0.0 and np.signbit(w[6])
    assert w[7] == fmax and w[8] == fmax  # just below the tie: down
    assert np.isposinf(w[14])
    assert w[9] == 1.0 and w[10] == 1.0 + 2.0**-22  # ties to even, both ways
    assert w[11] == FM.FLT_MIN and np.isposinf(w[12]) and np.isnan(w[13])
    # real and imaginary parts separately
    z = np.array([1e39 + 1e-46j, (1.0 + 2.0**-24) + (1.0 + 3 * 2.0**-24) * 1j])
    wz, over, flush = FM.demote(z)
    assert over == 1 and flush == 1 and np.isposinf(wz[0].real) and wz[0].imag == 0.0 and wz[1] == 1.0 + (1.0 + 2.0**-22) * 1j
    rng = np.random.default_rng(5)
    a = rng.standard_normal((7, 5))
    assert np.array_equal(FM.rounded(a), a.astype(np.float32).astype(np.float64)) and FM.rounded(a).shape == a.shape
    assert np.abs(FM.rounded(a) - a).max() <= 2.0**-24 * np.abs(a).max()
