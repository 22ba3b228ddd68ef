"""Solves with A + U V^H from the factors of A, on the CPU: the NumPy statement of the three identities (tests/mod_mirror.py) against
numpy.linalg.solve, the summation order of the inner-product kernel as a NumPy function, the new entry points of the C ABI and the argument
checks of the Python layer.  The device implementation (csrc/hs_mod.hip, csrc/kernels_mod.hip) is checked in tests/test_mod_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import mod_mirror as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(rng, shape, cplx):
    X = rng.standard_normal(shape)
    return X + 1j * rng.standard_normal(shape) if cplx else X


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("k", [0, 1, 5, 17])
def test_the_three_identities_match_a_dense_solve(k, cplx):
    n = 70
    rng = np.random.default_rng(10 * k + cplx)
    A = _rand(rng, (n, n), cplx) + 4.0 * np.sqrt(n) * np.eye(n)
    U = _rand(rng, (n, k), cplx)
    V = _rand(rng, (n, k), cplx)
    op = {"N": lambda M: M, "T": lambda M: M.T, "H": lambda M: M.conj().T}
    M = MM.Modified(lambda X, t: np.linalg.solve(op[t](A), X), U, V)
    A1 = A + U @ V.conj().T
    B = _rand(rng, (n, 7), cplx)
    for t in ("N", "T", "H"):
        X = M.ldiv(B, t)
        R = np.linalg.solve(op[t](A1), B)
        e = np.linalg.norm(X - R) / np.linalg.norm(R)
        cond = np.linalg.cond(M.C, 1) if k else 1.0
        print(f"k={k} cplx={cplx} trans={t}: {e:.2e} (cond_1(C) = {cond:.1e})")
        assert e < 1e-13 * max(cond, 1.0) * np.linalg.cond(A, 1)
    assert (M.W is not None) == (k > 0)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_mirror_of_the_inner_product_order(cplx):
    rng = np.random.default_rng(3)
    n, k, m = MM.SLAB + 37, 2, 2  # two slabs, the second partial and not a multiple of the step
    P = rng.integers(-3, 4, (n, k)).astype(float)
    Y = rng.integers(-3, 4, (n, m)).astype(float)
    if cplx:
        P = P + 1j * rng.integers(-3, 4, (n, k))
        Y = Y + 1j * rng.integers(-3, 4, (n, m))
    for conj in (False, True):  # integer data: every order gives the exact result
        ref = (P.T if conj else P.conj().T) @ Y
        assert np.array_equal(MM.inner(P, Y, conj), ref)
    P, Y = _rand(rng, (300, k), cplx), _rand(rng, (300, m), cplx)
    T = MM.inner(P, Y)
    assert np.allclose(T, P.conj().T @ Y, rtol=0, atol=1e-12)
    assert MM.fma(2.0**-30, 2.0**-30, 1.0) == 1.0 and MM.fma(1.0 + 2.0**-30, 1.0 + 2.0**-30, -1.0) == 2.0**-29 + 2.0**-60


NEW = ["hs_mod_create_d", "hs_mod_create_z", "hs_mod_create_dev_d", "hs_mod_create_dev_z", "hs_mod_create_sparse_d", "hs_mod_create_sparse_z", "hs_mod_ldiv_d",
       "hs_mod_ldiv_z", "hs_mod_ldiv_dev_d", "hs_mod_ldiv_dev_z", "hs_mod_info", "hs_gmres_block_mod_d", "hs_gmres_block_mod_z"]
HOOKS = ["hsk_mod_inner_d", "hsk_mod_inner_z", "hsk_mod_apply_d", "hsk_mod_apply_z", "hsk_mod_gather_d", "hsk_mod_gather_z", "hsk_mod_cap_d", "hsk_mod_cap_z"]


def test_new_entry_points_are_declared_exported_and_bound(hs):
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    ktxt = open(os.path.join(ROOT, "include", "hs_kernels.h")).read()
    lib = hs._lib.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    assert re.search(r"\bvoid\s+hs_mod_free\s*\(", txt) and "hs_mod_free" in hs._lib.EXPORTS and hasattr(lib, "hs_mod_free")
    for name in HOOKS:
        assert re.search(r"\bint\s+%s\s*\(" % name, ktxt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    # argument errors need no device: null handles and null objects are refused by every entry point
    h = C.c_void_p()
    b = np.zeros(4)
    pb = b.ctypes.data_as(hs._lib.p_f64)
    vb = b.ctypes.data_as(C.c_void_p)
    one = np.ones(3, dtype=np.int64).ctypes.data_as(hs._lib.p_i64)
    E = hs._lib.HS_ERR_ARGUMENT
    for sfx in ("_d", "_z"):
        assert getattr(lib, "hs_mod_create" + sfx)(None, 2, 1, vb, 2, vb, 2, C.byref(h)) == E and not h
        assert getattr(lib, "hs_mod_create_dev" + sfx)(None, 2, 1, None, 2, None, 2, None, C.byref(h)) == E
        assert getattr(lib, "hs_mod_create_sparse" + sfx)(None, 2, one, one, vb, C.byref(h)) == E
        assert getattr(lib, "hs_mod_ldiv" + sfx)(None, 0, pb, 2, pb, 2, 2, 1) == E
        assert getattr(lib, "hs_mod_ldiv_dev" + sfx)(None, 0, None, 2, None, 2, 2, 1, None) == E
        assert getattr(lib, "hs_gmres_block_mod" + sfx)(None, 0, 2, one, one, vb, vb, 2, vb, 2, 1, 0, 0, -1.0, 0.0, -1, 5, None, one, None, None) == E
    assert lib.hs_mod_info(None, pb) == E
    lib.hs_mod_free(None)
    assert np.all(b == 0)


def test_python_argument_checks_need_no_device(hs):
    assert callable(hs.modify) and callable(hs.ldiv_mod) and hs.ModifiedFactor is not None
    n = 70
    F = hs.FactorNode(None, np.float64, n, None)  # no handle: every check below comes before the library is called
    U = np.zeros((n, 3))
    with pytest.raises(TypeError):
        hs.modify(hs.transpose(F), U=U, V=U)
    with pytest.raises(ValueError, match="both U and V"):
        hs.modify(F, U=U)
    with pytest.raises(ValueError, match="both U and V"):
        hs.modify(F, V=U)
    with pytest.raises(ValueError, match="not both"):
        hs.modify(F, U=U, V=U, dA=sp.eye(n, format="csc"))
    with pytest.raises(hs.DimensionMismatch):
        hs.modify(F, U=np.zeros((n + 1, 3)), V=np.zeros((n + 1, 3)))
    with pytest.raises(hs.DimensionMismatch):
        hs.modify(F, U=U, V=np.zeros((n, 2)))
    with pytest.raises(hs.DimensionMismatch):
        hs.modify(F, dA=sp.eye(n + 1, format="csc"))
    with pytest.raises(TypeError):
        hs.modify(F, U=U.astype(complex), V=U)
    with pytest.raises(TypeError):
        hs.modify(F, dA=sp.eye(n, format="csc", dtype=complex))
    with pytest.raises(TypeError):
        hs.modify(F, dA=np.eye(n))
    M = hs.ModifiedFactor(None, F, 3)
    assert (M.n, M.k, M.dtype, M.shape) == (n, 3, np.dtype(np.float64), (n, n))
    with pytest.raises(TypeError):
        hs.ldiv_mod(F, np.zeros(n))
    with pytest.raises(ValueError, match="trans"):
        hs.ldiv_mod(M, np.zeros(n), trans="X")
    with pytest.raises(hs.DimensionMismatch):
        hs.ldiv_mod(M, np.zeros(n + 1))
    with pytest.raises(TypeError):
        hs.ldiv_mod(M, np.zeros(n, dtype=complex))
    with pytest.raises(TypeError):
        hs.ldiv_mod(M)
    with pytest.raises(ValueError, match="unmodified"):
        hs.gmres_block(None, np.zeros(n), Pr=M)
    with pytest.raises(ValueError, match="trans"):
        hs.gmres_block(sp.eye(n, format="csc"), np.zeros(n), Pr=M, trans="X")
