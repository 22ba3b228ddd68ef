"""The block solve on the CPU: the NumPy statement of its schedule (tests/ldiv_block_mirror.py) over the oracle's exact factorization
against SuperLU, and the new entry points of the C ABI.  The device implementation (csrc/hs_solve_multi.hip) is checked in
tests/test_ldiv_block_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import ldiv_block_mirror as M
from helpers import prepare, relerr
from oracle import hs_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a 2-D and a 3-D problem with fronts above 256 interior columns (ragged against 256), real and complex
PROBLEMS = [("convdiff", (30, 27), 450), ("convdiff_helmholtz", (30, 27), 450), ("convdiff", (18, 18, 18), 300)]


@pytest.mark.parametrize("lowrank", [False, True], ids=["dense", "lowrank"])
@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_mirror_of_the_schedule_matches_splu(hs, kind, shape, nmax, lowrank):
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    A = P["A"]
    n = A.shape[0]
    F = O.factor(A, P["ond"], P["ond_loc"], swlevel=0)
    levels = M.fronts_by_level(F, lowrank=lowrank)
    ni = [len(f.int) for fr in levels for f in fr]
    assert max(ni) > 256 and max(ni) % 256 != 0
    assert any(len(f.bnd) and f.lowrank is not None for fr in levels for f in fr) == lowrank
    lu = spla.splu(A)
    rng = np.random.default_rng(5)
    for k in (1, 17, 40):
        B = rng.standard_normal((n, k))
        if np.iscomplexobj(A.data):
            B = B + 1j * rng.standard_normal((n, k))
        X = M.ldiv_block(levels, B, kc=32)
        e = relerr(X, lu.solve(B))
        print(f"{kind} {shape} lowrank={lowrank} k={k}: {e:.2e}")
        assert e < 1e-11
    b = rng.standard_normal(n)
    assert M.ldiv_block(levels, b).shape == (n,)


def test_new_entry_points_are_declared_exported_and_bound(hs):
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    lib = hs._lib.lib()
    for name in ("hs_ldiv_block_d", "hs_ldiv_block_z", "hs_ldiv_block_dev_d", "hs_ldiv_block_dev_z", "hs_ldiv_block_info"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    assert callable(hs.ldiv_block) and callable(hs.ldiv_block_info)
    # argument errors need no device: a null handle is refused by every entry point
    b = np.zeros(4)
    pb = b.ctypes.data_as(hs._lib.p_f64)
    out = (C.c_double * 6)()
    for fn in (lib.hs_ldiv_block_d, lib.hs_ldiv_block_z):
        assert fn(None, 0, pb, 2, pb, 2, 2, 1) == hs._lib.HS_ERR_ARGUMENT
    for fn in (lib.hs_ldiv_block_dev_d, lib.hs_ldiv_block_dev_z):
        assert fn(None, 0, None, 2, None, 2, 2, 1, None) == hs._lib.HS_ERR_ARGUMENT
    assert lib.hs_ldiv_block_info(None, out) == hs._lib.HS_ERR_ARGUMENT
    assert np.all(b == 0)
