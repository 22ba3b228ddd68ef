"""The transposed / adjoint block solve on the CPU: the NumPy statement of its schedule (tests/ldiv_block_t_mirror.py) over the oracle's
exact factorization against SuperLU's transposed and adjoint solves, and the new entry points of the C ABI.  The device implementation
(csrc/hs_solve_multi.hip, csrc/kernels_solve_multi_t.hip) is checked in tests/test_ldiv_block_t_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import ldiv_block_mirror as M
import ldiv_block_t_mirror as MT
from helpers import prepare, relerr
from oracle import hs_oracle as O
from test_ldiv_block_host import PROBLEMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("lowrank", [False, True], ids=["dense", "lowrank"])
@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_mirror_of_the_transposed_schedule_matches_splu(hs, kind, shape, nmax, lowrank):
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    A = P["A"]
    n = A.shape[0]
    assert abs(A - A.T).max() > 0  # unsymmetric: a solve in the wrong direction cannot pass
    F = O.factor(A, P["ond"], P["ond_loc"], swlevel=0)
    levels = M.fronts_by_level(F, lowrank=lowrank)
    assert all(isinstance(f, M.Front) for fr in levels for f in fr)
    ni = [len(f.int) for fr in levels for f in fr]
    assert max(ni) > 256 and max(ni) % 256 != 0
    assert any(len(f.bnd) and f.lowrank is not None for fr in levels for f in fr) == lowrank
    lu = spla.splu(A)
    rng = np.random.default_rng(5)
    for trans in ("T", "H"):
        for k in (1, 17, 40):
            B = rng.standard_normal((n, k))
            if np.iscomplexobj(A.data):
                B = B + 1j * rng.standard_normal((n, k))
            R = lu.solve(B, trans=trans)
            for left in (False, True):
                X = MT.ldiv_block_t(levels, B, trans=trans, kc=32, left=left)
                e = relerr(X, R)
                print(f"{kind} {shape} lowrank={lowrank} trans={trans} k={k} left={left}: {e:.2e}")
                assert e < 1e-11
            assert relerr(lu.solve(B), R) > 1e-3  # the forward solve is a different answer
    b = rng.standard_normal(n)
    assert MT.ldiv_block_t(levels, b).shape == (n,)


def test_new_entry_points_are_declared_exported_and_bound(hs):
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    ktxt = open(os.path.join(ROOT, "include", "hs_kernels.h")).read()
    lib = hs._lib.lib()
    for name in ("hs_ldiv_block_t_d", "hs_ldiv_block_t_z", "hs_ldiv_block_dev_t_d", "hs_ldiv_block_dev_t_z"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    for name in ("hsk_multi_prob_t_d", "hsk_multi_prob_t_z"):
        assert re.search(r"\bint\s+%s\s*\(" % name, ktxt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    assert callable(hs.ldiv_block_t)
    # argument errors need no device: a null handle is refused by every entry point, whatever trans is
    b = np.zeros(4)
    pb = b.ctypes.data_as(hs._lib.p_f64)
    for trans in (0, 1, 2):
        for fn in (lib.hs_ldiv_block_t_d, lib.hs_ldiv_block_t_z):
            assert fn(None, trans, pb, 2, pb, 2, 2, 1) == hs._lib.HS_ERR_ARGUMENT
        for fn in (lib.hs_ldiv_block_dev_t_d, lib.hs_ldiv_block_dev_t_z):
            assert fn(None, trans, None, 2, None, 2, 2, 1, None) == hs._lib.HS_ERR_ARGUMENT
    # the hooks refuse bad arguments before they look for a device
    for fn in (lib.hsk_multi_prob_t_d, lib.hsk_multi_prob_t_z):
        assert fn(0, 1, 1, pb, 1, pb, 1, pb, 1, 0, 0, 0, None) == hs._lib.HS_ERR_ARGUMENT
        assert fn(2, 2, 65, pb, 2, pb, 2, pb, 2, 0, 0, 0, None) == hs._lib.HS_ERR_ARGUMENT
    # ... and a row map with an entry outside its range: K entries in 0..K-1 (transposed), M entries in 0..M-1 (forward)
    for bad in ([0, 2], [-1, 0]):
        m = (C.c_int32 * 2)(*bad)
        for fn in (lib.hsk_multi_prob_t_d, lib.hsk_multi_prob_t_z):
            assert fn(1, 2, 1, pb, 2, pb, 2, pb, 1, 0, 0, 0, m) == hs._lib.HS_ERR_ARGUMENT
        for fn in (lib.hsk_multi_prob_d, lib.hsk_multi_prob_z):
            assert fn(2, 1, 1, pb, 2, pb, 1, pb, 2, 0, 0, m) == hs._lib.HS_ERR_ARGUMENT
    assert np.all(b == 0)
