"""Selected inversion of compressed factorizations on the CPU: the rank-structured recurrence (tests/selinv_lr_mirror.py) over the oracle's
compressed tree (oracle/hs_oracle_lr.py) against the inverse that the same tree's solves define, O.ldiv(F, I), and against the dense-form
recurrence of tests/selinv_mirror.py on the same tree; and the new entry points of the C ABI.  The bound is 1e-10 * max|F^-1|, the one
tests/test_selinv_host.py uses; measured here <= 3.3e-14.  The device implementation is checked in tests/test_selinv_lr_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import selinv_lr_mirror as ML
import selinv_mirror as M
from helpers import prepare
from oracle import hs_oracle as O
from oracle import hs_oracle_lr as OL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    ("convdiff", (12, 12, 12), 100, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6)),
    ("convdiff_helmholtz", (12, 12, 12), 100, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6)),
    ("poisson", (16, 16, 16), 512, dict(swlevel=-1, atol=1e-4, rtol=1e-4)),
    ("helmholtz", (30, 27), 40, dict(swlevel=3, atol=1e-8, rtol=1e-8)),
]
_TREES = {}


def _tree(hs, kind, shape, nmax, kw):
    """(A, F, F^-1 by the tree's own solves), once per case."""
    key = (kind, shape, nmax, tuple(sorted(kw.items())))
    if key not in _TREES:
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        A = P["A"]
        F = OL.factor(A, P["ond"], P["ond_loc"], **kw)
        n = A.shape[0]
        cplx = np.iscomplexobj(A.data)
        Finv = O.ldiv(F, np.eye(n, dtype=np.complex128 if cplx else np.float64))
        _TREES[key] = (A, F, Finv)
    return _TREES[key]


@pytest.mark.parametrize("kind,shape,nmax,kw", CASES)
def test_rank_structured_mirror_against_the_trees_own_solves(hs, kind, shape, nmax, kw):
    A, F, Finv = _tree(hs, kind, shape, nmax, kw)
    n = A.shape[0]
    Z, lowrank, maxrank = ML.selinv_lr(F, n)
    assert lowrank > 0 and maxrank == OL.maxrank(F)
    r, c = A.nonzero()
    assert not np.isnan(Z[r, c]).any() and not np.isnan(Z[c, r]).any()  # every pattern entry and its transpose
    assert not np.isnan(np.diag(Z)).any()
    have = ~np.isnan(Z)
    scale = np.abs(Finv).max()
    err = np.abs(Z[have] - Finv[have]).max() / scale
    # the dense-form recurrence on the same tree: the same operator
    Zd = M.selinv(F, n)
    assert np.array_equal(np.isnan(Zd), ~have)
    errd = np.abs(Z[have] - Zd[have]).max() / scale
    lr, dn = ML.tree_flops(F)
    print(f"{kind} {shape}: {lowrank} low-rank fronts, max rank {maxrank}; error against ldiv(F, I) {err:.1e}, against the dense form {errd:.1e} "
          f"(* max|F^-1| = {scale:.2e}); flops rank-structured / dense form = {lr / dn:.2f}")
    assert err <= 1e-10 and errd <= 1e-10


def test_transforms_of_rank_zero(hs):
    """atol = 1e3 truncates every transform to rank 0: the flagged fronts decouple, Z[int, bnd] = Z[bnd, int] = 0, Z[int, int] = D^-1."""
    A, F, Finv = _tree(hs, "convdiff", (12, 12, 12), 100, dict(swlevel=2, swsize=8, atol=1e3, rtol=1e3))
    n = A.shape[0]
    assert OL.maxrank(F) == 0
    Z, lowrank, maxrank = ML.selinv_lr(F, n)
    assert lowrank > 0 and maxrank == 0
    have = ~np.isnan(Z)
    r, c = A.nonzero()
    assert have[r, c].all() and have[c, r].all()
    scale = np.abs(Finv).max()
    assert np.abs(Z[have] - Finv[have]).max() <= 1e-10 * scale
    assert np.abs(Z[have] - M.selinv(F, n)[have]).max() <= 1e-10 * scale


def test_flop_counts_of_the_two_forms():
    """The counts the device reports (hs_selinv_lr_info: flops, flops_dense_form) restated.  With one 256-block (ni <= 256) the dense form
    is 4 ni^3 + 6 ni^2 nb + 4 ni nb^2 real flops: Vb and the m x ni update are 2 ni nb^2 + 2 (ni + nb) ni nb, the back substitution
    multiplies [Vi | Vb] by the full inverse block, 2 ni^2 (ni + nb), the right substitution the m x ni block, 2 (ni + nb) ni^2.  The
    blocks are applied as full products, not triangles, so the count lies above 4/3 ni^3 + 4 ni^2 nb + 4 ni nb^2."""
    assert ML.dense_form_flops(200, 300) == 4 * 200 ** 3 + 6 * 200 ** 2 * 300 + 4 * 200 * 300 ** 2
    ni, nb = 360, 400
    d = ML.dense_form_flops(ni, nb)
    assert d >= 4 / 3 * ni ** 3 + 4 * ni * ni * nb + 4 * ni * nb * nb
    assert ML.dense_form_flops(ni, nb, cplx=True) == 4 * d
    assert ML.lr_form_flops(ni, nb, 86, 86) < 0.5 * d  # the issue's model: 0.44 at ranks 80-92
    assert ML.lr_form_flops(ni, nb, 200, 200) < d
    assert ML.lr_form_flops(ni, nb, 0, 0) < ML.lr_form_flops(ni, nb, 8, 8)
    assert ML.dense_form_flops(0, 5) == 0 and ML.dense_form_flops(7, 0) > 0


def test_new_entry_points_are_declared_exported_and_bound(hs):
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    lib = hs._lib.lib()
    for name in ("hs_selinv_lr", "hs_selinv_lr_info"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    for name in ("selinv_lr", "selinv_lr_diag", "selinv_lr_info"):
        assert callable(getattr(hs, name)), name
    out = (C.c_double * 8)()
    assert lib.hs_selinv_lr(None, 0, None, None, 0, 0, None) == hs._lib.HS_ERR_ARGUMENT
    assert lib.hs_selinv_lr_info(None, out) == hs._lib.HS_ERR_ARGUMENT
