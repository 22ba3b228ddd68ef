"""Log-determinant and selected inversion on the CPU: the NumPy statement of the recurrence (tests/selinv_mirror.py) over the oracle's exact
factorization against numpy.linalg.inv / slogdet, the rule that assigns every stored entry of A to a front, and the new entry points of
the C ABI.  The device implementation (csrc/hs_selinv.hip) is checked against the same dense references in tests/test_selinv_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import selinv_mirror as M
from helpers import prepare
from oracle import hs_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBLEMS = [
    ("poisson", (30, 27), 40), ("convdiff", (30, 27), 40), ("helmholtz", (30, 27), 40), ("convdiff_helmholtz", (30, 27), 40),
    ("convdiff", (12, 12, 12), 100), ("convdiff_helmholtz", (12, 12, 12), 100),
]


@pytest.mark.parametrize("kind,shape,nmax", PROBLEMS)
def test_mirror_against_dense_inverse_and_slogdet(hs, kind, shape, nmax):
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    A = P["A"]
    n = A.shape[0]
    F = O.factor(A, P["ond"], P["ond_loc"], swlevel=0)
    Ad = A.toarray()
    Zref = np.linalg.inv(Ad)
    Z = M.selinv(F, n)
    r, c = A.nonzero()
    assert not np.isnan(Z[r, c]).any() and not np.isnan(Z[c, r]).any()  # no pattern entry missing, Z_ij and Z_ji
    assert not np.isnan(np.diag(Z)).any()
    have = ~np.isnan(Z)
    err = np.abs(Z[have] - Zref[have]).max() / np.abs(Zref).max()
    print(f"{kind} {shape}: entries produced {have.sum()} of {n * n}, worst error {err:.1e} * max|A^-1|")
    assert err <= 1e-10
    la, sign = M.logabsdet(F)
    sref, lref = np.linalg.slogdet(Ad)
    assert abs(la - lref) <= 1e-11 * max(1.0, abs(lref))
    assert abs(sign - sref) <= 1e-10


def _graph_problem(hs, npts, nmax, seed):
    """A matrix built like `unstructured_problem` of tests/test_graph_nd.py, with its graph nested dissection."""
    from scipy.spatial import Delaunay

    rng = np.random.default_rng(seed)
    tri = Delaunay(rng.random((npts, 2))).simplices
    i = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    j = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    W = sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(npts, npts)).tocsr()
    W = ((W + W.T) > 0).astype(float)
    A = sp.csc_matrix(sp.diags(np.asarray(W.sum(axis=1)).ravel() + 0.1) - W)
    return A, hs.problems.graph_nested_dissection(A, nmax=nmax)


def test_every_stored_entry_has_exactly_one_owner(hs):
    """Grid and unstructured trees: every stored entry of A is owned by one front and lies inside that front's [int; bnd] block (the
    ownership is a function of the entry, so 'exactly once' is 'owner defined and entry inside')."""
    cases = []
    A, _, nd = hs.problems.make_problem((14, 13, 12), kind="convdiff", nmax=90, rhs="randn")
    cases.append((sp.csc_matrix(A), nd))
    cases.append(_graph_problem(hs, 1200, 60, 0))
    for A, nd in cases:
        nd, _ = hs.symfact(nd)
        fronts = M.fronts_of(nd)
        owner, inside = M.entry_owners(A, fronts)
        assert (owner >= 0).all() and inside.all(), (int((owner < 0).sum()), int((~inside).sum()))
        assert np.bincount(owner, minlength=len(fronts)).sum() == A.nnz


def test_an_entry_outside_every_front_is_reported(hs):
    """The rule must notice a pattern the tree does not cover: couple two DOFs that different leaves eliminate."""
    A, _, nd = hs.problems.make_problem((16, 16), kind="poisson", nmax=20, rhs="randn")
    nd, _ = hs.symfact(nd)
    fronts = M.fronts_of(nd)
    leaves = [f for f in fronts if len(f[0]) and f[2] == max(x[2] for x in fronts)]
    a, b = leaves[0][0][0], leaves[-1][0][0]
    B = sp.lil_matrix(A)
    B[a, b] = 1.0
    owner, inside = M.entry_owners(sp.csc_matrix(B), fronts)
    assert ((owner < 0) | ~inside).sum() == 1


def test_new_entry_points_are_declared_exported_and_bound(hs):
    txt = open(os.path.join(ROOT, "include", "hs_solver.h")).read()
    lib = hs._lib.lib()
    for name in ("hs_logabsdet", "hs_selinv", "hs_selinv_info"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in hs._lib.EXPORTS and hasattr(lib, name)
    for name in ("logabsdet", "logdet", "det", "selinv", "selinv_diag"):
        assert callable(getattr(hs, name)), name
    # argument errors need no device: a null handle is refused by every entry point
    la, sg, out = C.c_double(), (C.c_double * 2)(), (C.c_double * 4)()
    assert lib.hs_logabsdet(None, C.byref(la), sg) == hs._lib.HS_ERR_ARGUMENT
    assert lib.hs_selinv(None, 0, None, None, 0, 0, None) == hs._lib.HS_ERR_ARGUMENT
    assert lib.hs_selinv_info(None, out) == hs._lib.HS_ERR_ARGUMENT
