"""The determinant of a ULV-eliminated HSS matrix on the CPU: the formula hs_hss_logabsdet evaluates, restated in NumPy on the oracle's ULV
factors (oracle.hs_hss.rs_factor, the ones tests/ulv_t_mirror.py reads), against numpy.linalg.slogdet of the expanded matrix; and the new
entry points of the C ABI that need no device (hs_ulv_mode on a plan-only handle, the exports).  The device code is checked in
tests/test_ulv_det_gpu.py and tests/test_ulv_mode_gpu.py.

The formula: every non-root node replaces its local matrix M by X = E M F with E = [I -T; 0 I], F = [I 0; -T^T I] (unit triangular, so
det X = det M) after one symmetric permutation [R; S] of its rows and columns (det unchanged), and eliminates X_RR; what is left over all
levels is the root's block.  Hence det H = det(root LU) * prod over the eliminated nodes of det(X_RR), every factor the product of the
diagonal of a pivoted LU times the parity of its row exchanges.  A symmetric permutation of the whole matrix (H ~ A[perm][:, perm]) does
not change the determinant either."""
import ctypes as C

import numpy as np
import pytest

from helpers import prepare
from oracle import hs_hss as HS
from test_ulv_t_host import kernel_matrix


def lu_slogdet(lu_piv):
    """(sign, log|det|) of a matrix from scipy.linalg.lu_factor's output: the diagonal of U and the parity of the row exchanges."""
    lu, piv = lu_piv
    d = np.diag(lu)
    sign = np.prod(d / np.abs(d)) * (-1.0) ** int(np.count_nonzero(piv != np.arange(len(piv))))
    return sign, float(np.sum(np.log(np.abs(d))))


def ulv_slogdet(F):
    """The formula on the oracle's factors: the root's LU and the LU of X_RR of every node that eliminates something."""
    sign, la = lu_slogdet(F.root_lu)
    for i in sorted(F.lu):
        if F.lu[i] is not None:
            s, l = lu_slogdet(F.lu[i])
            sign, la = sign * s, la + l
    return sign, la


def check(Ho, complex_):
    # the comparison and the tolerance of _check_logabsdet in tests/test_selinv_gpu.py
    sref, lref = np.linalg.slogdet(HS.hss_full(Ho))
    sign, la = ulv_slogdet(HS.rs_factor(Ho))
    print(f"n={Ho.n} nodes={len(Ho.nodes)} complex={complex_}: log|det| {la:.12g} (ref {lref:.12g}), sign {sign} (ref {sref})")
    assert abs(la - lref) <= 1e-11 * max(1.0, abs(lref))
    assert abs(sign - sref) <= 1e-10
    assert np.iscomplexobj(sref) == complex_


@pytest.mark.parametrize("complex_", [False, True])
@pytest.mark.parametrize("n,leaf", [(70, 16), (500, 40)])
def test_formula_against_slogdet(n, leaf, complex_):
    Ho = HS.compress(kernel_matrix(n, complex_), leafsize=leaf, atol=1e-8, rtol=1e-8, kest=32)
    assert len(Ho.nodes) >= 3
    check(Ho, complex_)


@pytest.mark.parametrize("complex_", [False, True])
def test_formula_single_leaf_uneven_split_and_permuted(complex_):
    H1 = HS.compress(kernel_matrix(48, complex_), leafsize=64)
    assert len(H1.nodes) == 1
    check(H1, complex_)
    check(HS.compress(kernel_matrix(300, complex_), leafsize=50, atol=1e-8, rtol=1e-8, first_split=100), complex_)
    # H ~ A[perm][:, perm]: the determinant of A is that of the permuted matrix
    n = 300
    perm = np.random.default_rng(11).permutation(n)
    K = kernel_matrix(n, complex_)
    A = np.zeros_like(K)
    A[np.ix_(perm, perm)] = K
    Ho = HS.compress(A[perm][:, perm], leafsize=40, atol=1e-8, rtol=1e-8, kest=32)
    Ef = np.zeros_like(K)
    Ef[np.ix_(perm, perm)] = HS.hss_full(Ho)
    sref, lref = np.linalg.slogdet(Ef)
    sign, la = ulv_slogdet(HS.rs_factor(Ho))
    assert abs(la - lref) <= 1e-11 * max(1.0, abs(lref)) and abs(sign - sref) <= 1e-10


def test_a_negative_determinant_is_seen():
    """A real matrix with det < 0: the sign is not a by-product of diagonal dominance."""
    A = kernel_matrix(70)
    A[0] = -A[0]
    Ho = HS.compress(A, leafsize=16, atol=1e-10, rtol=1e-10, kest=32)
    sref, _ = np.linalg.slogdet(HS.hss_full(Ho))
    assert sref == -1.0
    check(Ho, False)


def test_exports_and_the_mode_switch_on_a_plan(hs):
    lib, E = hs._lib.lib(), hs._lib
    for name in ("hs_ulv_mode", "hs_hss_logabsdet", "hsk_ulv_det_d", "hsk_ulv_det_z"):
        assert name in E.EXPORTS and getattr(lib, name)
    assert callable(hs.ulv_mode) and callable(hs.hss.HssMatrix.logabsdet)
    # null arguments are refused without a device
    assert lib.hs_ulv_mode(None, 1) == E.HS_ERR_ARGUMENT and b"null" in lib.hs_last_error()
    la = C.c_double()
    assert lib.hs_hss_logabsdet(None, C.byref(la), C.byref(la), C.byref(la)) == E.HS_ERR_ARGUMENT
    # the mode is host state: a plan-only handle keeps it, over one rank or several
    P = prepare(hs, (12, 12), kind="convdiff", nmax=20, rhs="randn")
    for kw in ({}, {"rank": 0, "nranks": 2}):
        h = hs.dist.plan_only(P["A"], P["nd"], P["nd_loc"], **kw)
        try:
            assert lib.hs_ulv_mode(h, -1) == 0  # the default
            assert lib.hs_ulv_mode(h, 1) == 0 and lib.hs_ulv_mode(h, -1) == 1
            assert lib.hs_ulv_mode(h, 1) == 1  # setting it again returns the previous value
            for bad in (2, -2):
                assert lib.hs_ulv_mode(h, bad) == E.HS_ERR_ARGUMENT and lib.hs_ulv_mode(h, -1) == 1
            assert lib.hs_ulv_mode(h, 0) == 1 and lib.hs_ulv_mode(h, -1) == 0
        finally:
            lib.hs_free(h)
