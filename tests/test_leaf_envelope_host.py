"""The block envelope of leaf fronts (csrc/hs_envelope.h), on the CPU.

1. The builder the analysis runs (reached through hsk_leaf_envelope) equals a NumPy computation from the pattern of A[idx][:, idx], for every
   leaf of four trees.
2. The rule the kernels rely on, in the reference arithmetic alone (tests/lu_mirror.py): after the optimistic LU of a leaf front every entry
   of L, U, L21 = Abi U^-1 and U12 = L^-1 P Aib outside the 32-block envelope is exactly 0.0, and the Schur complement accumulated with the
   clipped sums (k ascending, a block pair starts at max(firstL[row block], firstU[column block])) equals the dense one bit for bit."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

from lu_mirror import optimistic_lu

G = 32
NONE = 1 << 30


def _prepare(hs, name_or_shape, **kw):
    A, b, nd = hs.problems.make_problem(name_or_shape, **kw)
    return _permute(hs, A, nd)


def _permute(hs, A, nd):
    nd, _ = hs.symfact(nd)
    perm = hs.postorder(nd)
    Ap = sp.csc_matrix(A[perm - 1][:, perm - 1])
    return Ap, hs.permuted(nd, hs.invperm(perm))


def _leaves(nd):
    out, stack = [], [nd]
    while stack:
        x = stack.pop()
        if x.left is None and x.right is None:
            out.append(x)
        else:
            stack += [c for c in (x.left, x.right) if c is not None]
    return out


def _pattern(A):
    """Structural pattern of A (explicitly stored zeros count), as a 0/1 CSC matrix."""
    A = sp.csc_matrix(A)
    return sp.csc_matrix((np.ones(A.indices.size), A.indices, A.indptr), shape=A.shape)


def _blk(i, ni):
    i = np.asarray(i)
    return np.where(i < ni, i // G, (ni + G - 1) // G + (i - ni) // G)


def envelope_numpy(P, idx, ni):
    """firstL / firstU of the front A[idx][:, idx] (idx = [int; bnd], 0-based), from its dense boolean pattern."""
    m = len(idx)
    D = np.asarray(P[idx][:, idx].todense()) != 0
    D[np.arange(ni), np.arange(ni)] = True  # the diagonal counts as present
    nblk = (ni + G - 1) // G + (m - ni + G - 1) // G
    fL = np.full(nblk, NONE, dtype=np.int64)
    fU = np.full(nblk, NONE, dtype=np.int64)
    r, c = np.nonzero(D)
    kc = c < ni
    np.minimum.at(fL, _blk(r[kc], ni), c[kc] // G * G)
    kr = r < ni
    np.minimum.at(fU, _blk(c[kr], ni), r[kr] // G * G)
    return fL, fU


def envelope_library(hs, A, idx, ni):
    L = hs._lib.lib()
    A = sp.csc_matrix(A)
    n = A.shape[0]
    colptr = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rowval = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    fidx = np.ascontiguousarray(idx, dtype=np.int32)
    m = len(idx)
    nblk = (ni + G - 1) // G + (m - ni + G - 1) // G
    fL = np.full(nblk, -7, dtype=np.int32)
    fU = np.full(nblk, -7, dtype=np.int32)
    p64, p32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    rc = L.hsk_leaf_envelope(n, colptr.ctypes.data_as(p64), rowval.ctypes.data_as(p64), fidx.ctypes.data_as(p32), ni, m - ni,
                             fL.ctypes.data_as(p32), fU.ctypes.data_as(p32))
    assert rc == 0
    return fL.astype(np.int64), fU.astype(np.int64)


def _graph_problem(hs):
    from test_graph_nd import unstructured_problem

    A = unstructured_problem(3000, seed=5)
    return _permute(hs, A, hs.problems.graph_nested_dissection(A, nmax=150))


@pytest.mark.parametrize("name", ["poisson3d_32", "poisson3d_64", "helmholtz3d_32", "graph"])
def test_builder_equals_numpy_on_every_leaf(hs, name):
    Ap, nd = _graph_problem(hs) if name == "graph" else _prepare(hs, name)
    P = _pattern(Ap).tocsr()
    leaves = _leaves(nd)
    assert len(leaves) >= 8
    frac = []
    for x in leaves:
        it, bd = np.asarray(x.int) - 1, np.asarray(x.bnd) - 1
        idx = np.concatenate([it, bd])
        ni = len(it)
        fL, fU = envelope_library(hs, Ap, idx, ni)
        gL, gU = envelope_numpy(P, idx, ni)
        assert np.array_equal(fL, gL) and np.array_equal(fU, gU), (name, ni, len(bd))
        nbi = (ni + G - 1) // G
        assert np.array_equal(fL[:nbi], np.minimum(fL[:nbi], np.arange(nbi) * G))  # the diagonal block is inside
        frac.append(np.mean(np.minimum(fL, ni)) / max(ni, 1))
    if name.startswith("poisson3d_64"):
        assert np.mean(frac) > 0.25  # banded interior: the envelope is far from full


def test_builder_counts_stored_zeros_and_empty_blocks(hs):
    """Explicit zeros of A are structural; a boundary block without any coupling to the interior reports 'none'; bad arguments are refused."""
    n, ni = 200, 70
    rows = np.r_[np.arange(n), [5, 150, 69]]
    cols = np.r_[np.arange(n), [40, 3, 199]]
    vals = np.r_[np.ones(n), [0.0, 2.0, 0.0]]  # A[5, 40] and A[69, 199] are stored zeros
    A = sp.csc_matrix(sp.coo_matrix((vals, (rows, cols)), shape=(n, n)))
    assert A.nnz == n + 3
    idx = np.arange(n)
    fL, fU = envelope_library(hs, A, idx, ni)
    gL, gU = envelope_numpy(_pattern(A).tocsr(), idx, ni)
    assert np.array_equal(fL, gL) and np.array_equal(fU, gU)
    nbi = 3
    assert fU[1] == 0            # column 40 (block 1) has the stored zero in row 5
    assert fL[nbi + (150 - ni) // G] == 0 and fL[nbi] == NONE  # row 150 couples to column 3; rows 70..101 to nothing
    assert fU[nbi + (199 - ni) // G] == 64 and fU[nbi] == NONE
    L = hs._lib.lib()
    assert L.hsk_leaf_envelope(0, None, None, None, 1, 1, None, None) != 0


# ---- the rule itself ------------------------------------------------------------------------------------------------------------------------

def _check_rule(Ap, x, values, seed=0):
    it, bd = np.asarray(x.int) - 1, np.asarray(x.bnd) - 1
    idx = np.concatenate([it, bd])
    ni, nb = len(it), len(bd)
    m = ni + nb
    Fs = np.asarray(Ap[idx][:, idx].todense(), dtype=np.float64)
    P = Fs != 0
    if values == "random":  # the stencil alone never swaps a row: random values on the pattern do, inside the 32-row diagonal blocks
        F = np.where(P, np.random.default_rng(seed).standard_normal((m, m)), 0.0)
    else:
        F = Fs
    fL, fU = envelope_numpy(sp.csr_matrix(P), np.arange(m), ni)
    rowfirst = fL[_blk(np.arange(m), ni)]
    colfirst = fU[_blk(np.arange(m), ni)]
    mir = optimistic_lu(F, ni)
    assert not mir["bad"]
    swaps = int(np.count_nonzero(mir["rperm"] != np.arange(ni)))
    L, U, L21 = mir["L"], mir["U"], mir["Lbi"]
    U12 = sla.solve_triangular(L, F[:ni, ni:][mir["rperm"]], lower=True, unit_diagonal=True) if nb else np.zeros((ni, 0))
    k = np.arange(ni)
    outL = k[None, :] < rowfirst[:, None]   # (m x ni): columns left of the row block's first
    outU = k[:, None] < colfirst[None, :]   # (ni x m): rows above the column block's first
    assert np.count_nonzero(L[outL[:ni]]) == 0 and np.count_nonzero(L21[outL[ni:]]) == 0
    assert np.count_nonzero(U[outU[:, :ni]]) == 0 and np.count_nonzero(U12[outU[:, ni:]]) == 0
    if nb:
        Sd = F[ni:, ni:].copy()
        Sc = F[ni:, ni:].copy()
        rf, cf = rowfirst[ni:], colfirst[ni:]
        for kk in range(ni):
            Sd -= np.outer(L21[:, kk], U12[kk])
            r = np.flatnonzero(rf <= kk)
            c = np.flatnonzero(cf <= kk)
            if r.size and c.size:
                Sc[np.ix_(r, c)] -= np.outer(L21[r, kk], U12[kk, c])
        assert np.array_equal(Sd, Sc)
    outside = (outL.sum() + outU.sum()) / float(m * ni + ni * m)
    return swaps, outside


@pytest.mark.parametrize("values", ["stencil", "random"])
def test_rule_on_leaves_of_poisson3d_32(hs, values):
    Ap, nd = _prepare(hs, "poisson3d_32")
    leaves = _leaves(nd)
    total = 0
    for i, x in enumerate(leaves[:: max(1, len(leaves) // 6)]):
        swaps, _ = _check_rule(Ap, x, values, seed=i)
        total += swaps
    assert (total > 0) == (values == "random")


@pytest.mark.parametrize("values", ["stencil", "random"])
def test_rule_on_a_12_cubed_box(hs, values):
    Ap, nd = _prepare(hs, (24, 24, 24), kind="poisson", nmax=1728)
    x = _leaves(nd)[0]
    assert len(x.int) >= 1000
    swaps, outside = _check_rule(Ap, x, values, seed=1)
    assert (swaps > 100) == (values == "random")
    assert outside > 0.25  # a good part of the L / U rectangles of such a box lies outside the envelope (sanity: the check is not vacuous)
