"""The block envelope of branch fronts (csrc/hs_envelope.h: hs_branch_envelope), on the CPU.

A branch front [int1; int2 | bnd1; bnd2] is assembled from the dense Schur complements of its two children, which own disjoint DOFs, and
from the entries of A across the cut.  Its structural pattern is therefore: every pair of positions of the same child, every stored entry
of A between the front's DOFs, and the interior diagonal.

1. The builder the analysis runs (reached through hsk_branch_envelope) equals a NumPy mirror written from that definition.
2. The rule the kernels rely on: unpivoted LU of the front assembled from the oracle's child S has exactly zero L / U outside the tables."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

from helpers import prepare
from oracle import hs_oracle as O
from test_leaf_envelope_host import G, NONE, _blk, _pattern

# ---- the mirror and the library ------------------------------------------------------------------------------------------------------------


def envelope_numpy(P, idx, ni, ni1, nb1):
    """firstL / firstU of the branch front on the DOFs idx = [int1; int2; bnd1; bnd2] (0-based), from its dense boolean pattern."""
    m = len(idx)
    p = np.arange(m)
    side = np.where(p < ni, p >= ni1, p - ni >= nb1)
    D = np.asarray(P[idx][:, idx].todense()) != 0          # the entries of A
    D |= side[:, None] == side[None, :]                    # the two dense Schur complements
    D[np.arange(ni), np.arange(ni)] = True                 # the interior diagonal
    nblk = (ni + G - 1) // G + (m - ni + G - 1) // G
    fL = np.full(nblk, NONE, dtype=np.int64)
    fU = np.full(nblk, NONE, dtype=np.int64)
    r, c = np.nonzero(D)
    kc = c < ni
    np.minimum.at(fL, _blk(r[kc], ni), c[kc] // G * G)
    kr = r < ni
    np.minimum.at(fU, _blk(c[kr], ni), r[kr] // G * G)
    return fL, fU


def envelope_library(hs, A, idx, ni, ni1, nb1):
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
    rc = L.hsk_branch_envelope(n, colptr.ctypes.data_as(p64), rowval.ctypes.data_as(p64), fidx.ctypes.data_as(p32), ni, m - ni, ni1, nb1,
                               fL.ctypes.data_as(p32), fU.ctypes.data_as(p32))
    assert rc == 0
    return fL.astype(np.int64), fU.astype(np.int64)


def _branches(nd):
    """(node, level) of every branch node, the root at level 1"""
    out, stack = [], [(nd, 1)]
    while stack:
        x, lv = stack.pop()
        if x.left is None and x.right is None:
            continue
        out.append((x, lv))
        stack += [(c, lv + 1) for c in (x.left, x.right) if c is not None]
    return out


def _front(x):
    """idx = [int; bnd] (0-based), ni, ni1, nb1 of a branch node after symfact: int = [left.bnd[loc.int]; right.bnd[loc.int]], bnd likewise"""
    it, bd = np.asarray(x.int) - 1, np.asarray(x.bnd) - 1
    lb = np.asarray(x.left.bnd) - 1
    i1, b1 = np.isin(it, lb), np.isin(bd, lb)
    ni1, nb1 = int(i1.sum()), int(b1.sum())
    assert i1[:ni1].all() and b1[:nb1].all()  # child 1 comes first
    return np.concatenate([it, bd]), len(it), ni1, nb1


@pytest.fixture(scope="module")
def p32(hs):
    return prepare(hs, "poisson3d_32", rhs="randn")


def _check_tree(hs, Ap, nd, min_branches):
    P = _pattern(Ap).tocsr()
    br = _branches(nd)
    assert len(br) >= min_branches
    for x, lv in br:
        idx, ni, ni1, nb1 = _front(x)
        fL, fU = envelope_library(hs, Ap, idx, ni, ni1, nb1)
        gL, gU = envelope_numpy(P, idx, ni, ni1, nb1)
        assert np.array_equal(fL, gL) and np.array_equal(fU, gU), (lv, ni, len(idx) - ni, ni1, nb1)
    return br


def test_builder_equals_numpy_on_poisson3d_32(hs, p32):
    br = _check_tree(hs, p32["A"], p32["nd"], 7)
    # the 7-point stencil: rows bnd2 have nothing in columns int1, and int2 starts at its partner in int1
    seen = 0
    for x, lv in br:
        idx, ni, ni1, nb1 = _front(x)
        nb = len(idx) - ni
        if nb - nb1 < 2 * G or ni1 < 2 * G:
            continue
        fL, fU = envelope_library(hs, p32["A"], idx, ni, ni1, nb1)
        nbi = (ni + G - 1) // G
        last = nbi + (nb - 1) // G  # a block of bnd2 alone
        assert fL[last] == ni1 // G * G and fU[last] == ni1 // G * G, (lv, ni, nb, ni1, nb1)
        assert fL[nbi] == 0 and fU[nbi] == 0  # bnd1 meets int1
        assert fL[nbi - 1] > 0 or ni - ni1 <= G  # the last block of int2 does not reach column 0
        seen += 1
    assert seen >= 3


def test_builder_equals_numpy_on_a_2d_problem(hs):
    P = prepare(hs, "poisson2d_p1_h64_nmax100", rhs="randn")
    _check_tree(hs, P["A"], P["nd"], 7)


def _random_symmetric_pattern(n, density, seed):
    R = sp.random(n, n, density=density, random_state=np.random.default_rng(seed), format="csc")
    return sp.csc_matrix(R + R.T + sp.identity(n))


@pytest.mark.parametrize("ni,nb,ni1,nb1", [(75, 50, 37, 21), (75, 100, 0, 64), (64, 40, 33, 40), (70, 0, 35, 0), (33, 97, 33, 0)])
def test_builder_on_synthetic_fronts(hs, ni, nb, ni1, nb1):
    """ni no multiple of 32 with an odd ni1 (a block shared by the two children takes the smaller start); a child without interior or
    without boundary part; a front without boundary."""
    n = 300
    A = _random_symmetric_pattern(n, 0.004, seed=ni + nb1)
    idx = np.random.default_rng(7).permutation(n)[: ni + nb]
    fL, fU = envelope_library(hs, A, idx, ni, ni1, nb1)
    gL, gU = envelope_numpy(_pattern(A).tocsr(), idx, ni, ni1, nb1)
    assert np.array_equal(fL, gL) and np.array_equal(fU, gU)
    nbi = (ni + G - 1) // G
    if ni1 == 0 and nb1 > 0:  # child 1 has boundary rows only: they see the interior through A alone
        dense_only = envelope_numpy(sp.csr_matrix((n, n)), idx, ni, ni1, nb1)[0]
        assert nb1 >= G and dense_only[nbi] == NONE  # (the first boundary block holds rows of child 1 only)
    L = hs._lib.lib()
    assert L.hsk_branch_envelope(0, None, None, None, 1, 1, 0, 0, None, None) != 0


def test_tables_open_up_for_int1_bnd2_entries(hs, p32):
    """A pattern with entries between int1 and bnd2 of a front, on the same tree: the tables of bnd2 must start where those entries are."""
    Ap, nd = p32["A"], p32["nd"]
    x = next(x for x, lv in _branches(nd) if lv == 2)
    idx, ni, ni1, nb1 = _front(x)
    nb = len(idx) - ni
    assert nb - nb1 >= 2 * G and ni1 >= 4 * G
    n = Ap.shape[0]
    r = idx[ni + nb - 1]      # the last DOF of bnd2
    c = idx[2 * G + 5]        # a DOF of int1, third block
    A2 = sp.csc_matrix(_pattern(Ap) + sp.csc_matrix((np.ones(2), ([r, c], [c, r])), shape=(n, n)))
    f0L, f0U = envelope_library(hs, Ap, idx, ni, ni1, nb1)
    f1L, f1U = envelope_library(hs, A2, idx, ni, ni1, nb1)
    g1L, g1U = envelope_numpy(_pattern(A2).tocsr(), idx, ni, ni1, nb1)
    assert np.array_equal(f1L, g1L) and np.array_equal(f1U, g1U)
    last = len(f0L) - 1
    assert f0L[last] == ni1 // G * G and f1L[last] == 2 * G
    assert f0U[last] == ni1 // G * G and f1U[last] == 2 * G
    assert np.array_equal(f0L[:last], f1L[:last]) and np.array_equal(f0U[:last], f1U[:last])
    # a random symmetric pattern on the same tree
    A3 = sp.csc_matrix(_pattern(Ap) + _pattern(_random_symmetric_pattern(n, 2e-4, seed=3)))
    P3 = _pattern(A3).tocsr()
    opened = 0
    for y, lv in _branches(nd):
        if lv > 3:
            continue
        idx, ni, ni1, nb1 = _front(y)
        fL, fU = envelope_library(hs, A3, idx, ni, ni1, nb1)
        gL, gU = envelope_numpy(P3, idx, ni, ni1, nb1)
        assert np.array_equal(fL, gL) and np.array_equal(fU, gU)
        hL, _ = envelope_library(hs, Ap, idx, ni, ni1, nb1)
        assert np.all(fL <= hL)
        opened += int(np.any(fL < hL))
    assert opened >= 1


# ---- the rule itself ------------------------------------------------------------------------------------------------------------------------


def _lu_nopivot(F, ni, bs=32):
    """Right-looking block LU of the first ni columns of F without any row exchange: L (m x ni, unit diagonal implied), U (ni x m)."""
    F = F.copy()
    m = F.shape[0]
    for k0 in range(0, ni, bs):
        k1 = min(k0 + bs, ni)
        for k in range(k0, k1):  # the diagonal block and the panel below it, column by column
            F[k + 1 :, k] /= F[k, k]
            F[k + 1 :, k + 1 : k1] -= np.outer(F[k + 1 :, k], F[k, k + 1 : k1])
        if k1 < m:
            F[k0:k1, k1:] = sla.solve_triangular(F[k0:k1, k0:k1], F[k0:k1, k1:], lower=True, unit_diagonal=True)
            F[k1:, k1:ni] -= F[k1:, k0:k1] @ F[k0:k1, k1:ni]  # (the Schur complement is not formed: L and U are all the rule speaks of)
            F[k1:ni, ni:] -= F[k1:ni, k0:k1] @ F[k0:k1, ni:]
    return np.tril(F[:, :ni], -1), np.triu(F[:ni, :])


def test_rule_on_the_top_levels_of_poisson3d_32(hs, p32):
    """Levels 1-3: the front assembled from the oracle's child S, eliminated without pivoting, has exactly zero L / U outside the tables."""
    Ap = sp.csc_matrix(p32["A"])
    ond, oloc = p32["ond"], p32["ond_loc"]
    # the oracle's factorization of the two subtrees below the root (the root's own elimination is not needed: only its children's S)
    opts = O.SolverOptions()
    Fl = O._factor(Ap, ond.left, oloc.left, 2, swlevel=0, opts=opts)
    Fr = O._factor(Ap, ond.right, oloc.right, 2, swlevel=0, opts=opts)
    FO = O.FactorNode(None, np.zeros((0, 0)), None, None, ond.int, ond.bnd, oloc.int, oloc.bnd, Fl, Fr)
    todo, stack = [], [(FO, ond, oloc, 1)]
    while stack:
        Fn, nd, loc, lv = stack.pop()
        if Fn.left is None or lv > 3:
            continue
        todo.append((Fn, nd, loc, lv))
        stack += [(Fn.left, nd.left, loc.left, lv + 1), (Fn.right, nd.right, loc.right, lv + 1)]
    assert len(todo) == 7
    covered = 0
    for Fn, nd, loc, lv in todo:
        int1 = nd.left.bnd[loc.left.int - 1]
        bnd1 = nd.left.bnd[loc.left.bnd - 1]
        int2 = nd.right.bnd[loc.right.int - 1]
        bnd2 = nd.right.bnd[loc.right.bnd - 1]
        Aii, Aib, Abi, Abb = O._assemble_blocks(Ap, O._dense(Fn.left.S), O._dense(Fn.right.S), int1, int2, bnd1, bnd2)
        F = np.block([[Aii.dense(), Aib.dense()], [Abi.dense(), Abb.dense()]]) if len(bnd1) + len(bnd2) else Aii.dense()
        F = np.asarray(F, dtype=np.float64)
        idx = np.concatenate([int1, int2, bnd1, bnd2]) - 1
        ni, ni1, nb1 = len(int1) + len(int2), len(int1), len(bnd1)
        m = len(idx)
        fL, fU = envelope_library(hs, Ap, idx, ni, ni1, nb1)
        rowfirst = fL[_blk(np.arange(m), ni)]
        colfirst = fU[_blk(np.arange(m), ni)]
        L, U = _lu_nopivot(F, ni)
        k = np.arange(ni)
        outL = k[None, :] < rowfirst[:, None]  # (m x ni): columns left of the row block's first
        outU = k[:, None] < colfirst[None, :]  # (ni x m): rows above the column block's first
        assert np.count_nonzero(L[outL]) == 0 and np.count_nonzero(U[outU]) == 0, (lv, ni, m - ni)
        covered += int(outL.sum() + outU.sum())
        assert (outL.sum() + outU.sum()) / (2.0 * m * ni) > 0.1  # (sanity: the check is not vacuous; the root: 0.12)
    assert covered > 0
