"""Sparse right-hand sides and selected rows of the solution (hs_ldiv_sparse_*, csrc/hs_solve_sparse.hip + kernels_solve_sparse.hip) on the
MI355X: bit for bit against the block solve of the expanded right-hand side, the counters against a closure computed here from the
elimination tree, entries of the inverse against SuperLU and hs_selinv, and the refusals.  Problems and option sets are those of
test_ldiv_block_gpu.py; one factorization per (kind, options) is shared by the tests of this file."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from helpers import prepare
from test_ldiv_block_gpu import COMPRESSED, EXACT, _kc, _rand
from test_ldiv_sparse_host import expected_plan, sources, tree_closure

pytestmark = pytest.mark.gpu

TOL = 1e-10  # per column, relative to its largest entry (test_ldiv_block_gpu.py, test_selinv_gpu.py)
BIG = ("convdiff", (24, 24, 24), 300), ("convdiff_helmholtz", (24, 24, 24), 300)
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for c in _CACHE.values():
        c["F"].free()
    _CACHE.clear()


def _get(hs, kind, shape, nmax, label="exact", **kw):
    key = (kind, shape, nmax, label)
    if key not in _CACHE:
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        F = hs.factor(P["A"], P["nd"], P["nd_loc"], **(kw or dict(swlevel=0)))
        n = P["A"].shape[0]
        owner, parent = tree_closure(P["nd"], n)
        leaves = [i for i in range(len(parent)) if i not in set(parent)]
        _CACHE[key] = dict(P=P, F=F, n=n, owner=owner, parent=parent, leaf=np.flatnonzero(owner == leaves[1]), far=np.flatnonzero(owner == leaves[-2]))
    return _CACHE[key]


def _op(hs, F, trans):
    return (F, hs.transpose(F), hs.adjoint(F))[trans]


def _rowsets(c, seed):
    rng = np.random.default_rng(seed)
    few = rng.choice(c["far"], size=4, replace=False)
    return {"few": few, "all": None, "repeated": np.array([few[2], few[0], c["n"] - 1, few[2], 0])}


def _check_exact(hs, c, trans, nrhs, where, empty, seed):
    F, n = c["F"], c["n"]
    B = sources(n, nrhs, where, c["leaf"], F.dtype.kind == "c", seed, empty)
    ref = hs.ldiv_block_t(_op(hs, F, trans), B.toarray().astype(F.dtype))
    for name, rows in _rowsets(c, seed).items():
        X = hs.ldiv_sparse(_op(hs, F, trans), B, rows)
        want = ref if rows is None else ref[rows]
        assert X.shape == want.shape and X.flags.f_contiguous
        assert np.array_equal(X, want), (trans, nrhs, where, empty, name)
        if empty is not None:
            assert np.all(X[:, empty] == 0)


@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_wanted_rows_carry_the_bits_of_the_block_solve(hs, kind, shape, nmax):
    c = _get(hs, kind, shape, nmax)
    variants = [("leaf", None), ("anywhere", None), ("leaf", 0)]
    i = 0
    for trans in (0, 1, 2):
        for nrhs in (1, 5, 40, 70):
            where, empty = variants[i % 3]
            _check_exact(hs, c, trans, nrhs, where, empty if empty is None else nrhs // 2, 10 * i + 1)
            i += 1
    # a block of empty columns only, and an empty chunk behind a full one: exact zeros, and nothing is launched for them
    for B in (sp.csc_matrix((c["n"], 3)), sp.hstack([sources(c["n"], _kc(), "leaf", c["leaf"], False, 3), sp.csc_matrix((c["n"], 2))]).tocsc()):
        X = hs.ldiv_sparse(c["F"], B.astype(c["F"].dtype), c["far"][:3])
        assert np.all(X[:, -2:] == 0) and X.shape == (3, B.shape[1])
    assert hs.ldiv_sparse_info(c["F"])["visits_forward"] < hs.ldiv_sparse_info(c["F"])["visits_dense"] / 2
    assert hs.ldiv_sparse(c["F"], sp.csc_matrix((c["n"], 0)), None).shape == (c["n"], 0)
    assert hs.ldiv_sparse(c["F"], sources(c["n"], 2, "leaf", c["leaf"], False, 1), np.zeros(0, dtype=np.int64)).shape == (0, 2)


@pytest.mark.parametrize("label,kind,shape,nmax,kw", COMPRESSED, ids=[x[0] for x in COMPRESSED])
def test_compressed_handles_carry_the_bits_of_the_block_solve(hs, label, kind, shape, nmax, kw):
    c = _get(hs, kind, shape, nmax, label, **kw)
    assert hs.maxrank(c["F"]) > 0  # low-rank Gauss transforms are in the solve
    i = 0
    for trans in (0, 1, 2):
        for nrhs, where, empty in ((5, "leaf", None), (40, "anywhere", 7)):
            _check_exact(hs, c, trans, nrhs, where, empty, 50 + i)
            i += 1


def test_another_chunk_width_in_a_fresh_process(hs, tmp_path):
    kind, shape, nmax = BIG[1]
    c = _get(hs, kind, shape, nmax)
    B = sources(c["n"], 70, "anywhere", c["leaf"], True, 77, empty=11)
    rows = _rowsets(c, 77)["repeated"]
    sp.save_npz(tmp_path / "B.npz", B)
    np.save(tmp_path / "rows.npy", rows)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"""
import sys, numpy as np, scipy.sparse as sp
sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, "tests")!r})
import hsamd
from helpers import prepare
hs = hsamd.load()
P = prepare(hs, {shape!r}, kind={kind!r}, nmax={nmax}, rhs="randn")
F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
B = sp.load_npz({str(tmp_path / "B.npz")!r}).tocsc()
rows = np.load({str(tmp_path / "rows.npy")!r})
for op in (F, hs.transpose(F), hs.adjoint(F)):
    X = hs.ldiv_sparse(op, B, rows)
    assert hs.ldiv_sparse_info(F)["chunks"] == 5
    assert np.array_equal(X, hs.ldiv_block_t(op, B.toarray())[rows])
np.save({str(tmp_path / "X16.npy")!r}, hs.ldiv_sparse(F, B, rows))
"""
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, HS_LDIV_BLOCK_COLS="16"), timeout=300)
    X16 = np.load(tmp_path / "X16.npy")
    X = hs.ldiv_sparse(c["F"], B, rows)
    scale = np.abs(X).max(axis=0)
    scale[scale == 0] = 1.0
    d = float((np.abs(X16 - X).max(axis=0) / scale).max())
    print(f"chunks of 16 against chunks of {_kc()}: bitwise {np.array_equal(X16, X)}, worst column {d:.2e}")
    assert d < 1e-11  # the bound test_ldiv_block_gpu.py sets between two chunk widths


@pytest.mark.parametrize("kind,shape,nmax", BIG)
def test_nothing_stale_and_nothing_left_behind(hs, kind, shape, nmax):
    c = _get(hs, kind, shape, nmax)
    F, n = c["F"], c["n"]
    cplx = F.dtype.kind == "c"
    Bd = _rand(n, 40, cplx, 31)
    b = _rand(n, 2, cplx, 32)
    B = sources(n, 37, "leaf", c["leaf"], cplx, 5)  # sources in one leaf, receivers in another: fronts only the backward sweep visits
    rows = c["far"][:6]
    plan = hs.ldiv_sparse_plan(F, B, rows)["active"]
    assert np.any((plan & 3) == 2) and np.any((plan & 3) == 1)
    for trans in (0, 1, 2):
        op = _op(hs, F, trans)
        ref = hs.ldiv_block_t(op, B.toarray().astype(F.dtype))[rows]
        x0 = hs.ldiv(op, b)
        X0 = hs.ldiv_block_t(op, Bd)  # fills work block 2 with the x of a dense block
        assert np.array_equal(hs.ldiv_sparse(op, B, rows), ref)
        assert np.array_equal(hs.ldiv_block_t(op, Bd), X0)
        assert np.array_equal(hs.ldiv(op, b), x0)
        assert np.array_equal(hs.ldiv_sparse(op, B, rows), ref)


@pytest.mark.parametrize("kind,shape,nmax", BIG)
def test_counters_equal_a_closure_computed_from_the_tree(hs, kind, shape, nmax):
    c = _get(hs, kind, shape, nmax)
    F, n = c["F"], c["n"]
    esz = 16 if F.dtype.kind == "c" else 8
    nn = F.nnodes
    assert nn == len(c["parent"])
    ni = np.array([F.node_info(i)[0] for i in range(nn)], dtype=np.float64)
    nb = np.array([F.node_info(i)[1] for i in range(nn)], dtype=np.float64)
    w = 0.5 * ni * ni + ni * nb
    for nrhs, where, rows in ((70, "anywhere", c["far"][:5]), (40, "leaf", None), (5, "leaf", np.array([3, 3, n - 1]))):
        B = sources(n, nrhs, where, c["leaf"], F.dtype.kind == "c", nrhs, empty=2)
        hs.ldiv_sparse(F, B, rows)
        info = hs.ldiv_sparse_info(F)
        order, active = expected_plan(c["owner"], c["parent"], B, rows, _kc())
        fwd, bwd = (active & 1).astype(bool), (active & 2).astype(bool)
        assert info["visits_forward"] == fwd.sum() and info["visits_backward"] == bwd.sum()
        assert info["visits_dense"] == nn * active.shape[0] and info["chunks"] == active.shape[0]
        assert info["factor_bytes"] == esz * float((fwd * w).sum() + (bwd * w).sum())
        assert info["values_moved"] == B.nnz + (n if rows is None else len(rows)) * nrhs
        assert info["seconds"] > 0 and info["workspace_bytes"] > 0 and info["seconds"] == F.stats()["t_solve"]
        got = hs.ldiv_sparse_plan(F, B, rows)
        assert np.array_equal(got["order"], order) and np.array_equal(got["active"], active)
        assert info["visits_forward"] < info["visits_dense"]
    # every front in both sweeps: the figure of the block solve
    Bd = _rand(n, 37, F.dtype.kind == "c", 9)
    X = hs.ldiv_sparse(F, sp.csc_matrix(Bd), None)
    info = hs.ldiv_sparse_info(F)
    Xb = hs.ldiv_block(F, Bd)
    assert np.array_equal(X, Xb)
    assert info["factor_bytes"] == hs.ldiv_block_info(F)["factor_bytes"]
    assert info["visits_forward"] == info["visits_backward"] == info["visits_dense"]


def _column_errors(got, ref, J):
    """Worst over the columns of max |got - ref| over the pairs of the column, relative to the largest entry of that column of the inverse."""
    worst = 0.0
    for j, (col, scale) in ref.items():
        m = J == j
        worst = max(worst, float(np.abs(got[m] - col[m]).max() / scale))
    return worst


@pytest.mark.parametrize("kind,shape,nmax", BIG)
def test_inv_entries_against_splu_and_selinv(hs, kind, shape, nmax):
    c = _get(hs, kind, shape, nmax)
    F, n, A = c["F"], c["n"], c["P"]["A"]
    lu = spla.splu(A)
    rng = np.random.default_rng(13)
    r8, c8 = rng.choice(n, 8, replace=False), rng.choice(n, 8, replace=False)
    I = np.concatenate([rng.integers(0, n, 200), np.repeat(r8, 8)])
    J = np.concatenate([rng.integers(0, n, 200), np.tile(c8, 8)])
    cols = np.unique(J)
    E = np.zeros((n, len(cols)), dtype=F.dtype)
    E[cols, np.arange(len(cols))] = 1
    S = lu.solve(E)
    ref = {}
    want = np.zeros(len(I), dtype=F.dtype)
    for k, j in enumerate(cols):
        col = np.zeros(len(I), dtype=F.dtype)
        col[J == j] = S[I[J == j], k]
        want[J == j] = S[I[J == j], k]
        ref[j] = (col, float(np.abs(S[:, k]).max()))
    got = hs.inv_entries(F, I, J)
    e = _column_errors(got, ref, J)
    # adjoint(F): (A^H)^-1[i, j] = conj(A^-1[j, i])
    ea = _column_errors(np.conj(hs.inv_entries(hs.adjoint(F), J, I)), ref, J)
    et = _column_errors(hs.inv_entries(hs.transpose(F), J, I), ref, J)
    # pairs inside the pattern of A: hs_selinv
    Ac = A.tocoo()
    pick = rng.choice(Ac.nnz, 60, replace=False)
    Ip, Jp = Ac.row[pick].astype(np.int64), Ac.col[pick].astype(np.int64)
    Z = hs.selinv(F, diag=False)[1]
    z = np.asarray(Z[Ip, Jp]).ravel()
    gp = hs.inv_entries(F, Ip, Jp)
    colsp = np.unique(Jp)
    Ep = np.zeros((n, len(colsp)), dtype=F.dtype)
    Ep[colsp, np.arange(len(colsp))] = 1
    scale = dict(zip(colsp, np.abs(lu.solve(Ep)).max(axis=0)))
    es = max(abs(gp[k] - z[k]) / scale[Jp[k]] for k in range(len(Ip)))
    print(f"{kind}: inv_entries vs splu {e:.2e}, adjoint {ea:.2e}, transpose {et:.2e}, vs selinv on the pattern {es:.2e}")
    assert e < TOL and ea < TOL and et < TOL and es < TOL
    assert hs.inv_entries(F, [], []).shape == (0,)
    with pytest.raises(hs.DimensionMismatch):
        hs.inv_entries(F, [0, 1], [n, 0])


def test_inv_entries_of_a_compressed_factorization(hs):
    label, kind, shape, nmax, kw = COMPRESSED[1]
    assert label == "tol1e-8"
    c = _get(hs, kind, shape, nmax, label, **kw)
    F, n = c["F"], c["n"]
    rng = np.random.default_rng(2)
    I, J = rng.integers(0, n, 90), rng.integers(0, n, 90)
    cols = np.unique(J)
    E = np.zeros((n, len(cols)), dtype=F.dtype)
    E[cols, np.arange(len(cols))] = 1
    X = hs.ldiv_block(F, E)
    assert np.array_equal(hs.inv_entries(F, I, J), X[I, np.searchsorted(cols, J)])


def _raw(hs, F, trans, n, B, rows, X, ldx, nrows=None, colptr=None, rowval=None, vals=True, dtype=None):
    E = hs._lib
    L = E.lib()
    fn = L.hs_ldiv_sparse_z if np.dtype(dtype or F.dtype).kind == "c" else L.hs_ldiv_sparse_d
    cp = np.ascontiguousarray(B.indptr, dtype=np.int64) + 1 if colptr is None else colptr
    rv = np.ascontiguousarray(B.indices, dtype=np.int64) + 1 if rowval is None else rowval
    v = np.ascontiguousarray(B.data, dtype=dtype or F.dtype)
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    return fn(F._h, trans, n, B.shape[1], cp.ctypes.data_as(E.p_i64), rv.ctypes.data_as(E.p_i64), v.ctypes.data_as(E.p_f64) if vals else None,
              None if r is None else r.ctypes.data_as(E.p_i64), (0 if r is None else len(r)) if nrows is None else nrows,
              None if X is None else X.ctypes.data_as(E.p_f64), ldx)


def test_refusals(hs):
    E = hs._lib
    for shape, nmax, kw in (((32, 32, 32), 512, dict(hss_min=1024)), ((24, 24, 24), 300, dict(mf=2, leafsize=128))):
        P = prepare(hs, shape, kind="convdiff", nmax=nmax, rhs="randn")
        F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, **kw)
        n = P["A"].shape[0]
        B = sources(n, 3, "anywhere", None, False, 1)
        with pytest.raises(hs.UnsupportedError, match="HSS"):
            hs.ldiv_sparse(F, B, [0, 1])
        with pytest.raises(hs.UnsupportedError, match="HSS"):
            hs.ldiv_sparse_plan(F, B, [0, 1])
        X = np.full((2, 3), 42.0, order="F")
        for trans in (0, 1, 2):
            assert _raw(hs, F, trans, n, B, [1, 2], X, 2) == E.HS_ERR_UNSUPPORTED
        assert np.all(X == 42.0)
        F.free()
    c = _get(hs, "convdiff", (30, 27), 40)
    F, n = c["F"], c["n"]
    B = sources(n, 3, "anywhere", None, False, 2)
    X = np.full((4, 3), 42.0, order="F")
    rows = [1, n, 5]
    cp = np.ascontiguousarray(B.indptr, dtype=np.int64) + 1
    rv = np.ascontiguousarray(B.indices, dtype=np.int64) + 1
    assert _raw(hs, F, 0, n, B, rows, X, 4) == E.HS_OK and not np.any(X[:3] == 42.0) and np.all(X[3] == 42.0)  # ldx > nrows: the padding row stays
    X[...] = 42.0
    assert _raw(hs, F, 3, n, B, rows, X, 4) == E.HS_ERR_ARGUMENT
    assert _raw(hs, F, 0, n - 1, B, rows, X, 4) == E.HS_ERR_DIMENSION
    assert _raw(hs, F, 0, n, B, rows, X, 2) == E.HS_ERR_DIMENSION  # ldx too small
    assert _raw(hs, F, 0, n, B, [0], X, 4) == E.HS_ERR_DIMENSION and _raw(hs, F, 0, n, B, [n + 1], X, 4) == E.HS_ERR_DIMENSION
    assert _raw(hs, F, 0, n, B, rows, X, 4, colptr=cp - 1) == E.HS_ERR_ARGUMENT
    bad = cp.copy()
    bad[1] = bad[-1] + 1
    assert _raw(hs, F, 0, n, B, rows, X, 4, colptr=bad) == E.HS_ERR_ARGUMENT
    out = rv.copy()
    out[-1] = n + 1
    assert _raw(hs, F, 0, n, B, rows, X, 4, rowval=out) == E.HS_ERR_DIMENSION
    two = sp.csc_matrix((np.ones(2), ([4, 9], [0, 0])), shape=(n, 1))
    assert _raw(hs, F, 0, n, two, rows, X, 4, rowval=np.array([10, 5], dtype=np.int64)) == E.HS_ERR_ARGUMENT
    assert _raw(hs, F, 0, n, two, rows, X, 4, rowval=np.array([5, 5], dtype=np.int64)) == E.HS_ERR_ARGUMENT
    assert _raw(hs, F, 0, n, B, rows, None, 4) == E.HS_ERR_ARGUMENT
    assert _raw(hs, F, 0, n, B, rows, X, 4, vals=False) == E.HS_ERR_ARGUMENT
    assert _raw(hs, F, 0, n, B, rows, X, 4, nrows=-1) == E.HS_ERR_DIMENSION
    Xz = np.full((4, 3), 42.0, dtype=np.complex128, order="F")
    assert _raw(hs, F, 0, n, B, rows, Xz, 4, dtype=np.complex128) == E.HS_ERR_ARGUMENT  # eltype of F and B differ
    assert _raw(hs, F, 0, n, B[:, :0], rows, X, 4) == E.HS_OK  # nrhs = 0
    assert _raw(hs, F, 0, n, B, [], X, 4) == E.HS_OK  # an empty row list
    assert np.all(X == 42.0) and np.all(Xz == 42.0)
    with pytest.raises(TypeError, match="MethodError"):
        hs.ldiv_sparse(F, B.astype(np.complex128), [0])
    with pytest.raises(hs.DimensionMismatch):
        hs.ldiv_sparse(F, B[:-1], [0])
    with pytest.raises(hs.DimensionMismatch):
        hs.ldiv_sparse(F, B, [n])
    with pytest.raises(TypeError):
        hs.ldiv_sparse(F, B.toarray(), [0])


@pytest.mark.parametrize("kind,shape,nmax", BIG)
def test_device_entry_point_on_a_side_stream(hs, kind, shape, nmax):
    import torch

    c = _get(hs, kind, shape, nmax)
    F, n = c["F"], c["n"]
    cplx = F.dtype.kind == "c"
    E = hs._lib
    fdev = E.lib().hs_ldiv_sparse_dev_z if cplx else E.lib().hs_ldiv_sparse_dev_d
    B = sources(n, 45, "anywhere", c["leaf"], cplx, 8, empty=44)
    B.sort_indices()
    cp = np.ascontiguousarray(B.indptr, dtype=np.int64) + 1
    rv = np.ascontiguousarray(B.indices, dtype=np.int64) + 1
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    dv = torch.from_numpy(np.ascontiguousarray(B.data, dtype=F.dtype)).to(dev)
    for trans in (0, 1, 2):
        for rows in (c["far"][:7], None):
            ref = hs.ldiv_sparse(_op(hs, F, trans), B, rows)
            nout = ref.shape[0]
            ld = nout + 3
            dX = torch.full((45, ld), 7.0, dtype=dv.dtype, device=dev)  # row j of dX = column j of X (column-major, ld)
            r1 = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64) + 1
            with torch.cuda.stream(s):
                hs._lib.check(fdev(F._h, trans, n, 45, cp.ctypes.data_as(E.p_i64), rv.ctypes.data_as(E.p_i64), C.c_void_p(dv.data_ptr()),
                                   None if r1 is None else r1.ctypes.data_as(E.p_i64), 0 if r1 is None else len(r1), C.c_void_p(dX.data_ptr()), ld,
                                   C.c_void_p(s.cuda_stream)))
            s.synchronize()
            got = dX.cpu().numpy().T
            assert np.array_equal(got[:nout], ref) and np.all(got[nout:] == 7.0)
            assert hs.ldiv_sparse_info(F)["values_moved"] == 0
