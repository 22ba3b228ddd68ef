"""hs_selinv_lr on the MI355X (csrc/hs_selinv.hip, csrc/kernels_selinv.hip): the selected inverse of COMPRESSED factorizations.

The reference is the same handle's own solves: hs.inv_entries(op, rows, cols) on A's pattern plus the diagonal (pruned sparse solves on unit
columns, the transposed sweeps for trans = 1).  Both sides compute entries of the same F^-1, the operator the stored factors define, so the
bound is the exact path's: <= 1e-10 * max|reference entries| (tests/test_selinv_gpu.py).  The distance to A^-1 is printed on the pattern
entries of 48 sampled columns (SuperLU solves of unit columns; numpy.linalg.inv of the 8000 x 8000 ComplexF64 matrix alone would take
longer than the whole file) and is not asserted: F approximates A to the compression tolerance only.

The handles are the COMPRESSED cases of tests/test_selinv_gpu.py: at 20^3 the flagged fronts have ni = 360, nb = 400 -- two 256-blocks with a
ragged second one, rL != rR, Float64 and ComplexF64 -- the smallest shape that runs the multi-block substitutions on the copied factors;
poisson 16^3 flags every level (with mf = 1 every branch is a matrix-free front whose D is eliminated densely)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import selinv_lr_mirror as ML
from helpers import prepare

pytestmark = pytest.mark.gpu

CKW = dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, leafsize=32)
COMPRESSED = [("convdiff", (20, 20, 20), 200, CKW), ("convdiff_helmholtz", (20, 20, 20), 200, CKW),
              ("poisson", (16, 16, 16), 512, dict(swlevel=None, swsize=8, atol=1e-6, rtol=1e-6, leafsize=128))]
BIG = ("convdiff", (20, 20, 20), 200)

_PREP = {}
_CACHE = {}
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for F in _CACHE.values():
        F.free()
    _CACHE.clear()
    _REF.clear()
    _PREP.clear()


def _prep(hs, kind, shape, nmax):
    if (kind, shape, nmax) not in _PREP:
        _PREP[(kind, shape, nmax)] = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    return _PREP[(kind, shape, nmax)]


def _factor(hs, kind, shape, nmax, **kw):
    P = _prep(hs, kind, shape, nmax)
    kw = dict(kw)
    if kw.get("swlevel", 0) is None:
        kw["swlevel"] = hs.depth(P["nd"])
    key = (kind, shape, nmax, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = hs.factor(P["A"], P["nd"], P["nd_loc"], **kw)
    return P, _CACHE[key], key


def _pattern(A):
    A = sp.csc_matrix(A)
    return A.indices.astype(np.int64), np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)).astype(np.int64)


def _own_entries(hs, F, key, A):
    """F^-1 on A's pattern and on the diagonal, trans = 0 and 1, by the handle's own solves; once per handle."""
    if key not in _REF:
        rows, cols = _pattern(A)
        dg = np.arange(A.shape[0], dtype=np.int64)
        I, J = np.concatenate([rows, dg]), np.concatenate([cols, dg])
        _REF[key] = (hs.inv_entries(F, I, J), hs.inv_entries(hs.transpose(F), I, J))
    return _REF[key]


def _check_against_own_solves(hs, F, key, A, tag):
    nnz = A.nnz
    worst = 0.0
    for trans, op in ((0, F), (1, hs.transpose(F))):
        ref = _own_entries(hs, F, key, A)[trans]
        scale = np.abs(ref).max()
        d, Z = hs.selinv_lr(op)
        assert np.array_equal(Z.indptr, A.indptr) and np.array_equal(Z.indices, A.indices)
        ed = np.abs(d - ref[nnz:]).max() / scale
        ez = np.abs(Z.data - ref[:nnz]).max() / scale
        print(f"{tag} trans={trans}: diag {ed:.1e}, pattern {ez:.1e} (* max|F^-1 entries| = {scale:.2e})")
        worst = max(worst, ed, ez)
    if worst > 1e-10:
        print(f"{tag}: condest(F) = {hs.condest(F):.3e}")
    assert worst <= 1e-10, (tag, worst)


def _print_distance_to_A(hs, F, A, tag, ncols=48):
    rng = np.random.default_rng(11)
    n = A.shape[0]
    js = np.sort(rng.choice(n, size=ncols, replace=False))
    E = np.zeros((n, ncols), dtype=A.dtype)
    E[js, np.arange(ncols)] = 1.0
    X = spla.splu(sp.csc_matrix(A)).solve(E)
    _, Z = hs.selinv_lr(F, diag=False)
    worst = 0.0
    for k, j in enumerate(js):
        sl = slice(Z.indptr[j], Z.indptr[j + 1])
        worst = max(worst, np.abs(Z.data[sl] - X[Z.indices[sl], k]).max())
    print(f"{tag}: distance to A^-1 on the pattern of {ncols} columns {worst / np.abs(X).max():.1e} * max|A^-1 columns| (not asserted)")


@pytest.mark.parametrize("mf", [0, 1])
@pytest.mark.parametrize("kind,shape,nmax,kw", COMPRESSED)
def test_against_the_same_handles_solves_and_info(hs, kind, shape, nmax, kw, mf):
    """Measured on the MI355X (diagonal and pattern, trans = 0 / 1, in units of max|F^-1 entries|): convdiff 20^3 2.6e-15 / 1.7e-15,
    convdiff_helmholtz 20^3 3.8e-15 / 3.3e-15, poisson 16^3 2.0e-15 / 1.8e-15, the same with mf = 1; distance to A^-1 2e-8 .. 4.5e-8 at
    atol = rtol = 1e-6.  Ranks: 207 / 211 at 20^3 (flops 0.96 of the dense form), 152 at 16^3."""
    P, F, key = _factor(hs, kind, shape, nmax, mf=bool(mf), **kw)
    A = P["A"]
    tag = f"{kind} {shape} mf={mf}"
    _check_against_own_solves(hs, F, key, A, tag)
    _print_distance_to_A(hs, F, A, tag)
    # info: the fronts served through low-rank transforms are the fronts that report compression, the largest rank is maxrank(F)
    info = hs.selinv_lr_info(F)
    flagged = [k for k in range(F.nnodes) if F.node_ranks(k)[0]]
    flow = (hs._lib.i64 * 8)()
    hs._lib.check(hs._lib.lib().hs_flow_info(F._h, flow))
    print(f"{tag}: {info}; flagged fronts {len(flagged)}, hs_flow_info {list(flow)}")
    assert info["lowrank_fronts"] == len(flagged) > 0
    if not mf:
        assert info["lowrank_fronts"] == flow[3]
    assert info["max_rank"] == hs.maxrank(F)
    # the dense-form count is the mirror's, exactly: both count the 256-blocks as they are launched (no rounding slack to allow for)
    cplx = F.dtype.kind == "c"
    dense = sum(ML.dense_form_flops(*F.node_info(k)[:2], cplx=cplx) for k in range(F.nnodes))
    assert info["flops_dense_form"] == dense
    lr = 0.0
    for k in range(F.nnodes):
        ni, nb, _ = F.node_info(k)
        comp, rl, rr = F.node_ranks(k)
        lr += ML.lr_form_flops(ni, nb, rl, rr, cplx) if comp else ML.dense_form_flops(ni, nb, cplx)
    if not mf:  # (a matrix-free front's ranks are not all reported by node_ranks)
        assert info["flops"] == lr
    assert info["seconds"] > 0 and info["peak_bytes"] > 0 and info["batches"] >= 1


def test_exact_handle_returns_the_bits_of_selinv(hs):
    kind, shape, nmax = BIG
    P, F, _ = _factor(hs, kind, shape, nmax, swlevel=0)
    d0, Z0 = hs.selinv(F)
    i0 = hs.selinv_info(F)
    for op in (F, hs.transpose(F)):
        d, Z = hs.selinv(op)
        dl, Zl = hs.selinv_lr(op)
        assert np.array_equal(d, dl) and np.array_equal(Z.data, Zl.data)
    il = hs.selinv_lr_info(F)
    assert il["lowrank_fronts"] == 0 and il["max_rank"] == 0
    assert il["flops"] == il["flops_dense_form"] == i0["flops"] and il["batches"] == i0["batches"]


def test_small_budget_cuts_levels_into_batches(hs):
    """A front's arithmetic does not depend on which fronts share its launches, low-rank fronts included."""
    kind, shape, nmax, kw = COMPRESSED[0]
    P, F, _ = _factor(hs, kind, shape, nmax, mf=False, **kw)
    d0, Z0 = hs.selinv_lr(F)
    i0 = hs.selinv_lr_info(F)
    d1, Z1 = hs.selinv_lr(F, budget=1)
    i1 = hs.selinv_lr_info(F)
    assert i1["batches"] == F.nnodes > i0["batches"] and i1["flops"] == i0["flops"] and i1["peak_bytes"] < i0["peak_bytes"]
    assert np.array_equal(d1, d0) and np.array_equal(Z1.data, Z0.data)
    d2, Z2 = hs.selinv_lr(F, budget=int(i0["peak_bytes"] // 2))
    i2 = hs.selinv_lr_info(F)
    print(f"batches {i0['batches']} -> {i2['batches']} -> {i1['batches']}, peak scratch {i0['peak_bytes'] / 2**20:.0f} -> {i2['peak_bytes'] / 2**20:.0f} "
          f"-> {i1['peak_bytes'] / 2**20:.0f} MiB")
    assert i0["batches"] < i2["batches"] and i2["flops"] == i0["flops"]
    assert np.array_equal(d2, d0) and np.array_equal(Z2.data, Z0.data)


@pytest.mark.parametrize("mf", [0, 1])
def test_repeatable_isolated_and_other_forms_of_the_call(hs, mf):
    import torch

    kind, shape, nmax, kw = COMPRESSED[1]  # ComplexF64
    P, F, _ = _factor(hs, kind, shape, nmax, mf=bool(mf), **kw)
    A = P["A"]
    n = A.shape[0]
    b = P["b"]
    x0, xt0 = F.solve(b), F.solve(b, "T")
    sel0 = hs.selinv_info(F)
    d0, Z0 = hs.selinv_lr(F)
    d1, Z1 = hs.selinv_lr(F)
    assert np.array_equal(d0, d1) and np.array_equal(Z0.data, Z1.data)  # two calls, the same bits
    assert np.array_equal(F.solve(b), x0) and np.array_equal(F.solve(b, "T"), xt0)  # the stored factors are only read
    assert hs.selinv_info(F) == sel0  # hs_selinv's figures are its own
    il = hs.selinv_lr_info(F)
    with pytest.raises(hs.UnsupportedError, match="low-rank"):
        hs.selinv(F)
    assert hs.selinv_lr_info(F) == il
    # device pointers on a side stream
    dev = torch.device("cuda:0")
    dd = torch.zeros(n, dtype=torch.complex128, device=dev)
    dz = torch.zeros(A.nnz, dtype=torch.complex128, device=dev)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        hs._lib.check(hs._lib.lib().hs_selinv_lr(F._h, 0, C.c_void_p(dd.data_ptr()), C.c_void_p(dz.data_ptr()), 1, 0, C.c_void_p(s.cuda_stream)))
    s.synchronize()
    assert np.array_equal(dd.cpu().numpy(), d0) and np.array_equal(dz.cpu().numpy(), Z0.data)
    # diagonal only / pattern only
    assert np.array_equal(hs.selinv_lr_diag(F), d0)
    dn, Zn = hs.selinv_lr(F, diag=False)
    assert dn is None and np.array_equal(Zn.data, Z0.data)
    dp, Zp = hs.selinv_lr(F, pattern=False)
    assert Zp is None and np.array_equal(dp, d0)
    # the adjoint is the conjugate of the transpose
    dt, Zt = hs.selinv_lr(hs.transpose(F))
    da, Za = hs.selinv_lr(hs.adjoint(F))
    assert np.array_equal(da, dt.conj()) and np.array_equal(Za.data, Zt.data.conj())


def test_ranks_of_zero(hs):
    """atol = rtol = 1e3: every transform is truncated to rank 0, the flagged fronts decouple from their boundaries."""
    kind, shape, nmax, kw = COMPRESSED[0]
    kw = dict(kw, atol=1e3, rtol=1e3)
    P, F, key = _factor(hs, kind, shape, nmax, mf=False, **kw)
    assert hs.maxrank(F) == 0
    _check_against_own_solves(hs, F, key, P["A"], "rank 0")
    info = hs.selinv_lr_info(F)
    assert info["lowrank_fronts"] > 0 and info["max_rank"] == 0


def test_fewer_flops_than_the_dense_form_at_a_loose_tolerance(hs):
    """convdiff 20^3 at tol 1e-2: the oracle's ranks (80-92 at ni = 360, nb = 400) give 0.44 of the dense form's flops on the flagged fronts,
    and device ranks are within 25 % of the oracle's elsewhere in this suite: the rank-structured form must execute fewer flops."""
    kind, shape, nmax, kw = COMPRESSED[0]
    kw = dict(kw, atol=1e-2, rtol=1e-2)
    P, F, key = _factor(hs, kind, shape, nmax, mf=False, **kw)
    _check_against_own_solves(hs, F, key, P["A"], "tol 1e-2")
    info = hs.selinv_lr_info(F)
    print(f"tol 1e-2: flops {info['flops']:.3e} of dense form {info['flops_dense_form']:.3e} = {info['flops'] / info['flops_dense_form']:.2f}, max rank {info['max_rank']}")
    assert info["flops"] < info["flops_dense_form"]


def test_refusals(hs):
    import torch

    L = hs._lib.lib()
    UNS, ARG = hs._lib.HS_ERR_UNSUPPORTED, hs._lib.HS_ERR_ARGUMENT
    # HSS interior blocks (mf = 2)
    P2 = _prep(hs, "convdiff", (20, 20, 20), 200)
    b = P2["b"]
    F2 = hs.factor(P2["A"], P2["nd"], P2["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    x2 = F2.solve(b)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.selinv_lr(F2)
    assert np.array_equal(F2.solve(b), x2)
    F2.free()
    # fronts eliminated in slices
    P3 = prepare(hs, "poisson3d_32", rhs="randn")  # (the root separator has 1024 DOFs: split_size = 256 cuts it into slices)
    F3 = hs.factor(P3["A"], P3["nd"], P3["nd_loc"], swlevel=3, swsize=8, atol=1e-6, rtol=1e-6, split_size=256)
    x3 = F3.solve(P3["b"])
    with pytest.raises(hs.UnsupportedError, match="slices"):
        hs.selinv_lr(F3)
    assert np.array_equal(F3.solve(P3["b"]), x3)
    F3.free()
    # rank 0 of a two-rank plan
    P = _prep(hs, "convdiff", (16, 16), 20)
    be = hs.dist.HipBackend(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=2, device=torch.device("cuda:0"), swlevel=0)
    d = np.zeros(P["A"].shape[0])
    assert L.hs_selinv_lr(be._h, 0, d.ctypes.data, None, 0, 0, None) == UNS and b"ranks" in L.hs_last_error()
    del be
    # argument errors on a compressed factorization
    kind, shape, nmax, kw = COMPRESSED[0]
    Pc, F, _ = _factor(hs, kind, shape, nmax, mf=False, **kw)
    bc = Pc["b"]
    x0 = F.solve(bc)
    d = np.zeros(Pc["A"].shape[0])
    for trans in (2, -1):
        assert L.hs_selinv_lr(F._h, trans, d.ctypes.data, None, 0, 0, None) == ARG and b"trans" in L.hs_last_error()
    assert L.hs_selinv_lr(F._h, 0, d.ctypes.data, None, 2, 0, None) == ARG and b"where" in L.hs_last_error()
    assert L.hs_selinv_lr(F._h, 0, None, None, 0, 0, None) == ARG and b"NULL" in L.hs_last_error()
    assert L.hs_selinv_lr(F._h, 0, d.ctypes.data, None, 0, -1, None) == ARG and b"budget" in L.hs_last_error()
    with pytest.raises(ValueError):
        hs.selinv_lr(F, diag=False, pattern=False)
    assert np.array_equal(F.solve(bc), x0)
    # a plan that was analyzed but not factored
    plan = C.c_void_p()
    A = sp.csc_matrix(P["A"])
    n = A.shape[0]
    flat = hs.flatten_tree(P["nd"], P["nd_loc"])
    t = hs._lib.hs_tree()
    t.nnodes = flat["nnodes"]
    keep = []
    for k in ("left", "right", "int_ptr", "int_idx", "bnd_ptr", "bnd_idx", "iloc_ptr", "iloc_idx", "bloc_ptr", "bloc_idx"):
        a = np.ascontiguousarray(flat[k], dtype=np.int64)
        keep.append(a)
        setattr(t, k, a.ctypes.data_as(hs._lib.p_i64))
    o = hs.SolverOptions(swlevel=2, swsize=8).to_c()
    cp, rv = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1, np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    hs._lib.check(L.hs_analyze(0, n, cp.ctypes.data_as(hs._lib.p_i64), rv.ctypes.data_as(hs._lib.p_i64), C.byref(t), C.byref(o), 0, 1, C.byref(plan)))
    d = np.zeros(n)
    assert L.hs_selinv_lr(plan, 0, d.ctypes.data, None, 0, 0, None) == ARG and b"factorization" in L.hs_last_error()
    L.hs_free(plan)
