"""hs_logabsdet and hs_selinv on the MI355X (csrc/hs_selinv.hip, csrc/kernels_selinv.hip) against numpy.linalg.inv / slogdet.

Tolerances and where they come from: entries of the selected inverse <= 1e-10 * max|A^-1| -- the bound the exact path is held to against
SuperLU and the golden blocks elsewhere in this suite, three orders of magnitude above what the CPU statement of the recurrence
(tests/selinv_mirror.py) and scipy's splu(A).solve(I) show on these inputs (<= 1.1e-13), which leaves room for the device's pivot order
and the summation order of the MFMA tiles; log|det| relative 1e-11 and sign 1e-10 (CPU: 1e-15, 1e-14; the sums run over at most 8000
terms)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import prepare

pytestmark = pytest.mark.gpu

_CACHE = {}
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for _, F in _CACHE.values():
        F.free()
    _CACHE.clear()
    _REF.clear()


def _factor(hs, kind, shape, nmax, shift=0.0, **kw):
    key = (kind, shape, nmax, shift, tuple(sorted(kw.items())))
    if key not in _CACHE:
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        if shift:
            P["A"] = sp.csc_matrix(P["A"] - shift * sp.identity(P["A"].shape[0]))  # same pattern (the diagonal is stored), same tree
            P["A"].sort_indices()
        F = hs.factor(P["A"], P["nd"], P["nd_loc"], **(kw or dict(swlevel=0)))
        _CACHE[key] = (P, F)
    return _CACHE[key]


def _dense_ref(key, A):
    """(A^-1, sign, log|det|) by NumPy, once per matrix."""
    if key not in _REF:
        Ad = A.toarray()
        s, l = np.linalg.slogdet(Ad)
        _REF[key] = (np.linalg.inv(Ad), s, l)
    return _REF[key]


def _pattern(A):
    A = sp.csc_matrix(A)
    return A.indices, np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))


EXACT = [("poisson", (30, 27), 40), ("convdiff", (30, 27), 40), ("convdiff_helmholtz", (30, 27), 40), ("convdiff", (12, 12, 12), 100),
         ("helmholtz", (30, 27), 40), ("convdiff_helmholtz", (12, 12, 12), 100)]
BIG = ("convdiff", (20, 20, 20), 200)  # fronts with ni > 256 (the root separator has 400 DOFs), seven levels


def _check_selinv(hs, F, A, Zref, tag):
    rows, cols = _pattern(A)
    scale = np.abs(Zref).max()
    worst = 0.0
    for trans, op in ((0, F), (1, hs.transpose(F))):
        d, Z = hs.selinv(op)
        assert np.array_equal(Z.indptr, A.indptr) and np.array_equal(Z.indices, A.indices)
        ref = Zref[rows, cols] if trans == 0 else Zref[cols, rows]
        ed = np.abs(d - np.diag(Zref)).max() / scale
        ez = np.abs(Z.data - ref).max() / scale
        print(f"{tag} trans={trans}: diag error {ed:.1e}, pattern error {ez:.1e} (* max|A^-1| = {scale:.2e})")
        worst = max(worst, ed, ez)
    assert worst <= 1e-10, (tag, worst)
    return worst


@pytest.mark.parametrize("kind,shape,nmax", EXACT + [BIG])
def test_selected_inverse_against_the_dense_inverse(hs, kind, shape, nmax):
    """Measured on the MI355X (diagonal and pattern, trans = 0 and 1, in units of max|A^-1|): poisson 2.9e-15, convdiff 1.3e-15,
    convdiff_helmholtz (30, 27) 5.9e-19 (cond_1 = 4.4e6, max|A^-1| = 1.55e4), convdiff 12^3 2.2e-15, helmholtz 4.4e-15,
    convdiff_helmholtz 12^3 9.4e-16, convdiff 20^3 2.7e-15: the plain measure holds for every case, the ill-conditioned one included."""
    import torch

    P, F = _factor(hs, kind, shape, nmax)
    A = P["A"]
    n = A.shape[0]
    Zref, _, _ = _dense_ref((kind, shape, nmax, 0.0), A)
    _check_selinv(hs, F, A, Zref, f"{kind} {shape}")
    # device pointers on a side stream: the same bits as the host-pointer call
    d0, Z0 = hs.selinv(F)
    dev = torch.device("cuda:0")
    cplx = F.dtype.kind == "c"
    tdt = torch.complex128 if cplx else torch.float64
    dd = torch.zeros(n, dtype=tdt, device=dev)
    dz = torch.zeros(A.nnz, dtype=tdt, device=dev)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        hs._lib.check(hs._lib.lib().hs_selinv(F._h, 0, C.c_void_p(dd.data_ptr()), C.c_void_p(dz.data_ptr()), 1, 0, C.c_void_p(s.cuda_stream)))
    s.synchronize()
    assert np.array_equal(dd.cpu().numpy(), d0) and np.array_equal(dz.cpu().numpy(), Z0.data)
    # diagonal only / pattern only
    assert np.array_equal(hs.selinv_diag(F), d0)
    dn, Zn = hs.selinv(F, diag=False)
    assert dn is None and np.array_equal(Zn.data, Z0.data)


def test_small_budget_cuts_levels_into_batches(hs):
    """A budget of one byte puts every front into a batch of its own (a level of 2^k fronts becomes 2^k batches, each followed by its
    subtree); a budget of half the unbatched peak cuts only the wide levels.  A front's arithmetic does not depend on which fronts share
    its launches -- the grouped GEMM sums every output element over K in the same order whatever tile shape the launcher picks for the
    list -- so the results are bitwise those of the unbatched run."""
    kind, shape, nmax = BIG
    P, F = _factor(hs, kind, shape, nmax)
    Zref, _, _ = _dense_ref((kind, shape, nmax, 0.0), P["A"])
    scale = np.abs(Zref).max()
    d0, Z0 = hs.selinv(F)
    i0 = hs.selinv_info(F)
    nlev = max(F.node_info(k)[2] for k in range(F.nnodes))
    assert i0["batches"] == nlev, (i0, nlev)  # the default budget holds every level of this problem at once
    d1, Z1 = hs.selinv(F, budget=1)
    i1 = hs.selinv_info(F)
    assert i1["batches"] == F.nnodes and F.nnodes >= 2 ** (nlev - 1) + 3  # every level below the second in at least 4 batches
    assert i1["flops"] == i0["flops"] and i1["peak_bytes"] < i0["peak_bytes"]
    dd, dz = np.abs(d1 - d0).max() / scale, np.abs(Z1.data - Z0.data).max() / scale
    print(f"batched vs unbatched: diag {dd:.1e}, pattern {dz:.1e} (* max|A^-1|); bitwise equal: {np.array_equal(d1, d0) and np.array_equal(Z1.data, Z0.data)}; "
          f"batches {i0['batches']} -> {i1['batches']}, peak scratch {i0['peak_bytes'] / 2**20:.0f} -> {i1['peak_bytes'] / 2**20:.0f} MiB")
    assert np.array_equal(d1, d0) and np.array_equal(Z1.data, Z0.data)
    # a budget in between: some levels whole, the wide ones cut
    mid = int(i0["peak_bytes"] // 2)
    d2, Z2 = hs.selinv(F, budget=mid)
    i2 = hs.selinv_info(F)
    assert nlev < i2["batches"] < F.nnodes, i2
    print(f"budget {mid / 2**20:.0f} MiB: batches {i2['batches']}, peak scratch {i2['peak_bytes'] / 2**20:.0f} MiB")
    assert np.array_equal(d2, d0) and np.array_equal(Z2.data, Z0.data)


def _check_logabsdet(hs, F, sref, lref, tag):
    la, sign = hs.logabsdet(F)
    print(f"{tag}: log|det| {la:.10g} (ref {lref:.10g}, rel {abs(la - lref) / max(1.0, abs(lref)):.1e}), sign {sign} (ref {sref}, diff {abs(sign - sref):.1e})")
    assert abs(la - lref) <= 1e-11 * max(1.0, abs(lref)), (tag, la, lref)
    assert abs(sign - sref) <= 1e-10, (tag, sign, sref)
    assert hs.logabsdet(F) == (la, sign)  # fixed-order reductions: the same bits
    return la, sign


@pytest.mark.parametrize("kind,shape,nmax", EXACT + [BIG])
def test_logabsdet_against_slogdet(hs, kind, shape, nmax):
    P, F = _factor(hs, kind, shape, nmax)
    _, sref, lref = _dense_ref((kind, shape, nmax, 0.0), P["A"])
    la, sign = _check_logabsdet(hs, F, sref, lref, f"{kind} {shape}")
    # transpose: the same determinant; adjoint: the conjugate
    assert hs.logabsdet(hs.transpose(F)) == (la, sign)
    assert hs.logabsdet(hs.adjoint(F)) == (la, np.conj(sign) if F.dtype.kind == "c" else sign)
    if F.dtype.kind == "c":
        ld = hs.logdet(F)
        assert ld.real == la and abs(np.exp(1j * ld.imag) - sign) <= 1e-12 and -np.pi < ld.imag <= np.pi
    elif sign > 0:
        assert hs.logdet(F) == la
    if abs(lref) < 600:
        assert hs.det(F) == pytest.approx(sref * np.exp(lref), rel=1e-8)


INDEFINITE = [("poisson", (30, 27), 40, 0.35, -1.0), ("poisson", (30, 27), 40, 0.7, 1.0), ("convdiff", (12, 12, 12), 100, 1.0, -1.0)]


@pytest.mark.parametrize("kind,shape,nmax,sigma,sign", INDEFINITE)
def test_logabsdet_of_real_indefinite_matrices(hs, kind, shape, nmax, sigma, sign):
    """A - sigma I on the pattern and tree of A: negative pivots and rows moved by partial pivoting; a wrong parity flips the sign."""
    P, F = _factor(hs, kind, shape, nmax, shift=sigma)
    Zref, sref, lref = _dense_ref((kind, shape, nmax, sigma), P["A"])
    assert sref == sign
    la, sg = _check_logabsdet(hs, F, sref, lref, f"{kind} {shape} - {sigma} I")
    if sg < 0:
        with pytest.raises(ValueError, match="DomainError"):
            hs.logdet(F)
    moved = sum(int((F.node_blocks(k)["rperm"] != np.arange(F.node_info(k)[0])).sum()) for k in range(F.nnodes))
    print(f"rows moved by pivoting: {moved}")
    assert moved > 0
    _check_selinv(hs, F, P["A"], Zref, f"{kind} {shape} - {sigma} I")


def _redo_matrix(hs, n=20, nmax=100):
    """The construction of `redo_matrix` in tests/test_lu_paths_gpu.py: a 7-point pattern on an n^3 grid, diagonally dominant except among
    the DOFs of the root separator, where the diagonal is tiny and the couplings to z +- 1 dominate (+10 up, -10 down).  A z-neighbour
    sits 2n rows away in the root front -- outside the 32-row diagonal block -- so optimistic pivoting gives up on the root level, which is
    redone with tournament pivoting."""
    N = n ** 3
    g = np.arange(N)
    x, y, z = g % n, (g // n) % n, g // (n * n)
    sep = (x == n // 2 - 1) | (x == n // 2)
    rows, cols, vals = [g], [g], [np.where(sep, 1e-2, 6.5)]
    for d, ok in ((1, x < n - 1), (n, y < n - 1), (n * n, z < n - 1)):
        i = g[ok]
        j = i + d
        both = sep[i] & sep[j] & (d == n * n)
        rows += [i, j]
        cols += [j, i]
        vals += [np.where(both, 10.0, -1.0), np.where(both, -10.0, -1.0)]
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    return A, hs.problems.grid_nested_dissection((n, n, n), nmax)


@pytest.mark.parametrize("cplx", [False, True])
def test_logabsdet_after_a_level_was_redone_with_tournament_pivoting(hs, cplx, capfd):
    A0, nd = _redo_matrix(hs)
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    nd = hs.permuted(nd, hs.invperm(perm))
    A = (A0 * (1 + 0.5j) + 0.1j * sp.identity(A0.shape[0])) if cplx else A0
    A = sp.csc_matrix(A[perm - 1][:, perm - 1])
    capfd.readouterr()
    F = hs.factor(A, nd, nd_loc, swlevel=0, verbose=True)
    err = capfd.readouterr().err
    assert "redoing the level with tournament pivoting" in err
    sref, lref = np.linalg.slogdet(A.toarray())
    _check_logabsdet(hs, F, sref, lref, f"redone level, complex={cplx}")
    F.free()


CKW = dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, leafsize=32)
# the last case flags every level (swlevel = depth of the tree, set in the test): with mf = 1 every branch is then a matrix-free front whose D
# is expanded and eliminated densely -- the fronts hs_logabsdet reads through their own buffers
COMPRESSED = [("convdiff", (20, 20, 20), 200, CKW), ("convdiff_helmholtz", (20, 20, 20), 200, CKW),
              ("poisson", (16, 16, 16), 512, dict(swlevel=None, swsize=8, atol=1e-6, rtol=1e-6, leafsize=128))]


@pytest.mark.parametrize("mf", [0, 1])
@pytest.mark.parametrize("kind,shape,nmax,kw", COMPRESSED)
def test_compressed_factorization_logabsdet_is_consistent_and_selinv_refuses(hs, kind, shape, nmax, kw, mf):
    """det(F) = prod det(D_front): hs_logabsdet against the sum of numpy.linalg.slogdet over D = P'LU of every front, rebuilt from the
    exported LU and permutation.  How far log|det F| is from log|det A| is printed, not asserted: F approximates A to the compression
    tolerance only."""
    kw = dict(kw)
    if kw["swlevel"] is None:
        kw["swlevel"] = hs.depth(prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")["nd"])
    P, F = _factor(hs, kind, shape, nmax, mf=bool(mf), **kw)
    flow = hs._lib.i64 * 8
    info = flow()
    hs._lib.check(hs._lib.lib().hs_flow_info(F._h, info))
    assert info[3] > 0  # fronts with low-rank Gauss transforms
    if kw["leafsize"] == 128:
        assert (info[1] > 0) == bool(mf)  # matrix-free fronts exactly in the mf flow
    lref, sref = 0.0, 1.0
    for k in range(F.nnodes):
        LU, rp = F.node_lu(k)
        ni = LU.shape[0]
        D = np.empty_like(LU)
        D[rp] = (np.tril(LU, -1) + np.eye(ni)) @ np.triu(LU)  # (P D)[i] = D[rperm[i]]
        s, l = np.linalg.slogdet(D)
        lref += l
        sref = sref * s
    la, _ = _check_logabsdet(hs, F, sref, lref, f"compressed {kind} {shape} mf={mf} (matrix-free fronts: {info[1]})")
    _, l_a = np.linalg.slogdet(P["A"].toarray())
    print(f"  log|det F| - log|det A| = {la - l_a:.2e} (F approximates A to atol = rtol = 1e-6)")
    with pytest.raises(hs.UnsupportedError, match="low-rank"):
        hs.selinv(F)
    b = P["b"]
    assert np.array_equal(F.solve(b), F.solve(b))  # the refusal did no harm


def test_refusals(hs):
    import torch

    L = hs._lib.lib()
    la, sg = C.c_double(), (C.c_double * 2)()
    # HSS interior blocks (mf = 2): no LU to read
    P2 = prepare(hs, (20, 20, 20), kind="convdiff", nmax=200, rhs="randn")
    F2 = hs.factor(P2["A"], P2["nd"], P2["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.logabsdet(F2)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.selinv(F2)
    F2.free()
    # rank 0 of a two-rank plan
    P = prepare(hs, (16, 16), kind="convdiff", nmax=20, rhs="randn")
    be = hs.dist.HipBackend(P["A"], P["nd"], P["nd_loc"], rank=0, nranks=2, device=torch.device("cuda:0"), swlevel=0)
    n = P["A"].shape[0]
    d = np.zeros(n)
    assert L.hs_logabsdet(be._h, C.byref(la), sg) == hs._lib.HS_ERR_UNSUPPORTED and b"ranks" in L.hs_last_error()
    assert L.hs_selinv(be._h, 0, d.ctypes.data, None, 0, 0, None) == hs._lib.HS_ERR_UNSUPPORTED and b"ranks" in L.hs_last_error()
    del be
    # argument errors on an exact factorization
    P, F = _factor(hs, "convdiff", (30, 27), 40)
    n = P["A"].shape[0]
    d = np.zeros(n)
    for trans in (2, -1):
        assert L.hs_selinv(F._h, trans, d.ctypes.data, None, 0, 0, None) == hs._lib.HS_ERR_ARGUMENT and b"trans" in L.hs_last_error()
    assert L.hs_selinv(F._h, 0, d.ctypes.data, None, 2, 0, None) == hs._lib.HS_ERR_ARGUMENT and b"where" in L.hs_last_error()
    assert L.hs_selinv(F._h, 0, None, None, 0, 0, None) == hs._lib.HS_ERR_ARGUMENT and b"NULL" in L.hs_last_error()
    assert L.hs_logabsdet(F._h, None, sg) == hs._lib.HS_ERR_ARGUMENT
    with pytest.raises(ValueError):
        hs.selinv(F, diag=False, pattern=False)
    # a plan that was analyzed but not factored
    plan = C.c_void_p()
    A = sp.csc_matrix(P["A"])
    flat = hs.flatten_tree(P["nd"], P["nd_loc"])
    t = hs._lib.hs_tree()
    t.nnodes = flat["nnodes"]
    keep = []
    for k in ("left", "right", "int_ptr", "int_idx", "bnd_ptr", "bnd_idx", "iloc_ptr", "iloc_idx", "bloc_ptr", "bloc_idx"):
        a = np.ascontiguousarray(flat[k], dtype=np.int64)
        keep.append(a)
        setattr(t, k, a.ctypes.data_as(hs._lib.p_i64))
    o = hs.SolverOptions(swlevel=0).to_c()
    cp, rv = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1, np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    hs._lib.check(L.hs_analyze(0, n, cp.ctypes.data_as(hs._lib.p_i64), rv.ctypes.data_as(hs._lib.p_i64), C.byref(t), C.byref(o), 0, 1, C.byref(plan)))
    assert L.hs_logabsdet(plan, C.byref(la), sg) == hs._lib.HS_ERR_ARGUMENT and b"factorization" in L.hs_last_error()
    assert L.hs_selinv(plan, 0, d.ctypes.data, None, 0, 0, None) == hs._lib.HS_ERR_ARGUMENT
    L.hs_free(plan)


def test_adjoint_forms_solves_untouched_and_reproducible(hs):
    kind, shape, nmax = "convdiff_helmholtz", (12, 12, 12), 100
    P, F = _factor(hs, kind, shape, nmax)
    A = P["A"]
    Zref, _, _ = _dense_ref((kind, shape, nmax, 0.0), A)
    rows, cols = _pattern(A)
    scale = np.abs(Zref).max()
    rng = np.random.default_rng(5)
    b = rng.standard_normal(A.shape[0]) + 1j * rng.standard_normal(A.shape[0])
    x0, xt0 = F.solve(b), F.solve(b, "T")
    d, Z = hs.selinv(F)
    assert np.array_equal(F.solve(b), x0) and np.array_equal(F.solve(b, "T"), xt0)  # the factors are only read
    d2, Z2 = hs.selinv(F)
    assert np.array_equal(d, d2) and np.array_equal(Z.data, Z2.data)  # two calls, the same bits
    dt, Zt = hs.selinv(hs.transpose(F))
    da, Za = hs.selinv(hs.adjoint(F))
    assert np.array_equal(da, dt.conj()) and np.array_equal(Za.data, Zt.data.conj())
    assert np.abs(Za.data - Zref[cols, rows].conj()).max() <= 1e-10 * scale and np.abs(da - np.diag(Zref).conj()).max() <= 1e-10 * scale
    # trace(A^-1 A) = n from the pattern values alone
    assert abs((Zt.data * A.data).sum() - A.shape[0]) <= 1e-8 * A.shape[0]


def test_root_that_keeps_a_boundary(hs):
    """A tree whose root keeps a boundary (the construction of test_root_with_boundary in tests/test_factor_gpu.py): the boundary is
    eliminated by the handle's pseudo-root, an ordinary front for the determinant and the selected inversion."""
    A, b, nd = hs.problems.make_problem((12, 10), kind="convdiff", nmax=16, rhs="randn")
    sub = nd.left
    dofs = np.sort(np.concatenate([x.int for x in hs.postorder_nodes(sub)] + [sub.bnd]))
    remap = np.zeros(A.shape[0] + 1, dtype=np.int64)
    remap[dofs] = np.arange(1, len(dofs) + 1)
    for x in hs.postorder_nodes(sub):
        x.int, x.bnd = remap[x.int], remap[x.bnd]
    As = A[dofs - 1][:, dofs - 1].tocsc()
    As.sort_indices()
    sub, sub_loc = hs.symfact(sub)
    assert len(sub.bnd) > 0
    F = hs.factor(As, sub, sub_loc, swlevel=0)
    Ad = As.toarray()
    _check_selinv(hs, F, As, np.linalg.inv(Ad), "root with boundary")
    s, l = np.linalg.slogdet(Ad)
    _check_logabsdet(hs, F, s, l, "root with boundary")
    F.free()


def test_plain_c_pointer_calls(hs):
    P, F = _factor(hs, "convdiff", (12, 12, 12), 100)
    A = P["A"]
    n = A.shape[0]
    L = hs._lib.lib()
    la, sg = C.c_double(), (C.c_double * 2)()
    hs._lib.check(L.hs_logabsdet(F._h, C.byref(la), sg))
    assert (la.value, sg[0]) == hs.logabsdet(F) and sg[1] == 0.0
    d = np.zeros(n)
    z = np.zeros(A.nnz)
    hs._lib.check(L.hs_selinv(F._h, 1, d.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), 0, 0, None))
    dt, Zt = hs.selinv(hs.transpose(F))
    assert np.array_equal(d, dt) and np.array_equal(z, Zt.data)
    out = (C.c_double * 4)()
    hs._lib.check(L.hs_selinv_info(F._h, out))
    assert out[0] > 0 and out[1] > 0 and out[2] > 0 and out[3] >= 1
