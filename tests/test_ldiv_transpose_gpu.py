"""ldiv!(transpose(F), B) and ldiv!(adjoint(F), B) on the MI355X (kernels_solve_t.hip): the same factors, read along their columns.

The test problems of the rest of the suite are symmetric (Poisson) or complex symmetric (Helmholtz), so A^T = A there; `convdiff` and
`convdiff_helmholtz` (problems.py) are not, and tell A from A^T and A^H."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from helpers import prepare, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _rand(n, k, cplx, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, k))
    if cplx:
        B = B + 1j * rng.standard_normal((n, k))
    return B


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cached_factors():
    yield
    for _, F, _ in _CACHE.values():
        F.free()
    _CACHE.clear()


def _exact(hs, kind, shape, nmax):
    key = (kind, shape, nmax)
    if key not in _CACHE:
        P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
        F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
        _CACHE[key] = (P, F, spla.splu(P["A"]))
    return _CACHE[key]


# 2-D, and 3-D with fronts above 256 columns and ragged interior sizes
EXACT = [("convdiff", (30, 27), 40), ("convdiff_helmholtz", (30, 27), 40), ("convdiff", (24, 24, 24), 300), ("convdiff_helmholtz", (24, 24, 24), 300)]


@pytest.mark.parametrize("kind,shape,nmax", EXACT)
def test_transposed_and_adjoint_solves_match_splu(hs, kind, shape, nmax):
    P, F, lu = _exact(hs, kind, shape, nmax)
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    ni_max = max(F.node_info(i)[0] for i in range(F.nnodes))
    if len(shape) == 3:
        assert ni_max > 256 and ni_max % 256 != 0
    for nrhs in (1, 3):
        B = _rand(n, nrhs, cplx, nrhs)
        b = B[:, 0] if nrhs == 1 else B
        xt = hs.ldiv(hs.transpose(F), b)
        xh = hs.ldiv(hs.adjoint(F), b)
        assert relerr(xt, lu.solve(b, trans="T")) < TOL
        assert relerr(xh, lu.solve(b, trans="H")) < TOL
        assert relerr(xt, lu.solve(b)) > 1e-3  # A^T is not A here
        # two calls: bitwise the same
        assert np.array_equal(xt, hs.ldiv(hs.transpose(F), b)) and np.array_equal(xh, hs.ldiv(hs.adjoint(F), b))
        assert np.array_equal(xt, F.solve(b, trans="T")) and np.array_equal(xh, F.solve(b, trans="C"))
    # leading dimensions larger than n, C aliasing B
    L = hs._lib.lib()
    fn = L.hs_ldiv_t_z if cplx else L.hs_ldiv_t_d
    B = _rand(n, 3, cplx, 7)
    ld = n + 5
    Bp = np.zeros((ld, 3), dtype=F.dtype, order="F")
    Bp[:n] = B
    Cp = np.full((ld + 3, 3), 7.0, dtype=F.dtype, order="F")
    for trans, tr in ((1, "T"), (2, "H")):
        hs._lib.check(fn(F._h, trans, Cp.ctypes.data_as(hs._lib.p_f64), ld + 3, Bp.ctypes.data_as(hs._lib.p_f64), ld, n, 3))
        ref = lu.solve(B, trans=tr)
        assert relerr(Cp[:n], ref) < TOL and np.all(Cp[n:] == 7.0)
        Bq = Bp.copy(order="F")
        hs._lib.check(fn(F._h, trans, Bq.ctypes.data_as(hs._lib.p_f64), ld, Bq.ctypes.data_as(hs._lib.p_f64), ld, n, 3))
        assert np.array_equal(Bq[:n], Cp[:n]) and np.all(Bq[n:] == 0)
    Bq = B.copy(order="F")
    assert hs.ldiv(Bq, hs.transpose(F), Bq) is Bq and relerr(Bq, lu.solve(B, trans="T")) < TOL
    assert F.stats()["t_solve"] > 0
    # trans = 0 is hs_ldiv_*
    X0 = np.empty_like(B, order="F")
    Bf = np.asfortranarray(B)
    hs._lib.check(fn(F._h, 0, X0.ctypes.data_as(hs._lib.p_f64), n, Bf.ctypes.data_as(hs._lib.p_f64), n, n, 3))
    assert np.array_equal(X0, hs.ldiv(F, B))


def test_symmetric_problems_identities(hs):
    """Helmholtz is complex symmetric: F^T \\ b = F \\ b (different kernels on the same factors) and F^H \\ b = conj(F \\ conj(b))."""
    P, F, _ = _exact(hs, "helmholtz", (20, 20, 20), 300)
    b = _rand(P["A"].shape[0], 1, True, 3)[:, 0]
    x = hs.ldiv(F, b)
    assert relerr(hs.ldiv(hs.transpose(F), b), x) < TOL
    assert relerr(hs.ldiv(hs.adjoint(F), b), np.conj(hs.ldiv(F, np.conj(b)))) < TOL


COMPRESSED = [
    ("tol1e-4", "convdiff_helmholtz", (24, 24, 24), 300, dict(swlevel=2, swsize=8, atol=1e-4, rtol=1e-4)),
    ("tol1e-8", "convdiff", (24, 24, 24), 300, dict(swlevel=3, swsize=8, atol=1e-8, rtol=1e-8)),
    ("split", "convdiff", (24, 24, 24), 300, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, split_size=256)),
    ("mf-dense-D", "convdiff_helmholtz", (24, 24, 24), 300, dict(swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=True, leafsize=128)),
]


@pytest.mark.parametrize("label,kind,shape,nmax,kw", COMPRESSED, ids=[c[0] for c in COMPRESSED])
def test_compressed_flows_adjoint_identity(hs, label, kind, shape, nmax, kw):
    """For the approximate operator F^-1 of any tolerance: <v, F^-1 u> = <F^-H v, u> and v^T F^-1 u = (F^-T v)^T u."""
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], **kw)
    assert hs.maxrank(F) > 0  # low-rank Gauss transforms are in the solve
    n = P["A"].shape[0]
    cplx = F.dtype.kind == "c"
    u, v = _rand(n, 1, cplx, 11)[:, 0], _rand(n, 1, cplx, 12)[:, 0]
    Fu = hs.ldiv(F, u)
    scale = np.linalg.norm(v) * np.linalg.norm(Fu)
    assert abs(np.vdot(v, Fu) - np.vdot(hs.ldiv(hs.adjoint(F), v), u)) <= 1e-11 * scale
    assert abs(np.dot(v, Fu) - np.dot(hs.ldiv(hs.transpose(F), v), u)) <= 1e-11 * scale
    lu = spla.splu(P["A"])
    b = P["b"]
    e = relerr(hs.ldiv(F, b), lu.solve(b))
    et = relerr(hs.ldiv(hs.transpose(F), b), lu.solve(b, trans="T"))
    print(f"{label}: F\\b {e:.2e}  F^T\\b {et:.2e}  maxrank {hs.maxrank(F)}")
    assert et <= 10 * e + 1e-12
    F.free()


@pytest.mark.parametrize("kind", ["convdiff", "convdiff_helmholtz"])
def test_transposed_dataflow_sweeps_agree_with_the_launch_per_step_sweeps(hs, kind, tmp_path):
    """The transposed sweeps run as ONE dataflow launch per level (t_flow_kernel); HS_SOLVE_FLOW=0 (read once per process: a child process)
    selects the launch-per-step transposed sweeps (t_diag_kernel + t_update_kernel).  Two implementations on the same factors: they must agree,
    fronts above 256 columns with ragged ni included, over repeated solves (the exchange vectors are re-armed by every sweep, ldiv! in between)."""
    shape, nmax = (24, 24, 24), 300
    P, F, lu = _exact(hs, kind, shape, nmax)
    B = _rand(P["A"].shape[0], 3, kind != "convdiff", 5)
    for _ in range(3):
        X = hs.ldiv(hs.transpose(F), B)
        XH = hs.ldiv(hs.adjoint(F), B)
        hs.ldiv(F, B)  # a dataflow ldiv! in between
        assert relerr(X, lu.solve(B, trans="T")) < TOL and relerr(XH, lu.solve(B, trans="H")) < TOL
    np.save(tmp_path / "B.npy", B)
    code = f"""
import sys, numpy as np
sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r}); sys.path.insert(0, {os.path.dirname(os.path.abspath(__file__))!r})
import hsamd
from helpers import prepare
hs = hsamd.load()
P = prepare(hs, {shape!r}, kind={kind!r}, nmax={nmax}, rhs="randn")
F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
B = np.load({str(tmp_path / "B.npy")!r})
for _ in range(3):
    X, XH = hs.ldiv(hs.transpose(F), B), hs.ldiv(hs.adjoint(F), B)
    hs.ldiv(F, B)
np.save({str(tmp_path / "X0.npy")!r}, X)
np.save({str(tmp_path / "XH0.npy")!r}, XH)
"""
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, HS_SOLVE_FLOW="0"), timeout=300)
    X0, XH0 = np.load(tmp_path / "X0.npy"), np.load(tmp_path / "XH0.npy")
    assert relerr(X0, lu.solve(B, trans="T")) < TOL and relerr(XH0, lu.solve(B, trans="H")) < TOL
    assert relerr(X, X0) < 1e-11 and relerr(XH, XH0) < 1e-11
    assert not np.array_equal(X, X0)  # (different reduction orders: a bitwise match would mean one implementation ran twice)


@pytest.mark.parametrize("shape,nmax,kind", [((7, 5), 6, "convdiff"), ((9, 9), 12, "convdiff_helmholtz"), ((6, 6, 6), 30, "convdiff"), ((3, 3), 100, "convdiff"), ((40, 3), 9, "convdiff")])
def test_small_and_ragged_trees(hs, shape, nmax, kind):
    P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
    lu = spla.splu(P["A"])
    assert relerr(hs.ldiv(hs.transpose(F), P["b"]), lu.solve(P["b"], trans="T")) < TOL
    assert relerr(hs.ldiv(hs.adjoint(F), P["b"]), lu.solve(P["b"], trans="H")) < TOL


def test_root_with_boundary(hs):
    A, b, nd = hs.problems.make_problem((12, 10), kind="convdiff", nmax=16, rhs="randn")
    sub = nd.left
    dofs = np.sort(np.concatenate([x.int for x in hs.postorder_nodes(sub)] + [sub.bnd]))
    remap = np.zeros(A.shape[0] + 1, dtype=np.int64)
    remap[dofs] = np.arange(1, len(dofs) + 1)
    for x in hs.postorder_nodes(sub):
        x.int, x.bnd = remap[x.int], remap[x.bnd]
    As = A[dofs - 1][:, dofs - 1].tocsc()
    bs = b[dofs - 1]
    sub, sub_loc = hs.symfact(sub)
    assert len(sub.bnd) > 0
    F = hs.factor(As, sub, sub_loc, swlevel=0)
    assert relerr(hs.ldiv(hs.transpose(F), bs), spla.splu(As).solve(bs, trans="T")) < TOL


def test_device_api_on_a_side_stream(hs):
    """hs_ldiv_dev_t_* on torch device tensors, on a non-default stream: bitwise the host API's result."""
    import torch

    P, F, _ = _exact(hs, "convdiff_helmholtz", (24, 24, 24), 300)
    n = P["A"].shape[0]
    B = _rand(n, 3, True, 9)
    L = hs._lib.lib()
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    for trans, wrap in ((1, hs.transpose), (2, hs.adjoint)):
        ref = hs.ldiv(wrap(F), B)
        dB = torch.from_numpy(np.asfortranarray(B).T.copy()).to(dev)  # row r of dB = column r of B (column-major n x 3, ld n)
        dC = torch.empty_like(dB)
        with torch.cuda.stream(s):
            hs._lib.check(L.hs_ldiv_dev_t_z(F._h, trans, C.c_void_p(dC.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, 3, C.c_void_p(s.cuda_stream)))
        s.synchronize()
        assert np.array_equal(dC.cpu().numpy().T, ref)
        hs._lib.check(L.hs_ldiv_dev_t_z(F._h, trans, C.c_void_p(dB.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, 3, C.c_void_p(s.cuda_stream)))
        s.synchronize()
        assert np.array_equal(dB.cpu().numpy().T, ref)  # C aliasing B


def test_refusals(hs):
    L = hs._lib.lib()
    # a front that keeps D as an HSS matrix
    P = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, hss_min=1024)
    x = hs.ldiv(F, P["b"])  # the factorization itself is fine
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.ldiv(hs.transpose(F), P["b"])
    F.free()
    # mf = 2: every matrix-free interior block an HSS matrix
    P = prepare(hs, (24, 24, 24), kind="convdiff", nmax=300, rhs="randn")
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    with pytest.raises(hs.UnsupportedError, match="ULV"):
        hs.ldiv(hs.adjoint(F), P["b"])
    F.free()
    # argument errors of an exact factorization
    P, F, _ = _exact(hs, "convdiff", (30, 27), 40)
    n = P["A"].shape[0]
    b = np.asfortranarray(P["b"])
    assert L.hs_ldiv_t_d(F._h, 3, b.ctypes.data_as(hs._lib.p_f64), n, b.ctypes.data_as(hs._lib.p_f64), n, n, 1) == hs._lib.HS_ERR_ARGUMENT
    with pytest.raises(TypeError, match="MethodError"):
        hs.ldiv(hs.transpose(F), P["b"] + 1j)
    with pytest.raises(hs.DimensionMismatch):
        hs.ldiv(hs.transpose(F), P["b"][:-1])
    with pytest.raises(hs.DimensionMismatch):
        hs._lib.check(L.hs_ldiv_t_d(F._h, 1, b.ctypes.data_as(hs._lib.p_f64), n, b.ctypes.data_as(hs._lib.p_f64), n, n - 1, 1))
    assert np.all(np.isfinite(x))
