"""Host-side checks of hs_options.equilibrate: no device needed.

  * the NumPy restatement of the sweep rule (equil_mirror.equilibrate) terminates within its cap and ends with every row and column
    maximum in [0.5, 2), on D1 A D2 with random power-of-two diagonals (exponents in +-20 and +-40) for Poisson 12^3, convdiff 20^3,
    convdiff_helmholtz 30 x 27 and Helmholtz 12^3; D A D of a symmetric A gives er == ec; a stored zero row keeps exponent 0;
  * hs_options_default leaves the field 0, the field is appended, the new symbols are exported, the Python layer carries the option;
  * hs_plan refuses the option over several ranks."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import equil_mirror as EM

CASES = [((12, 12, 12), "poisson"), ((20, 20, 20), "convdiff"), ((30, 27), "convdiff_helmholtz"), ((12, 12, 12), "helmholtz")]


@functools.lru_cache(maxsize=None)
def matrix(shape, kind):
    import hsamd

    return hsamd.load().problems.grid_matrix(shape, kind)


@pytest.mark.parametrize("span", [20, 40])
@pytest.mark.parametrize("shape,kind", CASES)
def test_mirror_terminates_with_maxima_in_range(shape, kind, span):
    B, _, _ = EM.badly_scaled(matrix(shape, kind), 11 + span, span)
    er, ec, sweeps = EM.equilibrate(B)
    assert 2 <= sweeps < EM.MAX_SWEEPS, sweeps  # a fixed point, not the cap
    rows, cols, mag = EM.magnitudes(B)
    rmax, cmax = EM.maxima(rows, cols, mag, er.astype(np.int64), ec.astype(np.int64), B.shape[0])
    print(f"[equil mirror] {kind} {shape} +-{span}: {sweeps} sweeps, maxima in [{min(rmax.min(), cmax.min()):.3f}, {max(rmax.max(), cmax.max()):.3f}]")
    assert rmax.min() >= 0.5 and cmax.min() >= 0.5 and rmax.max() < 2.0 and cmax.max() < 2.0
    # the scaled matrix is exact: scaling back gives B's bits
    Bs = EM.scaled(B, er, ec)
    assert np.array_equal(EM.scaled(Bs, -er, -ec).data, B.data)
    # and a second run on the scaled matrix moves nothing
    er2, ec2, sweeps2 = EM.equilibrate(Bs)
    assert sweeps2 == 1 and not er2.any() and not ec2.any()


@pytest.mark.parametrize("shape,kind", [((12, 12, 12), "poisson"), ((12, 12, 12), "helmholtz")])
def test_mirror_symmetric_input_gives_equal_exponents(shape, kind):
    A = matrix(shape, kind)
    assert (A != A.T).nnz == 0
    e = np.random.default_rng(5).integers(-40, 41, A.shape[0]).astype(np.int32)
    B = EM.scaled(A, e, e)
    assert (B != B.T).nnz == 0
    er, ec, _ = EM.equilibrate(B)
    assert np.array_equal(er, ec)
    Bs = EM.scaled(B, er, ec)
    assert (Bs != Bs.T).nnz == 0


def test_mirror_zero_row_keeps_exponent_zero():
    A = sp.lil_matrix(matrix((6, 6), "poisson") * 1024.0)
    A[7, :] = 0.0
    A = sp.csc_matrix(A)
    Az = sp.csc_matrix(matrix((6, 6), "poisson") * 1024.0)
    Az.data[Az.indices == 7] = 0.0  # the same with the zeros stored
    for M in (A, Az):
        er, ec, sweeps = EM.equilibrate(M)
        assert er[7] == 0 and sweeps < EM.MAX_SWEEPS
        assert np.all(er[np.arange(36) != 7] < 0)


def test_step_rule():
    m = np.array([0.0, 0.25, 0.49, 0.5, 1.0, 1.99, 2.0, 3.9, 4.0, 2.0 ** -7, 2.0 ** 9, np.inf, np.nan, 5e-324])
    want = np.array([0, 1, 1, 0, 0, 0, -1, -1, -1, 3, -5, 0, 0, 537])
    assert np.array_equal(EM.step(m), want)


def test_option_default_exports_and_python_layer():
    import hsamd

    hs = hsamd.load()
    L = hs._lib.lib()
    o = hs._lib.hs_options()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    L.hs_options_default(C.byref(o))
    assert o.equilibrate == 0 and o.symmetric == 0
    for name in ("hs_equil_info", "hs_equil_scales"):
        assert name in hs._lib.EXPORTS
        getattr(L, name)
    Co = hs._lib.hs_options
    assert Co.equilibrate.offset == Co.symmetric.offset + 1 and Co.symmetric.offset == 80 and Co.seed.offset == 72
    so = hs.SolverOptions(equilibrate=True)
    hs.chkopts(so)
    assert so.to_c().equilibrate == 1 and hs.SolverOptions().to_c().equilibrate == 0
    assert so.copy().equilibrate is True and so.copy(equilibrate=False).equilibrate is False
    assert so.copy(swlevel=2, symmetric=True).to_c().equilibrate == 1
    with pytest.raises(TypeError):
        hs.SolverOptions(equilibrated=True)
    assert callable(hs.equil_info) and callable(hs.equil_scales)


def test_plan_refuses_several_ranks():
    """hs_plan needs no device: hs_options.equilibrate with two ranks is HS_ERR_UNSUPPORTED, with one rank it plans."""
    import hsamd

    hs = hsamd.load()
    A, _, nd = hs.problems.make_problem((8, 8, 8), kind="poisson")
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    A = A[perm - 1][:, perm - 1].tocsc()
    nd = hs.permuted(nd, hs.invperm(perm))
    with pytest.raises(hs._lib.UnsupportedError) as ei:
        hs.dist.plan_only(A, nd, nd_loc, rank=0, nranks=2, equilibrate=True)
    assert "equilibrate" in str(ei.value)
    h = hs.dist.plan_only(A, nd, nd_loc, rank=0, nranks=1, equilibrate=True)
    out = np.zeros(6, dtype=np.int64)
    assert L_ok(hs, h, out) and out[0] == 1 and out[1] == 0
    hs._lib.lib().hs_free(h)


def L_ok(hs, h, out):
    return hs._lib.lib().hs_equil_info(h, out.ctypes.data_as(hs._lib.p_i64)) == 0
