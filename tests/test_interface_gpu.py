"""Schur-complement mode on the device: the triangular product kernel alone (exact integer data, random data against NumPy), the interface
matrix of real handles against their own exported LU and against the dense Schur complement, the bits of condense; solve; expand against
hs.ldiv_block_t, what the two outer phases mean (against SuperLU on A_ii), and the refusals."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from helpers import prepare
from interface_cases import dense_schur, interface_problem

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
EXACT = [("convdiff", (30, 27), 40), ("convdiff_helmholtz", (30, 27), 40), ("convdiff_helmholtz", (24, 24, 24), 300)]
COMPRESSED_KW = dict(swlevel=2, swsize=8, atol=1e-4, rtol=1e-4)


@pytest.fixture(scope="module")
def handles(hs):
    """get(key) -> (P, F) of one of the module's handles, factored once and freed with the module: 'exact0..2', 'compressed' (24^3 at 1e-4),
    'plain' (an ordinary tree, nb = 0)."""
    cache = {}

    def get(key):
        if key not in cache:
            if key.startswith("exact"):
                kind, shape, nmax = EXACT[int(key[5:])]
                P = interface_problem(hs, kind, shape, nmax)
                F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
            elif key == "compressed":
                P = interface_problem(hs, "convdiff_helmholtz", (24, 24, 24), 300)
                F = hs.factor(P["A"], P["nd"], P["nd_loc"], **COMPRESSED_KW)
                assert hs.maxrank(F) > 0
            else:
                P = interface_problem(hs, "convdiff", (30, 27), 40, with_interface=False)
                F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
            cache[key] = (P, F)
        return cache[key]

    yield get
    for _, F in cache.values():
        F.free()


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def _gamma(k):
    return k * EPS / (1 - k * EPS)


def _pack(Lm, Um, ldl):
    nb = Lm.shape[0]
    LF = np.full((ldl, nb), 99.0, dtype=Lm.dtype, order="F")  # the rows past nb are never read: poison
    LF[:nb] = np.tril(Lm, -1) + np.triu(Um)
    return LF


def _lu_product(hs, LF, nb, rperm, lds, fill=7.0):
    cplx = LF.dtype.kind == "c"
    S = np.full((lds, nb), fill, dtype=LF.dtype, order="F")
    fl = C.c_double(-1.0)
    fn = hs._lib.lib().hsk_lu_product_z if cplx else hs._lib.lib().hsk_lu_product_d
    rp = np.ascontiguousarray(rperm, dtype=np.int32)
    hs._lib.check(fn(nb, LF.ctypes.data_as(hs._lib.p_f64), LF.shape[0], rp.ctypes.data_as(C.POINTER(C.c_int32)), S.ctypes.data_as(hs._lib.p_f64), lds, C.byref(fl)))
    return S, fl.value


def _placed(PS, rperm):
    S = np.empty_like(PS)
    S[rperm] = PS  # (P S)[i] = S[rperm[i]]
    return S


# ---- a: the kernel alone, exact data ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
@pytest.mark.parametrize("nb", [1, 3, 16, 17, 63, 64, 65, 255, 256, 257, 600])
def test_kernel_is_exact_on_small_integers(hs, nb, cplx):
    rng = np.random.default_rng(100 + nb)
    ints = lambda: rng.integers(-3, 4, (nb, nb)).astype(np.float64)  # noqa: E731
    Lm = np.tril(ints() + (1j * ints() if cplx else 0), -1) + np.eye(nb)
    Um = np.triu(ints() + (1j * ints() if cplx else 0))
    rperm = rng.permutation(nb)
    S, _ = _lu_product(hs, _pack(Lm, Um, nb + 5), nb, rperm, nb + 2)
    assert np.array_equal(S[:nb], _placed(Lm @ Um, rperm))
    assert (S[nb:] == 7.0).all()  # rows of S past nb are untouched


@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
def test_kernel_cuts_the_k_range(hs, cplx):
    nb = 1024
    rng = np.random.default_rng(5)
    LF = np.asfortranarray(_rand(rng, (nb, nb), cplx))
    _, flops = _lu_product(hs, LF, nb, np.arange(nb), nb)
    full = 2.0 * nb**3 * (4 if cplx else 1)
    print(f"executed flops / full product at nb = {nb}: {flops / full:.4f}")
    assert 0 < flops <= 0.5 * full


# ---- b: random data against NumPy on the same factors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
@pytest.mark.parametrize("nb", [65, 257, 600])
def test_kernel_on_random_data(hs, nb, cplx):
    rng = np.random.default_rng(200 + nb)
    Lm = np.tril(_rand(rng, (nb, nb), cplx), -1) + np.eye(nb)
    Um = np.triu(_rand(rng, (nb, nb), cplx))
    rperm = rng.permutation(nb)
    LF = _pack(Lm, Um, nb + 5)
    S, _ = _lu_product(hs, LF, nb, rperm, nb + 1)
    bound = _placed(2 * _gamma(nb) * (np.abs(Lm) @ np.abs(Um)), rperm)
    err = np.abs(S[:nb] - _placed(Lm @ Um, rperm))
    print(f"nb = {nb}: worst error / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    S2, _ = _lu_product(hs, LF, nb, rperm, nb + 1)
    assert np.array_equal(S, S2)  # two calls, the same bits


# ---- c: the interface matrix of real handles ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["exact0", "exact1", "exact2", "compressed"])
def test_schur_complement_of_a_handle(hs, handles, key):
    P, F = handles(key)
    idx = hs.interface_indices(F)
    nb = len(idx)
    assert np.array_equal(idx, P["iface"]) and nb == len(P["iface0"])
    S = hs.schur_complement(F)
    assert S.shape == (nb, nb) and S.dtype == F.dtype
    LU, rp = F.node_lu(F.nnodes)  # the pseudo-root: the node id after the user's tree
    assert LU.shape == (nb, nb)
    Lm, Um = np.tril(LU, -1) + np.eye(nb), np.triu(LU)
    bound = _placed(2 * _gamma(nb) * (np.abs(Lm) @ np.abs(Um)), rp)
    err = np.abs(S - _placed(Lm @ Um, rp))
    print(f"{key}: nb = {nb}, worst error / bound against the exported LU {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    if key != "compressed":
        ref, _ = dense_schur(P["A"], idx)
        d = np.max(np.abs(S - ref))
        print(f"{key}: max |S - dense Schur complement| = {d:.2e}, max |S| = {np.max(np.abs(ref)):.2e}")
        assert d <= 1e-10 * np.max(np.abs(ref))
    assert np.array_equal(hs.schur_complement(F), S)  # the same bits again
    Sd = hs.schur_complement(F, device=True)
    assert np.array_equal(Sd.cpu().numpy(), S)
    info = hs.interface_info(F)
    assert info["nb"] == nb and info["matrix_seconds"] > 0
    assert 0 < info["matrix_flops"] <= (4 if F.dtype.kind == "c" else 1) * 2.0 * (256 * -(-nb // 256)) ** 3  # never more than the full product padded to a 256-tile
    assert np.array_equal(hs.schur_complement(hs.transpose(F)), S.T)
    assert np.array_equal(hs.schur_complement(hs.adjoint(F)), S.conj().T)


def test_no_interface_gives_an_empty_matrix(hs, handles):
    _, F = handles("plain")
    assert len(hs.interface_indices(F)) == 0
    assert hs.schur_complement(F).shape == (0, 0)
    assert hs.interface_info(F)["nb"] == 0


# ---- d: condense; solve; expand has the bits of the one-call block solve --------------------------------------------------------------
def _wraps(hs, F):
    return (("N", F), ("T", hs.transpose(F)), ("H", hs.adjoint(F)))


@pytest.mark.parametrize("key", ["exact0", "exact1", "exact2", "compressed", "plain"])
def test_three_phases_have_the_bits_of_the_block_solve(hs, handles, key):
    P, F = handles(key)
    n = P["n"]
    rng = np.random.default_rng(7)
    for nrhs in (1, 17, 33, 70):
        B = np.asfortranarray(_rand(rng, (n, nrhs), F.dtype.kind == "c"))
        for name, Fw in _wraps(hs, F):
            ref = hs.ldiv_block_t(Fw, B)
            Cb = B.copy(order="F")
            out = hs.expand(Fw, hs.interface_solve(Fw, hs.condense(Fw, Cb)))
            assert out is Cb
            assert np.array_equal(Cb, ref), (key, name, nrhs)
    info = hs.interface_info(F)
    assert info["chunks"] == 3 and info["expand_seconds"] > 0 and info["condense_seconds"] > 0
    v = B[:, 0].copy()  # a vector is a block of one column
    assert np.array_equal(hs.expand(F, hs.interface_solve(F, hs.condense(F, v))), hs.ldiv_block_t(F, B[:, 0]))


def test_phases_on_device_tensors(hs, handles):
    import torch

    P, F = handles("exact2")
    n = P["n"]
    B = np.asfortranarray(_rand(np.random.default_rng(8), (n, 40), True))
    ref = hs.ldiv_block_t(hs.adjoint(F), B)
    dB = torch.from_numpy(B.T.copy()).to("cuda").t()  # n x 40, column-major on the device
    assert dB.stride(0) == 1
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = hs.expand(hs.adjoint(F), hs.interface_solve(hs.adjoint(F), hs.condense(hs.adjoint(F), dB)))
    s.synchronize()
    assert out is dB and np.array_equal(dB.cpu().numpy(), ref)
    with pytest.raises(ValueError, match="column-major"):
        hs.condense(F, torch.zeros((n, 2), dtype=torch.complex128, device="cuda"))


# ---- e: what condense and expand mean -------------------------------------------------------------------------------------------------
def _worst_col(X, R):
    return float(np.max(np.linalg.norm(X - R, axis=0) / np.linalg.norm(R, axis=0)))


@pytest.mark.parametrize("key", ["exact0", "exact1", "exact2"])
def test_condense_and_expand_against_superlu(hs, handles, key):
    """Both outer phases against SuperLU on A_ii, within 10 max(e0, eps) with e0 the worst-column error of hs.ldiv_block_t against SuperLU on
    the same handle.  Measured on the MI355X (e0 / condense / expand, worst over N, T, H): 30x27 convdiff 1.4e-15 / 1.0e-15 / 8.8e-16,
    30x27 convdiff_helmholtz 2.2e-14 / 1.6e-14 / 1.4e-14, 24^3 convdiff_helmholtz 1.9e-14 / 7.4e-15 / 7.8e-15."""
    P, F = handles(key)
    n, idx = P["n"], hs.interface_indices(F)
    cplx = F.dtype.kind == "c"
    rng = np.random.default_rng(11)
    B = np.asfortranarray(_rand(rng, (n, 5), cplx))
    Y = _rand(rng, (len(idx), 5), cplx)
    for name, Fw in _wraps(hs, F):
        M = {"N": P["A"], "T": P["A"].T, "H": P["A"].conj().T}[name].tocsc()
        e0 = _worst_col(hs.ldiv_block_t(Fw, B), spla.splu(M).solve(B))
        tol = 10 * max(e0, EPS)
        _, ii = dense_schur(M, idx)
        lu = spla.splu(M[ii][:, ii].tocsc())
        Mbi, Mib = M[idx][:, ii], M[ii][:, idx]
        Cb = hs.condense(Fw, B.copy(order="F"))
        eg = _worst_col(Cb[idx], B[idx] - Mbi @ lu.solve(B[ii]))
        Cb[idx] = Y
        hs.expand(Fw, Cb)
        ex = _worst_col(Cb[ii], lu.solve(B[ii] - Mib @ Y))
        print(f"{key} {name}: e0 = {e0:.2e}, condense {eg:.2e}, expand {ex:.2e} (bound {tol:.2e})")
        assert np.array_equal(Cb[idx], Y)  # expand leaves the interface rows alone
        assert eg <= tol and ex <= tol


# ---- f: refusals, outputs untouched ---------------------------------------------------------------------------------------------------
def _all_refused(hs, F, n, nb, code, trans=0):
    L = hs._lib.lib()
    z = F.dtype.kind == "c"
    sfx = "_z" if z else "_d"
    S = np.full((max(nb, 1), max(nb, 1)), 7.0, dtype=F.dtype, order="F")
    assert getattr(L, "hs_interface_matrix" + sfx)(F._h, S.ctypes.data, max(nb, 1), 0, None) == code and (S == 7.0).all()
    Cb = np.full((n, 2), 7.0, dtype=F.dtype, order="F")
    for p in ("condense", "solve", "expand"):
        assert getattr(L, f"hs_interface_{p}{sfx}")(F._h, trans, Cb.ctypes.data_as(hs._lib.p_f64), n, n, 2) == code, p
    assert (Cb == 7.0).all()


def test_refusals_hss_interior_blocks(hs):
    E = hs._lib
    P = prepare(hs, (32, 32, 32), kind="convdiff", nmax=512, rhs="randn")  # the hss_d handle tests/test_ldiv_block_t_gpu.py refuses
    n = P["A"].shape[0]
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, hss_min=1024)
    assert len(hs.interface_indices(F)) == 0  # the sizes are still served
    _all_refused(hs, F, n, 0, E.HS_ERR_UNSUPPORTED)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.schur_complement(F)
    with pytest.raises(hs.UnsupportedError, match="HSS"):
        hs.condense(hs.transpose(F), np.zeros((n, 1), order="F"))
    F.free()
    P = interface_problem(hs, "convdiff", (24, 24, 24), 300)
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, mf=2, leafsize=128)
    _all_refused(hs, F, P["n"], 579, E.HS_ERR_UNSUPPORTED)
    F.free()


def test_refusals_bad_arguments(hs, handles):
    L = hs._lib.lib()
    E = hs._lib
    P, F = handles("exact0")
    n, nb = P["n"], 30
    pf = hs._lib.p_f64
    S = np.full((nb, nb), 7.0, order="F")
    Cb = np.full((n + 1, 2), 7.0, order="F")
    assert L.hs_interface_matrix_d(F._h, S.ctypes.data, nb, 2, None) == E.HS_ERR_ARGUMENT  # where
    assert L.hs_interface_matrix_d(F._h, S.ctypes.data, nb, -1, None) == E.HS_ERR_ARGUMENT
    assert L.hs_interface_matrix_d(F._h, S.ctypes.data, nb - 1, 0, None) == E.HS_ERR_DIMENSION  # lds
    assert L.hs_interface_matrix_d(F._h, None, nb, 0, None) == E.HS_ERR_ARGUMENT
    assert L.hs_interface_matrix_z(F._h, S.ctypes.data, nb, 0, None) == E.HS_ERR_ARGUMENT  # element type
    for p in ("condense", "solve", "expand"):
        fn, fz = getattr(L, f"hs_interface_{p}_d"), getattr(L, f"hs_interface_{p}_z")
        for trans in (-1, 3):
            assert fn(F._h, trans, Cb.ctypes.data_as(pf), n + 1, n, 2) == E.HS_ERR_ARGUMENT
        assert fn(F._h, 0, Cb.ctypes.data_as(pf), n - 1, n, 2) == E.HS_ERR_DIMENSION  # ldc
        assert fn(F._h, 0, Cb.ctypes.data_as(pf), n + 1, n + 1, 2) == E.HS_ERR_DIMENSION  # n
        assert fn(F._h, 0, Cb.ctypes.data_as(pf), n + 1, n, -1) == E.HS_ERR_DIMENSION  # nrhs
        assert fn(F._h, 0, None, n + 1, n, 2) == E.HS_ERR_ARGUMENT
        assert fz(F._h, 0, Cb.ctypes.data_as(pf), n + 1, n, 1) == E.HS_ERR_ARGUMENT
        assert fn(F._h, 0, Cb.ctypes.data_as(pf), n + 1, n, 0) == E.HS_OK  # no columns: nothing to do
    assert (S == 7.0).all() and (Cb == 7.0).all()
    with pytest.raises(TypeError):
        hs.condense(F, np.zeros((n, 1), dtype=np.complex128, order="F"))


def test_split_handle(hs):
    """hs_options.split slices the fronts of the user's tree; the pseudo-root is added after that rewrite and is never sliced, so a handle
    built with split keeps one dense LU of the interface block and is served (the refusal for a sliced pseudo-root has no handle that
    reaches it today)."""
    P = interface_problem(hs, "convdiff", (24, 24, 24), 300)
    F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=2, swsize=8, atol=1e-6, rtol=1e-6, split_size=256)
    S = hs.schur_complement(F)
    assert S.shape == (579, 579) and np.array_equal(S, hs.schur_complement(F))
    ref, _ = dense_schur(P["A"], hs.interface_indices(F))
    print(f"split handle at 1e-6: max |S - dense| / max |S| = {np.max(np.abs(S - ref)) / np.max(np.abs(ref)):.2e}")
    B = np.asfortranarray(_rand(np.random.default_rng(3), (P["n"], 33), False))
    for _, Fw in _wraps(hs, F):
        assert np.array_equal(hs.expand(Fw, hs.interface_solve(Fw, hs.condense(Fw, B.copy(order="F")))), hs.ldiv_block_t(Fw, B))
    F.free()
