"""hs_options.equilibrate on the MI355X (csrc/kernels_equil.hip, csrc/hs_api.hip): power-of-two row and column scaling on the device.

The inputs are B = D1 A D2 with seeded random power-of-two diagonals (exponents in +-40).  Scaling by 2^e is exact, so an equilibrated
handle F_e of B must behave bit for bit like a plain handle F_t (the "twin") of the prescaled matrix B_s = 2^er B 2^ec between two exact
scalings done on the host:

  * the exponents hs.equil_scales returns are those of the NumPy restatement (tests/equil_mirror.py), integer for integer;
  * op(F_e)^-1 b == 2^ec (F_t^-1 (2^er b)) (N) / 2^er (F_t^-T (2^ec b)) (T, C) with np.array_equal, for every ldiv entry point, host blocks
    and device tensors, C is B and C is not B, widths 1, 5 and 33 -- after the same test has asserted that two plain factorizations of B_s
    give equal solve bits (they do on all six flows, the compressed and the HSS ones included: DESIGN.md 4p);
  * the handle's own A stays the caller's B: berr, opnorm, GMRES iteration counts, condest;
  * the drivers built on the solves (sensitivity, misfit, tangent, ldiv_mod, gmres, eigs) against their twins;
  * logabsdet, the symmetric mode, a refactorization, the refusals, and the option off.

One problem, one set of factorizations per case, shared by the tests of this file and never modified."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import equil_mirror as EM
from helpers import prepare

pytestmark = pytest.mark.gpu

WIDTHS = (1, 5, 33)  # 33: a chunk boundary of the block solve (32 columns) is crossed
MF = dict(swsize=8, atol=1e-6, rtol=1e-6, leafsize=128)
CASES = {
    "poisson12": ("poisson", (12, 12, 12), 100, dict(swlevel=0)),
    "convdiff20": ("convdiff", (20, 20, 20), 100, dict(swlevel=0)),
    "cdh30x27": ("convdiff_helmholtz", (30, 27), 40, dict(swlevel=0)),
    "cdh24": ("convdiff_helmholtz", (24, 24, 24), 100, dict(swlevel=0)),
    "cdh24-lr": ("convdiff_helmholtz", (24, 24, 24), 100, dict(swlevel=2, atol=1e-4, rtol=1e-4)),
    "convdiff20-mf2": ("convdiff", (20, 20, 20), 200, dict(swlevel=2, mf=2, **MF)),
}
ULV = {"convdiff20-mf2"}  # HSS interior blocks: served by hs.ldiv (N) and hs.ldiv_ulv, the lockstep drivers through hs.ulv_mode
_S = {}


class Case:
    pass


@pytest.fixture(scope="module", autouse=True)
def _free_handles():
    yield
    for c in _S.values():
        for F in (c.Fe, c.Ft, c.Ft2):
            F.free()
    _S.clear()


def case(hs, label):
    if label in _S:
        return _S[label]
    kind, shape, nmax, kw = CASES[label]
    c = Case()
    c.label, c.kw = label, kw
    c.P = prepare(hs, shape, kind=kind, nmax=nmax, rhs="randn")
    c.B, c.e1, c.e2 = EM.badly_scaled(c.P["A"], 77, 40)
    c.n = c.B.shape[0]
    c.cplx = np.iscomplexobj(c.B.data)
    c.Fe = hs.factor(c.B, c.P["nd"], c.P["nd_loc"], equilibrate=True, **kw)
    c.er, c.ec = hs.equil_scales(c.Fe)
    c.Bs = EM.scaled(c.B, c.er, c.ec)
    c.Ft = hs.factor(c.Bs, c.P["nd"], c.P["nd_loc"], **kw)
    c.Ft2 = hs.factor(c.Bs, c.P["nd"], c.P["nd_loc"], **kw)
    if label in ULV:
        for F in (c.Fe, c.Ft, c.Ft2):
            hs.ulv_mode(F, True)
    _S[label] = c
    return c


def block(c, k, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((c.n, k))
    if c.cplx:
        X = X + 1j * rng.standard_normal((c.n, k))
    # right-hand sides as badly scaled as the rows of B
    return np.asfortranarray(EM.scale_rows(X, np.random.default_rng(seed + 1).integers(-40, 41, c.n)))


def scales(c, trans):
    """(exponents applied to B before the solve, to the result after it)"""
    return (c.er, c.ec) if trans == "N" else (c.ec, c.er)


def op(hs, F, trans):
    return {"N": F, "T": hs.transpose(F), "C": hs.adjoint(F)}[trans]


def entries(hs, c):
    """(name, host function of (F, trans, B), device symbol, trans list)"""
    def via(fn):
        return lambda F, t, B: fn(op(hs, F, t), B)

    out = [("ldiv", via(hs.ldiv), None, ("N",) if c.label in ULV else ("N", "T", "C"))]
    if c.label not in ULV:
        out += [("ldiv_block", via(hs.ldiv_block), "hs_ldiv_block_dev", ("N",)), ("ldiv_block_t", via(hs.ldiv_block_t), "hs_ldiv_block_dev_t", ("N", "T", "C"))]
    out += [("ldiv_ulv", via(hs.ldiv_ulv), "hs_ldiv_ulv_dev", ("N", "T", "C"))]
    return out


def compare(c, what, xe, xt, xt2, post):
    """xe (equilibrated handle, in B's scaling) against the twin's xt, both plain factorizations having been compared first."""
    assert np.array_equal(xt, xt2), (what, "two plain factorizations differ", np.linalg.norm(xt - xt2) / np.linalg.norm(xt))
    assert np.array_equal(xe, EM.scale_rows(xt, post)), (what, np.linalg.norm(EM.scale_rows(xe, -post) - xt) / np.linalg.norm(xt))


# ---- the exponents ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("label", list(CASES))
def test_exponents_equal_the_mirror(hs, label):
    c = case(hs, label)
    er, ec, sweeps = EM.equilibrate(c.B)
    assert c.er.dtype == np.int32 and np.array_equal(c.er, er) and np.array_equal(c.ec, ec)
    i = hs.equil_info(c.Fe)
    assert i == dict(option=True, sweeps=sweeps, er_min=int(er.min()), er_max=int(er.max()), ec_min=int(ec.min()), ec_max=int(ec.max())), i
    assert hs.equil_info(hs.transpose(c.Fe)) == i
    rows, cols, mag = EM.magnitudes(c.Bs)
    rmax, cmax = EM.maxima(rows, cols, mag, np.zeros(c.n, dtype=np.int64), np.zeros(c.n, dtype=np.int64), c.n)
    assert min(rmax.min(), cmax.min()) >= 0.5 and max(rmax.max(), cmax.max()) < 2.0


# ---- the twin identity ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("label", list(CASES))
def test_twin_identity_host_blocks(hs, label):
    c = case(hs, label)
    for name, fn, _, translist in entries(hs, c):
        for trans in translist:
            pre, post = scales(c, trans)
            for k in WIDTHS:
                Bk = block(c, k, 100 + k)
                if k == 1 and name == "ldiv":
                    Bk = Bk[:, 0].copy()  # a vector
                Bt = EM.scale_rows(Bk, pre)
                compare(c, (label, name, trans, k), fn(c.Fe, trans, Bk), fn(c.Ft, trans, Bt), fn(c.Ft2, trans, Bt), post)


def _dev_call(hs, F, sym, trans, dC, dB, k):
    import torch

    L = hs._lib.lib()
    fn = getattr(L, sym + ("_z" if F.dtype.kind == "c" else "_d"))
    hs._lib.check(fn(F._h, "NTC".index(trans), dC.data_ptr(), F.n, dB.data_ptr(), F.n, F.n, k, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def _dev_solve(hs, F, sym, trans, Bk, inplace):
    """The device entry on a column-major device block: C is B (in place) or C is not B (B must come back untouched)."""
    import torch

    k = Bk.shape[1]
    dB = torch.from_numpy(np.ascontiguousarray(Bk.T)).to("cuda")  # k x n row-major == n x k column-major
    if inplace:
        _dev_call(hs, F, sym, trans, dB, dB, k)
        return dB.cpu().numpy().T
    dC = torch.full_like(dB, 42.0)
    _dev_call(hs, F, sym, trans, dC, dB, k)
    assert np.array_equal(dB.cpu().numpy().T, Bk)
    return dC.cpu().numpy().T


@pytest.mark.parametrize("label", list(CASES))
def test_twin_identity_device_tensors(hs, label):
    c = case(hs, label)
    L = hs._lib.lib()
    ents = [(n, s, t) for n, _, s, t in entries(hs, c) if s]
    ents.append(("ldiv_dev_t", "hs_ldiv_dev_t", ("N",) if label in ULV else ("N", "T", "C")))
    for name, sym, translist in ents:
        for trans in translist:
            if sym == "hs_ldiv_block_dev" and trans != "N":
                continue
            pre, post = scales(c, trans)
            for k in WIDTHS:
                Bk = block(c, k, 200 + k)
                Bt = EM.scale_rows(Bk, pre)
                for inplace in (True, False):
                    xe = _dev_solve(hs, c.Fe, sym, trans, Bk, inplace)
                    xt = _dev_solve(hs, c.Ft, sym, trans, Bt, inplace)
                    xt2 = _dev_solve(hs, c.Ft2, sym, trans, Bt, inplace)
                    compare(c, (label, name, trans, k, "C is B" if inplace else "C is not B"), xe, xt, xt2, post)
    if label not in ULV:  # hs_ldiv_dev_* itself: the one entry without a trans argument
        import torch

        Bk = block(c, 5, 300)
        outs = []
        for F, Bx in ((c.Fe, Bk), (c.Ft, EM.scale_rows(Bk, c.er)), (c.Ft2, EM.scale_rows(Bk, c.er))):
            dB = torch.from_numpy(np.ascontiguousarray(Bx.T)).to("cuda")
            dC = torch.full_like(dB, 42.0)
            fn = L.hs_ldiv_dev_z if c.cplx else L.hs_ldiv_dev_d
            hs._lib.check(fn(F._h, dC.data_ptr(), c.n, dB.data_ptr(), c.n, c.n, 5, torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            outs.append(dC.cpu().numpy().T)
        compare(c, (label, "hs_ldiv_dev", "N", 5), outs[0], outs[1], outs[2], c.ec)


# ---- the handle's own A is the caller's, unscaled ------------------------------------------------------------------------------------------------

def consistent(c, k, seed, trans="N"):
    """op(B) X for X = 2^ec Z (N) / 2^er Z (T) with Z standard normal: right-hand sides of solutions that are well scaled in the scaled
    system -- b = 2^-er (B_s Z) (N), 2^-ec (B_s^T Z) (T).  Row i of the residual of such a system carries rounding errors of the size of
    eps |b_i|, in B's scaling and in B_s's alike; a block with arbitrary row scales (block above) has rows where |B| |x| exceeds |b| by many
    orders of magnitude, and no solver reaches a small 2-norm residual for it in B's own scaling."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((c.n, k))
    if c.cplx:
        Z = Z + 1j * rng.standard_normal((c.n, k))
    M, post = (c.Bs, c.er) if trans == "N" else (c.Bs.T, c.ec)
    return np.asfortranarray(EM.scale_rows(M @ Z, -post))


@pytest.mark.parametrize("label", ["poisson12", "convdiff20", "cdh30x27", "convdiff20-mf2"])
def test_own_matrix_is_unscaled(hs, label):
    c = case(hs, label)
    for trans in ("N", "T"):
        pre, post = scales(c, trans)
        for b in (block(c, 1, 400)[:, 0], consistent(c, 1, 401, trans)[:, 0]):
            _, be_e, _, _ = hs.ldiv_refine(op(hs, c.Fe, trans), b, itmax=0)
            _, be_t, _, _ = hs.ldiv_refine(op(hs, c.Ft, trans), EM.scale_rows(b, pre), itmax=0)
            print(f"[equil berr] {label} {trans}: equilibrated {be_e:.6e} twin {be_t:.6e}")
            # the componentwise backward error is invariant under exact diagonal scaling; a mix-up of A and A_s moves it by orders of magnitude
            assert be_e == pytest.approx(be_t, rel=1e-10), (trans, be_e, be_t)
    assert hs.opnorm(c.Fe, 1) == pytest.approx(spla.norm(c.B, 1), rel=1e-14)
    assert hs.opnorm(c.Fe, np.inf) == pytest.approx(spla.norm(c.B, np.inf), rel=1e-14)
    assert hs.opnorm(c.Ft, 1) == pytest.approx(spla.norm(c.Bs, 1), rel=1e-14)
    assert hs.condest(c.Fe, 1) == hs.opnorm(c.Fe, 1) * hs.opnormestinv(c.Fe)
    assert hs.opnormestinv(c.Fe) > 0.0


@pytest.mark.parametrize("label", ["poisson12", "convdiff20", "cdh30x27"])
def test_gmres_on_the_own_matrix_takes_the_iterations_of_the_twin(hs, label):
    """GMRES on the handle's own A (A=None) with the handle as preconditioner: the residuals are those of B, not of B_s.

    The stopping test of the equilibrated run measures 2^-er r where the twin's measures r, so the two counts are equal only at a
    tolerance no residual comes near in either norm.  With an exact factorization as preconditioner the first step leaves a residual of
    the size of the factorization's backward error and the second one rounding errors: measured on an MI355X, relative to the first
    residual, 4e-11 .. 5e-9 then <= 2e-19 in B's scaling and 6e-9 .. 2e-5 then <= 4e-13 in B_s's.  reltol = 1e-3 lies two orders of
    magnitude above every first-step residual: one iteration per column on both sides.  (At 1e-9, which falls between the first-step
    residuals of the two scalings, the equilibrated run takes 1 - 2 iterations where the twin takes 2: there the counts are asserted to differ
    by one step at the most, and both runs to converge.)
    A wrong matrix behind A=None -- B_s for B -- is preconditioned by nothing like its inverse and converges to neither tolerance."""
    c = case(hs, label)
    Bk = consistent(c, 5, 500)
    for reltol in (1e-3, 1e-9):
        gm = dict(reltol=reltol, restart=30, maxiter=30, log=True)
        Xe, he = hs.gmres_block(None, Bk, Pr=c.Fe, **gm)
        Xt, ht = hs.gmres_block(None, EM.scale_rows(Bk, c.er), Pr=c.Ft, **gm)
        ie, it = [h["iters"] for h in he], [h["iters"] for h in ht]
        print(f"[equil gmres] {label} reltol {reltol:g}: iterations equilibrated {ie} twin {it}")
        for k in range(len(he)):
            re_, rt_ = np.asarray(he[k]["resnorm"]), np.asarray(ht[k]["resnorm"])
            print(f"[equil gmres]   column {k}: relative residuals equilibrated {np.array2string(re_ / re_[0], precision=2)} twin {np.array2string(rt_ / rt_[0], precision=2)}")
        assert all(h["isconverged"] for h in he) and all(h["isconverged"] for h in ht), (ie, it)
        if reltol == 1e-3:
            assert ie == it == [1] * 5, (ie, it)
        else:  # the tolerance lies between the first-step residuals of the two scalings: one step of difference at the most, more than one step taken
            assert all(abs(a - b) <= 1 for a, b in zip(ie, it)) and max(it) >= 2, (ie, it)
        # the residual of B itself, on the host: a wrong matrix behind A=None would leave one of the size of b
        R = Bk - c.B @ Xe
        assert np.all(np.linalg.norm(R, axis=0) <= reltol * np.linalg.norm(Bk, axis=0)), np.linalg.norm(R, axis=0) / np.linalg.norm(Bk, axis=0)


def _inverse_norm1(c, transposed):
    """||op(B)^-1||_1 from the dense inverse of the well-scaled B_s: op(B)^-1[:, j] = 2^post (op(B_s)^-1[:, j]) 2^pre[j].  The columns that
    can hold the maximum are refined with residuals in extended precision, so that the reference is good to its last bits: the plain
    dense inverse carries cond(B_s) eps ~ 1e-9, more than the 1e-10 the bound below allows the estimate to exceed it by."""
    M = c.Bs.toarray().T if transposed else c.Bs.toarray()
    pre, post = (c.ec, c.er) if transposed else (c.er, c.ec)
    X0 = np.linalg.inv(M)
    sums = np.ldexp(np.ldexp(np.abs(X0), post.astype(np.int32)[:, None]).sum(axis=0), pre.astype(np.int32))
    ML, XL = M.astype(np.clongdouble), X0.astype(np.clongdouble)
    best = np.longdouble(0)
    for j in np.flatnonzero(sums >= sums.max() * (1 - 1e-6)):
        x = XL[:, j].copy()
        e = np.zeros(c.n, dtype=np.clongdouble)
        e[j] = 1
        for _ in range(3):
            x += XL @ (e - ML @ x)
        best = max(best, np.ldexp(np.ldexp(np.abs(x), post.astype(np.int32)).sum(), int(pre[j])))
    return float(best)


def test_condest_against_the_dense_inverse(hs):
    c = case(hs, "cdh30x27")
    for p, F, transposed in ((1, c.Fe, False), (np.inf, c.Fe, True), (1, hs.transpose(c.Fe), True)):
        # cond_inf(B) = cond_1(B^T)
        true = spla.norm(c.B.T if transposed else c.B, 1) * _inverse_norm1(c, transposed)
        est = hs.condest(F, p)
        print(f"[equil condest] p={p} {'transpose(F)' if F is not c.Fe else 'F'}: estimate {est:.12e} true {true:.12e}")
        assert est <= true * (1 + 1e-10) and est >= true / 3, (p, est, true)


# ---- determinant -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("label", list(CASES))
def test_logabsdet(hs, label):
    c = case(hs, label)
    (le, se), (lt, st) = hs.logabsdet(c.Fe), hs.logabsdet(c.Ft)
    shift = float(np.log(2.0)) * int(c.er.astype(np.int64).sum() + c.ec.astype(np.int64).sum())
    print(f"[equil logabsdet] {label}: equilibrated {le:.12g} twin {lt:.12g} shift {shift:.12g}")
    assert le == pytest.approx(lt - shift, rel=1e-12)
    assert se == st  # the phase is that of A_s: unchanged
    assert hs.logabsdet(hs.adjoint(c.Fe)) == (le, np.conj(se) if c.cplx else se)
    if label == "cdh30x27":
        # The determinant of the dense B.  numpy.linalg.slogdet applied to B itself is no reference: cond_1(B) ~ 1e51, the partial
        # pivoting of its LU follows the scales of D1 and D2, and its log|det| is off by about 40 from the value its own results for A
        # and for B_s give, each shifted by the exact power of two (those two agree to 2e-12).  So the reference is slogdet of the dense
        # A, shifted by ln 2 (sum e1 + sum e2) exactly; the tolerances are those of tests/test_selinv_gpu.py against its reference.
        sa, la = np.linalg.slogdet(c.P["A"].toarray())
        lref, sref = la + float(np.log(2.0)) * int(c.e1.astype(np.int64).sum() + c.e2.astype(np.int64).sum()), sa
        sb, lb = np.linalg.slogdet(c.B.toarray())
        ss, ls = np.linalg.slogdet(c.Bs.toarray())
        print(f"[equil logabsdet] log|det B| {le:.13g}; numpy.linalg.slogdet of A, shifted: {lref:.13g} (sign diff {abs(sref - se):.2e}); of B_s, shifted: "
              f"{ls - shift:.13g} (sign diff {abs(ss - se):.2e}); of B itself: {lb:.13g} (sign diff {abs(sb - se):.2e})")
        assert abs(le - lref) <= 1e-11 * max(1.0, abs(lref)), (le, lref)
        assert abs(se - sref) <= 1e-10, (se, sref)
        assert abs(le - (ls - shift)) <= 1e-11 * max(1.0, abs(lref)), (le, ls - shift)


# ---- the drivers built on the solves, against their twins ------------------------------------------------------------------------------------

def _entry_scales(c):
    """er[row] + ec[col] of every stored entry (CSC order)."""
    rows, cols, _ = EM.magnitudes(c.B)
    return (c.er[rows].astype(np.int64) + c.ec[cols]).astype(np.int32)


def _ldexp(v, s):
    return np.ldexp(v.real, s) + 1j * np.ldexp(v.imag, s) if np.iscomplexobj(v) else np.ldexp(v, s)


@pytest.mark.parametrize("label", ["convdiff20", "cdh30x27"])
def test_sensitivity_misfit_and_tangent_equal_their_twins(hs, label):
    """With X = 2^ec X_s and Lam = 2^er Lam_s every product of the reductions is the twin's times an exact power of two:
    G[i, j] = 2^(er_i + ec_j) G_s[i, j] for W_s = 2^ec W, and dX = 2^ec dX_s for E_s = 2^(er_i + ec_j) E -- bit for bit."""
    c = case(hs, label)
    se = _entry_scales(c)
    b, W = consistent(c, 2, 900), block(c, 2, 901)
    G, X, Lam = hs.sensitivity(c.Fe, b, W, want=("X", "Lam"))
    Gt, Xt, Lt = hs.sensitivity(c.Ft, EM.scale_rows(b, c.er), EM.scale_rows(W, c.ec), want=("X", "Lam"))
    assert np.array_equal(X, EM.scale_rows(Xt, c.ec)) and np.array_equal(Lam, EM.scale_rows(Lt, c.er))
    assert np.array_equal(G, _ldexp(Gt, se)) and np.any(G != 0)
    # misfit: its cotangent is built on the device, sparse, and solved through the block solve on such a handle
    rows = np.array([5, 17, c.n - 3])
    D = X[rows] * 0.5
    J, Gm, R = hs.misfit(c.Fe, b, rows, D, want_residual=True)
    assert np.array_equal(R, X[rows] - D)
    assert np.allclose(J, 0.5 * np.sum(np.abs(R) ** 2, axis=0), rtol=1e-13, atol=0.0)
    Wd = np.zeros_like(b)
    Wd[rows] = R
    Gd = hs.sensitivity(c.Fe, b, Wd)
    assert np.linalg.norm(Gm - Gd) <= 1e-12 * np.linalg.norm(Gd), np.linalg.norm(Gm - Gd) / np.linalg.norm(Gd)
    # tangent: E a perturbation of the stored entries, of their own size
    E = c.B.data * np.random.default_rng(902).standard_normal(c.B.nnz)
    dX = hs.tangent(c.Fe, b, E)
    dXt = hs.tangent(c.Ft, EM.scale_rows(b, c.er), _ldexp(E, se))
    assert np.array_equal(dX, EM.scale_rows(dXt, c.ec)) and np.any(dX != 0)
    sub = np.array([0, 9, c.n - 1])
    assert np.array_equal(hs.tangent(c.Fe, b, E, rows=sub), dX[sub])


@pytest.mark.parametrize("label", ["convdiff20", "cdh30x27"])
def test_ldiv_mod_equals_its_twin(hs, label):
    """A1 = B + U V^T with U = 2^-er U_s, V = 2^-ec V_s is 2^-er (B_s + U_s V_s^T) 2^-ec: the twin's modification, and every inner
    product of the capacitance system is the twin's exactly."""
    c = case(hs, label)
    rng = np.random.default_rng(910)
    Us, Vs = 0.05 * rng.standard_normal((c.n, 3)), rng.standard_normal((c.n, 3))
    if c.cplx:
        Us = Us + 0.05j * rng.standard_normal((c.n, 3))
    Me = hs.modify(c.Fe, U=EM.scale_rows(Us, -c.er), V=EM.scale_rows(Vs, -c.ec))
    Mt = hs.modify(c.Ft, U=Us, V=Vs)
    b = consistent(c, 5, 911)
    for trans in ("N", "T"):
        pre, post = scales(c, trans)
        xe = hs.ldiv_mod(Me, b, trans=trans)
        xt = hs.ldiv_mod(Mt, EM.scale_rows(b, pre), trans=trans)
        assert np.array_equal(xe, EM.scale_rows(xt, post)), (trans, np.linalg.norm(EM.scale_rows(xe, -post) - xt) / np.linalg.norm(xt))
        assert not np.array_equal(xe, hs.ldiv_block_t(op(hs, c.Fe, trans), b))  # the modification is felt
    Me.free()
    Mt.free()


def test_single_vector_gmres_on_the_own_matrix(hs):
    c = case(hs, "convdiff20")
    b = consistent(c, 1, 920)[:, 0]
    xe, he = hs.gmres(None, b, Pr=c.Fe, reltol=1e-3, restart=30, maxiter=30, log=True)
    xt, ht = hs.gmres(None, EM.scale_rows(b, c.er), Pr=c.Ft, reltol=1e-3, restart=30, maxiter=30, log=True)
    assert he["isconverged"] and ht["isconverged"] and he["iters"] == ht["iters"] == 1, (he["iters"], ht["iters"])
    assert np.linalg.norm(b - c.B @ xe) <= 1e-3 * np.linalg.norm(b)


def test_eigs_of_a_similarity_scaled_matrix(hs):
    """D A D^-1 has A's eigenvalues; the handle factors its equilibrated form and hs.eigs iterates with op(F)^-1 of D A D^-1 itself."""
    c = case(hs, "poisson12")
    A = c.P["A"]
    e = np.random.default_rng(930).integers(-4, 5, c.n).astype(np.int32)
    S = EM.scaled(A, e, -e)
    F = hs.factor(S, c.P["nd"], c.P["nd_loc"], swlevel=0, equilibrate=True)
    er, ec = hs.equil_scales(F)
    assert er.any() and ec.any()
    lam, X = hs.eigs(F, nev=4, sigma=0.0, tol=1e-10)
    ref = np.linalg.eigvalsh(A.toarray())[:4]
    print(f"[equil eigs] {np.sort(np.asarray(lam).real)} reference {ref}")
    assert np.allclose(np.sort(np.asarray(lam).real), ref, rtol=1e-8, atol=0.0) and np.all(np.abs(np.asarray(lam).imag) <= 1e-8)
    R = S @ X - X * lam
    assert np.all(np.linalg.norm(R, axis=0) <= 1e-8 * np.linalg.norm(X, axis=0))
    F.free()


# ---- with hs_options.symmetric -----------------------------------------------------------------------------------------------------------------

def test_symmetric_mode(hs):
    c = case(hs, "poisson12")
    A = c.P["A"]
    e = np.random.default_rng(5).integers(-40, 41, c.n).astype(np.int32)
    Bd = EM.scaled(A, e, e)
    assert (Bd != Bd.T).nnz == 0
    Fe = hs.factor(Bd, c.P["nd"], c.P["nd_loc"], swlevel=0, symmetric=True, equilibrate=True)
    er, ec = hs.equil_scales(Fe)
    assert np.array_equal(er, ec) and np.array_equal(er, EM.equilibrate(Bd)[0])
    Bs = EM.scaled(Bd, er, ec)
    Ft = hs.factor(Bs, c.P["nd"], c.P["nd_loc"], swlevel=0, symmetric=True)
    ie, it = hs.sym_info(Fe), hs.sym_info(Ft)
    assert ie == it and ie["option"] and ie["fronts_lower"] > 0 and ie["fronts_general"] == 0, (ie, it)
    b = block(c, 5, 600)
    assert np.array_equal(hs.ldiv_block(Fe, b), EM.scale_rows(hs.ldiv_block(Ft, EM.scale_rows(b, er)), ec))
    # the claim is checked on the caller's values: D1 A D2 with D1 != D2 is refused as without the option
    with pytest.raises(ValueError) as ei:
        hs.factor(c.B, c.P["nd"], c.P["nd_loc"], swlevel=0, symmetric=True, equilibrate=True)
    assert "symmetric" in str(ei.value)
    Fe.free()
    Ft.free()


# ---- refactorization ---------------------------------------------------------------------------------------------------------------------------

def test_refactorization_finds_the_exponents_anew(hs):
    import torch

    from hierarchicalsolvers_jl_amd import dist as hsdist

    c = case(hs, "convdiff20")
    S = hsdist.StagedSolver(c.B, c.P["nd"], c.P["nd_loc"], device="cuda:0", swlevel=0, equilibrate=True)
    Fv = hs.FactorNode(S.backend._h, c.B.dtype, c.n, None)  # a borrowed view of the staged handle: never freed here
    try:
        seen = []
        for seed in (77, 78):
            Bx, _, _ = EM.badly_scaled(c.P["A"], seed, 40)
            assert np.array_equal(Bx.indices, c.B.indices)
            S.numeric(torch.from_numpy(np.ascontiguousarray(Bx.data)).to("cuda:0"))
            er, ec = hs.equil_scales(Fv)
            mr, mc, sweeps = EM.equilibrate(Bx)
            assert np.array_equal(er, mr) and np.array_equal(ec, mc) and hs.equil_info(Fv)["sweeps"] == sweeps
            seen.append((er, ec))
            Ft = hs.factor(EM.scaled(Bx, er, ec), c.P["nd"], c.P["nd_loc"], swlevel=0)
            b = block(c, 5, 700 + seed)
            for trans in ("N", "T"):
                pre, post = scales_of(er, ec, trans)
                xe = hs.ldiv_block_t(op(hs, Fv, trans), b)
                xt = hs.ldiv_block_t(op(hs, Ft, trans), EM.scale_rows(b, pre))
                assert np.array_equal(xe, EM.scale_rows(xt, post)), (seed, trans)
            # the staged solve goes through the library's own ldiv! on such a handle (the level sweeps are refused)
            d = torch.from_numpy(b[:, 0].copy()).to("cuda:0")
            S.solve(d)
            torch.cuda.synchronize()
            assert np.array_equal(d.cpu().numpy(), hs.ldiv(Fv, b[:, 0]))
            Ft.free()
        assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[0][1], seen[1][1])
        assert np.array_equal(seen[0][0], c.er)  # the first values are those of the shared case
    finally:
        Fv._h = None


def scales_of(er, ec, trans):
    return (er, ec) if trans == "N" else (ec, er)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------

def test_direct_readers_of_the_factors_refuse(hs):
    c = case(hs, "poisson12")
    F, n = c.Fe, c.n
    L, E = hs._lib.lib(), hs._lib
    b = block(c, 2, 800)
    Bsp = sp.csc_matrix((np.ones(2), ([3, 40], [0, 1])), shape=(n, 2))
    calls = {
        "mul": lambda: hs.mul(F, b),
        "mul transposed": lambda: hs.mul(hs.transpose(F), b),
        "factor_error": lambda: hs.factor_error(F, k=4),
        "selinv": lambda: hs.selinv(F),
        "selinv_lr": lambda: hs.selinv_lr(F),
        "demote": lambda: hs.demote(F),
        "schur_complement": lambda: hs.schur_complement(F),
        "condense": lambda: hs.condense(F, b.copy(order="F")),
        "interface_solve": lambda: hs.interface_solve(F, b.copy(order="F")),
        "expand": lambda: hs.expand(F, b.copy(order="F")),
        "ldiv_sparse": lambda: hs.ldiv_sparse(F, Bsp),
        "ldiv_sparse_plan": lambda: hs.ldiv_sparse_plan(F, Bsp),
        "sensitivity, sparse blocks": lambda: hs.sensitivity(F, Bsp, Bsp),
        "tangent, sparse block": lambda: hs.tangent(F, Bsp, c.B.data),
        "gn_hessvec, sparse block": lambda: hs.gn_hessvec(F, Bsp, [3, 40], c.B.data),
        "gn_hessvec, pruned adjoint": lambda: hs.gn_hessvec(F, b, [3, 40], c.B.data),
        "gn_diag, pruned adjoint": lambda: hs.gn_diag(F, b, [3, 40]),
        "modify, sparse dA": lambda: hs.modify(F, dA=sp.csc_matrix(([0.5], ([3], [3])), shape=(n, n))),
        "inv_entries": lambda: hs.inv_entries(F, [1, 2], [3, 4]),
    }
    for name, call in calls.items():
        with pytest.raises(E.UnsupportedError) as ei:
            call()
        assert "equilibrate" in str(ei.value), (name, str(ei.value))
    import torch

    d = torch.zeros(n, dtype=torch.float64, device="cuda")
    for fn in (L.hs_solve_fwd_levels, L.hs_solve_bwd_levels):
        assert fn(F._h, d.data_ptr(), 1, 1, None) == E.HS_ERR_UNSUPPORTED and b"equilibrate" in L.hs_last_error()
    # the twin serves every one of them
    for name, call in (("mul", lambda: hs.mul(c.Ft, b)), ("selinv", lambda: hs.selinv_diag(c.Ft)), ("ldiv_sparse", lambda: hs.ldiv_sparse(c.Ft, Bsp))):
        call()
    # ... and the dense-block drivers serve the equilibrated handle
    assert np.all(np.isfinite(hs.sensitivity(F, b, b)))


def _extreme(c):
    """The Poisson matrix with the other entries of one row i and of one column j scaled by 2^800 and the crossing entry (i, j) set to
    2^-300: the sweeps bring the large entries to O(1) with exponents near -400 on both sides, and the crossing entry to about 2^-1100,
    below the normal range."""
    A = sp.csc_matrix(c.P["A"], copy=True)
    A.sort_indices()
    coo = A.tocoo()
    j = 101
    i = int([r for r in A.indices[A.indptr[j]:A.indptr[j + 1]] if r != j][0])
    v = coo.data.copy()
    big = ((coo.row == i) | (coo.col == j)) & ~((coo.row == i) & (coo.col == j))
    v[big] = np.ldexp(v[big], 800)
    v[(coo.row == i) & (coo.col == j)] = np.ldexp(1.0, -300)
    return sp.csc_matrix((v, (coo.row, coo.col)), shape=A.shape), (i, j)


def test_refuses_an_entry_that_leaves_the_normal_range(hs):
    c = case(hs, "poisson12")
    X, (i, j) = _extreme(c)
    er, ec, _ = EM.equilibrate(X)
    Xs = EM.scaled(X, er, ec)
    X.sort_indices()
    lost = np.flatnonzero((X.data != 0) & (np.abs(Xs.data) < np.finfo(np.float64).tiny))
    cols = np.repeat(np.arange(c.n), np.diff(X.indptr))
    assert lost.size == 1 and (int(X.indices[lost[0]]), int(cols[lost[0]])) == (i, j), lost  # the mirror agrees: this entry and no other is lost
    with pytest.raises(hs._lib.UnsupportedError) as ei:
        hs.factor(X, c.P["nd"], c.P["nd_loc"], swlevel=0, equilibrate=True)
    msg = str(ei.value)
    assert "equilibrate" in msg and f"(row {i + 1}, column {j + 1})" in msg, msg


def test_zero_row_raises_what_it_raises_without_the_option(hs):
    c = case(hs, "poisson12")
    Z = sp.csc_matrix(c.B, copy=True)
    Z.sort_indices()
    Z.data[Z.indices == 7] = 0.0  # a stored zero row
    assert EM.equilibrate(Z)[0][7] == 0

    def outcome(eq):
        try:
            F = hs.factor(Z, c.P["nd"], c.P["nd_loc"], swlevel=0, equilibrate=eq)
        except Exception as e:  # noqa: BLE001
            return type(e).__name__, getattr(e, "status", None)
        F.free()
        return "factored", None

    off, on = outcome(False), outcome(True)
    print(f"[equil zero row] without the option: {off}, with it: {on}")
    assert on == off and off[0] != "UnsupportedError", (off, on)


def test_option_off(hs):
    c = case(hs, "poisson12")
    assert hs.equil_info(c.Ft) == dict(option=False, sweeps=0, er_min=0, er_max=0, ec_min=0, ec_max=0)
    with pytest.raises(ValueError):
        hs.equil_scales(c.Ft)
    er = (C.c_int32 * c.n)()
    assert hs._lib.lib().hs_equil_scales(c.Ft._h, er, None) == hs._lib.HS_ERR_ARGUMENT
