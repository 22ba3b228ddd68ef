"""Host-side checks of the symmetric mode (hs_options.symmetric; Sched::sym, csrc/hs_sched.h): no device needed.

  * the generator of the symmetric test fronts (sym_mirror.sym_front) has the margins the kernel tests need;
  * the NumPy restatement of the schedule (sym_mirror.sym_schedule_lu: lower strips, upper blocks by transposition, everything the
    invariant says is never read poisoned with NaN) takes the pivots of lu_mirror.optimistic_lu on the whole front and agrees with its
    factors within 1e-12 of their largest entry; no NaN survives; S is exactly symmetric;
  * the closed-form count of the plain updates of a lone front ni = nb = 2048 with the production strips (Sched::sym_strip: 256 columns
    inside the interior, 512 on S; look-ahead block columns of 1024): 0.8218 of the full count (the cap is 0.85; the ideal lower-triangle
    count is 0.75, fixed strips of 256 would give 0.7927, of 512 0.8255);
  * the Python layer carries the option."""
import functools

import numpy as np
import pytest

from sym_mirror import LA_NB, SYM_STRIP, find_sym_front, schedule_flops, sym_schedule_lu

SHAPES = [(False, 33, 5), (False, 257, 40), (False, 300, 300), (False, 600, 0), (False, 1537, 37),
          (True, 33, 5), (True, 257, 40), (True, 300, 300), (True, 600, 0), (True, 1200, 37)]


@functools.lru_cache(maxsize=None)
def front_and_mirror(cplx, ni, nb):
    """(F, optimistic_lu(F, ni)) with the margins checked below, built once per process and shared: callers must not modify either."""
    return find_sym_front(np.random.default_rng(9000 + 1000 * cplx + ni), ni, nb, cplx)


@pytest.mark.parametrize("cplx,ni,nb", SHAPES)
def test_sym_front_margins(cplx, ni, nb):
    F, mir = front_and_mirror(cplx, ni, nb)
    assert np.array_equal(F, F.T)  # plain transpose, also when complex
    assert not mir["flag"] and not mir["bad"]
    assert np.any(mir["rperm"] != np.arange(ni))  # the front pivots
    assert mir["lmax"] <= 1.93, mir["lmax"]
    assert mir["gap"] >= 3.7e-5, mir["gap"]


def _schedules(cplx, ni):
    """(block column, strip) pairs: small ones that give every shape several block columns and strips, and the production pair."""
    out = [(64, 32), (256, 256)]
    if ni > 1024:
        out = [(LA_NB[cplx], SYM_STRIP)]
    return out


@pytest.mark.parametrize("cplx,ni,nb", SHAPES)
def test_sym_schedule_matches_mirror(cplx, ni, nb):
    F, mir = front_and_mirror(cplx, ni, nb)
    Aii, Aib, Abi, Abb = F[:ni, :ni], F[:ni, ni:], F[ni:, :ni], F[ni:, ni:]
    LU = np.tril(mir["L"], -1) + mir["U"]
    Uib = np.linalg.solve(mir["L"], Aib[mir["rperm"]])
    S = Abb - mir["Lbi"] @ Uib
    for nbcol, strip in _schedules(cplx, ni):
        r = sym_schedule_lu(F, ni, nbcol, strip)
        what = (cplx, ni, nb, nbcol, strip)
        assert np.array_equal(r["rperm"], mir["rperm"]), what
        for got, ref, name in ((r["LF"][:ni], LU, "L\\U"), (r["LF"][ni:], mir["Lbi"], "Lbi"), (r["UR"], Uib, "Uib"), (r["S"], S, "S")):
            assert not np.isnan(got).any(), (what, name)  # a NaN here: the schedule read a block it may not read
            if ref.size:
                e = np.abs(got - ref).max() / np.abs(ref).max()
                assert e <= 1e-12, (what, name, e)
        assert np.array_equal(r["S"], r["S"].T), what


def test_strip_flop_count():
    """Lone Float64 front ni = nb = 2048, production schedule: the strips execute at most 0.85 of the plain-update flops (counted here: 0.8218)."""
    full = schedule_flops(2048, 2048, False)
    sym = schedule_flops(2048, 2048, True)
    print(f"[sym flops] ni = nb = 2048: full {full:.4g}  symmetric {sym:.4g}  ratio {sym / full:.4f}")
    assert sym <= 0.85 * full, sym / full
    # a root front (nb = 0) on the recursive schedule saves inside the interior too; the strips never execute more than the full updates
    for ni, nb, la in ((4096, 0, False), (4096, 0, True), (16384, 0, True), (600, 300, True), (1537, 37, True)):
        assert schedule_flops(ni, nb, True, lookahead=la) <= schedule_flops(ni, nb, False, lookahead=la)
    assert schedule_flops(4096, 0, True, lookahead=False) < schedule_flops(4096, 0, False, lookahead=False)
    assert schedule_flops(16384, 0, True) < 0.80 * schedule_flops(16384, 0, False)


def test_python_option():
    import hsamd

    hs = hsamd.load()
    o = hs.SolverOptions(symmetric=True)
    assert o.to_c().symmetric == 1
    assert hs.SolverOptions().to_c().symmetric == 0
    assert o.copy().symmetric is True and o.copy(symmetric=False).symmetric is False
    assert o.copy(swlevel=2).to_c().symmetric == 1
    with pytest.raises(TypeError):
        hs.SolverOptions(symmetrical=True)
    with pytest.raises(TypeError):
        o.copy(hermitian=True)
    # the field is appended: the offsets of the older fields do not move
    C = hs._lib.hs_options
    assert C.symmetric.offset == C.seed.offset + 8 and C.seed.offset == 72
    assert "hs_sym_info" in hs._lib.EXPORTS and "hsk_front_batch_sym_d" in hs._lib.EXPORTS and "hsk_front_batch_sym_z" in hs._lib.EXPORTS
    assert callable(hs.sym_info)


def test_plan_refuses_several_ranks():
    """hs_plan needs no device: hs_options.symmetric with two ranks is HS_ERR_UNSUPPORTED, with one rank it plans."""
    import hsamd

    hs = hsamd.load()
    A, _, nd = hs.problems.make_problem((8, 8, 8), kind="poisson")
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    A = A[perm - 1][:, perm - 1].tocsc()
    nd = hs.permuted(nd, hs.invperm(perm))
    with pytest.raises(hs._lib.UnsupportedError):
        hs.dist.plan_only(A, nd, nd_loc, rank=0, nranks=2, symmetric=True)
    hs._lib.lib().hs_free(hs.dist.plan_only(A, nd, nd_loc, rank=0, nranks=2))
    hs._lib.lib().hs_free(hs.dist.plan_only(A, nd, nd_loc, rank=0, nranks=1, symmetric=True))
