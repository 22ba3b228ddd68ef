"""Host tests of tests/lu_mirror.py, the NumPy restatement of optimistic pivoting that tests/test_lu_paths_gpu.py holds the kernels to:
against LAPACK's partial pivoting where the two must coincide, P A = L U everywhere, and the pivot key and growth flag on hand-built cases."""
import numpy as np
import pytest
import scipy.linalg as sla

from lu_mirror import GROWTH_MAX, find_good_front, optimistic_lu, pivot_key


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ni", [1, 5, 32, 33, 64, 100, 257])
def test_mirror_matches_lapack_on_block_diagonal(ni, cplx):
    """Block-diagonal Aii (32 x 32 blocks, the last one partial): partial pivoting over all rows and over the block's rows pick the same
    pivots, so the mirror must reproduce scipy.linalg.lu (LAPACK getrf: idamax / izamax, i.e. abs1 for complex) exactly up to rounding."""
    rng = np.random.default_rng(ni + 100 * cplx)
    A = np.zeros((ni, ni), dtype=np.complex128 if cplx else np.float64)
    for c0 in range(0, ni, 32):
        c1 = min(ni, c0 + 32)
        A[c0:c1, c0:c1] = _rand(rng, (c1 - c0, c1 - c0), cplx)
    r = optimistic_lu(A, ni)
    P, L, U = sla.lu(A)
    assert np.array_equal(r["rperm"], np.argmax(P, axis=0))
    assert np.linalg.norm(r["L"] - L) <= 1e-12 * np.linalg.norm(L)
    assert np.linalg.norm(r["U"] - U) <= 1e-12 * np.linalg.norm(U)
    # partial pivoting on abs1 keeps every multiplier within its block at abs1 <= 1 (Float64) or <= 2 (ComplexF64: |l| <= sqrt 2)
    assert not r["bad"] and r["lmax"] <= (2.0 if cplx else 1.0) + 1e-12


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ni,nb", [(40, 9), (96, 0), (300, 50)])
def test_mirror_factors_general_fronts(ni, nb, cplx):
    """P Aii = L U and Lbi U = Abi on dense fronts, including ones with multipliers far above the bound (the factorization is still an
    exact-arithmetic LU; only its stability is lost)."""
    rng = np.random.default_rng(ni * 3 + nb)
    for F in (_rand(rng, (ni + nb, ni + nb), cplx), find_good_front(rng, ni, nb, cplx)[0]):
        r = optimistic_lu(F, ni)
        Aii, Abi = F[:ni, :ni], F[ni:, :ni]
        assert sorted(r["rperm"].tolist()) == list(range(ni))
        scale = np.linalg.norm(np.abs(r["L"]) @ np.abs(r["U"]))
        assert np.linalg.norm(r["L"] @ r["U"] - Aii[r["rperm"]]) <= 1e-13 * scale
        if nb:
            assert np.linalg.norm(r["Lbi"] @ r["U"] - Abi) <= 1e-13 * (np.linalg.norm(np.abs(r["Lbi"]) @ np.abs(r["U"])) + np.linalg.norm(Abi))
        assert r["flag"] == (r["lmax"] > GROWTH_MAX or r["bad"])


def _eye_front(ni, nb=0, cplx=False):
    return np.eye(ni + nb, dtype=np.complex128 if cplx else np.float64)


def test_mirror_flag_threshold_below_the_block():
    """A multiplier of a row below the diagonal block: 5 > 4 raises the flag, 3.9 does not; the bound is on the multiplier, not the
    entry (the same entry under a pivot of 2 gives 2.5)."""
    for v, piv, flag in ((5.0, 1.0, True), (3.9, 1.0, False), (-4.5, 1.0, True), (5.0, 2.0, False), (8.5, 2.0, True)):
        F = _eye_front(64)
        F[3, 3] = piv
        F[40, 3] = v
        r = optimistic_lu(F, 64)
        assert r["flag"] == flag, (v, piv)
        assert r["lmax"] == pytest.approx(abs(v) / piv)
        assert np.array_equal(r["rperm"], np.arange(64))  # a row below the block is never a candidate


def test_mirror_flag_complex_uses_abs1():
    """ComplexF64 bounds abs1 = |re| + |im| (what the kernels compare), not the modulus: 3 + 1.5i has modulus 3.35 but abs1 4.5."""
    F = _eye_front(64, cplx=True)
    F[40, 3] = 3 + 1.5j
    assert optimistic_lu(F, 64)["flag"]
    F[40, 3] = 2 + 1.5j
    assert not optimistic_lu(F, 64)["flag"]


def test_mirror_flag_nan_and_zero_column():
    F = _eye_front(64)
    F[50, 7] = np.nan
    r = optimistic_lu(F, 64)
    assert r["flag"] and np.isnan(r["lmax"])
    # column 35 is zero on the rows of its own block (32..63) but not below it: no candidate -> flag
    F = _eye_front(96)
    F[35, 35] = 0.0
    F[70, 35] = 1.0
    r = optimistic_lu(F, 96)
    assert r["flag"] and r["bad"]
    # the same column with its only nonzero entry inside the block is an ordinary swap
    F = _eye_front(96)
    F[35, 35] = 0.0
    F[40, 35] = 1.0
    F[35, 40] = 1.0
    F[40, 40] = 0.0
    r = optimistic_lu(F, 96)
    assert not r["flag"] and r["rperm"][3 + 32] == 40


def test_mirror_rows_of_abi_never_raise_the_flag():
    F = _eye_front(64, nb=10)
    F[64 + 3, 5] = 1e6  # Abi
    r = optimistic_lu(F, 64)
    assert not r["flag"] and r["lmax"] == 0.0
    assert r["Lbi"][3, 5] == 1e6


def test_mirror_pivot_key_ties():
    """The key drops the low 8 bits of abs1: candidates that differ only there tie, and a tie goes to the lowest row by its position at
    the start of the panel."""
    assert pivot_key(1.0) == pivot_key(1.0 + 2.0**-46)  # 64 ulp apart: same key
    assert pivot_key(1.0) < pivot_key(1.0 + 2.0**-43)  # 512 ulp apart: different keys
    for second, win in ((1.0 + 2.0**-46, 0), (1.0 + 2.0**-43, 1), (-1.0, 0)):
        F = _eye_front(4)
        F[0, 0], F[1, 0] = 1.0, second
        F[1, 1] = 3.0
        assert optimistic_lu(F, 4)["rperm"][0] == win, second
    # lane order, not current position: step 0 moves row 0 to position 2 (row 2 wins); at step 1 rows 0 and 1 tie in column 1 and row 0
    # (lane 0) wins although it now sits below row 1
    F = np.array([[1.0, 2.0, 0.0], [0.0, -2.0, 1.0], [4.0, 0.0, 1.0]])
    r = optimistic_lu(F, 3)
    assert r["rperm"].tolist() == [2, 0, 1]
