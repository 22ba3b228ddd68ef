"""The block 1-norm estimator and the xGERFS formulas of csrc/hs_condest.hip, checked on the CPU through their NumPy restatement
(tests/normest_mirror.py): bounds on random dense and sparse matrices, exact cases, agreement with scipy's onenormest, berr / ferr."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import normest_mirror as M


def _est(B, t=2, itmax=5, seed=123):
    Bh = B.conj().T
    n = B.shape[0]
    return M.normest1(lambda X: B @ X, lambda X: Bh @ X, n, t=t, itmax=itmax, seed=seed, cplx=np.iscomplexobj(B))


def _norm1(B):
    return float(abs(B).sum(axis=0).max())


def test_hash_columns_are_deterministic_and_balanced():
    a = M.pm1(4096, 1, 0, 123)
    assert np.array_equal(a, M.pm1(4096, 1, 0, 123))
    assert set(np.unique(a)) == {-1.0, 1.0} and abs(a.sum()) < 300
    assert not np.array_equal(a, M.pm1(4096, 2, 0, 123))
    assert not np.array_equal(a, M.pm1(4096, 1, 65, 123))
    assert not np.array_equal(a, M.pm1(4096, 1, 0, 124))
    # the key of the device: splitmix64(splitmix64(seed) ^ salt << 8 ^ col), entry i = low bit of splitmix64(key ^ i)
    assert M.col_key(123, 1, 0) == int(M._sm64(np.uint64(int(M._sm64(np.uint64(123))) ^ 1)))


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("t", [1, 2, 4])
def test_bounds_on_random_dense_matrices(seed, t):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 60))
    B = rng.standard_normal((n, n)) * np.exp(rng.standard_normal((1, n)))  # columns of very different weight
    if seed % 3 == 0:
        B = B + 1j * rng.standard_normal((n, n))
    est, ns = _est(B, t=t, seed=seed)
    true = _norm1(B)
    assert est <= true * (1 + 1e-12)
    assert est >= true / 3
    assert ns % t == 0 and ns <= 2 * t * 6


@pytest.mark.parametrize("seed", range(8))
def test_bounds_on_random_sparse_inverses(seed):
    rng = np.random.default_rng(100 + seed)
    n = 200
    A = sp.random(n, n, density=0.02, random_state=seed, format="csc") + sp.diags(rng.uniform(1, 3, n))
    lu = spla.splu(A.tocsc())
    est, _ = M.normest1(lambda X: lu.solve(X), lambda X: lu.solve(X, trans="T"), n, t=2)
    true = _norm1(np.linalg.inv(A.toarray()))
    assert true / 3 <= est <= true * (1 + 1e-12)


@pytest.mark.parametrize("t", [1, 2, 3])
def test_exact_on_diagonal_and_rank_one_plus_identity(t):
    rng = np.random.default_rng(7)
    d = rng.standard_normal(50)
    D = np.diag(d)
    assert _est(D, t=t)[0] == pytest.approx(np.abs(d).max(), rel=1e-14)
    u, v = rng.standard_normal(40), rng.standard_normal(40)
    R = np.eye(40) + np.outer(u, v)
    assert _est(R, t=t)[0] == pytest.approx(_norm1(R), rel=1e-13)


def test_agrees_with_scipy_onenormest_where_scipy_is_exact():
    hits = 0
    for seed in range(20):
        rng = np.random.default_rng(seed)
        n = 80
        B = sp.random(n, n, density=0.05, random_state=seed, format="csr") + sp.eye(n)
        true = _norm1(B)
        ref = spla.onenormest(B, t=2)
        if ref != pytest.approx(true, rel=1e-14):
            continue
        hits += 1
        est, _ = M.normest1(lambda X: B @ X, lambda X: B.T @ X, n, t=2, seed=seed)
        assert est == pytest.approx(ref, rel=1e-13)
    assert hits >= 10


def test_parallel_sign_columns_are_redrawn():
    """t = 2 on a rank-one matrix: both sign columns come out parallel; the second is re-drawn from the hash."""
    n = 32
    u = np.linspace(1, 2, n)
    B = np.outer(u, np.ones(n))
    calls = []

    def apply_h(S):
        calls.append(S.copy())
        return B.T @ S

    est, _ = M.normest1(lambda X: B @ X, apply_h, n, t=2)
    assert est == pytest.approx(_norm1(B), rel=1e-14)
    S = calls[0]
    assert abs(S[:, 0] @ S[:, 1]) != n


def _refine_dense(A, b, F, itmax=5):
    """xGERFS with a perturbed inverse F for op(A) = A (the driver of hs_ldiv_refine_* on dense matrices)."""
    n = A.shape[0]
    nz = int((A != 0).sum(axis=1).max()) + 1
    x = F @ b
    lst, steps = 3.0, 0
    while True:
        berr, r, w = M.gerfs_berr(A, x, b, nz)
        if not (berr > M.EPS and 2 * berr <= lst and steps < itmax):
            break
        x = x + F @ r
        lst, steps = berr, steps + 1
    return x, berr, r, w, nz, steps


@pytest.mark.parametrize("cplx", [False, True])
def test_gerfs_berr_and_ferr_formulas(cplx):
    rng = np.random.default_rng(3)
    n = 40
    A = rng.standard_normal((n, n)) + n * np.eye(n)
    if cplx:
        A = A + 1j * rng.standard_normal((n, n))
    x_true = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
    b = A @ x_true
    F = np.linalg.inv(A) @ (np.eye(n) + 1e-6 * rng.standard_normal((n, n)))  # an inexact inverse, like a compressed factorization
    x, berr, r, w, nz, steps = _refine_dense(A, b, F)
    # berr restated directly: max_i |r_i| / (|b| + |A| |x|)_i with cabs1
    c1 = (lambda z: np.abs(z.real) + np.abs(z.imag)) if cplx else np.abs
    direct = max(c1(b - A @ x)[i] / (c1(b)[i] + sum(c1(A[i, j]) * c1(x[j]) for j in range(n))) for i in range(n))
    assert berr == pytest.approx(direct, rel=1e-12)
    assert steps > 0 and berr <= 10 * np.finfo(float).eps
    _, berr0, _, _, _, _ = _refine_dense(A, b, F, itmax=0)
    assert berr0 > 1e4 * berr
    # ferr: the estimator on diag(v) A^-H (the device uses F^-H; exact inverse here) against the exact bound
    safe1 = nz * M.SAFMIN
    v = np.where(w > safe1 / M.EPS, c1(r) + nz * M.EPS * w, c1(r) + nz * M.EPS * w + safe1)
    Ai = np.linalg.inv(A)
    B = np.diag(v) @ Ai.conj().T
    est, _ = _est(B)
    ferr = est / c1(x).max()
    exact = M.gerfs_ferr_exact(A, x, r, w, nz)
    assert exact / 3 <= ferr <= exact * (1 + 1e-12)
    assert ferr >= np.abs(x - x_true).max() / np.abs(x).max() * 0.5  # (bounds the true error up to the estimator's looseness)


def test_normestinv_wrapper_maps_the_adjoint_codes():
    """normestinv(trans) applies op(F)^-1 forward and its adjoint backward: the estimate is ||op(A)^-1||_1."""
    rng = np.random.default_rng(5)
    n = 30
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) + 5 * np.eye(n)
    Ai = np.linalg.inv(A)

    def solve(X, tr):
        return {"N": Ai, "T": Ai.T, "C": Ai.conj().T}[tr] @ X

    for trans, op in ((0, Ai), (1, Ai.T), (2, Ai.conj().T)):
        est, ns = M.normestinv(solve, n, trans=trans, cplx=True)
        assert _norm1(op) / 3 <= est <= _norm1(op) * (1 + 1e-12)
        assert ns >= 4


def test_c_abi_declares_the_accuracy_tools():
    import os

    import hsamd

    hs = hsamd.load()
    for name in ("hs_opnorm", "hs_normestinv", "hs_condest", "hs_ldiv_refine_d", "hs_ldiv_refine_z", "hs_ldiv_refine_dev_d", "hs_ldiv_refine_dev_z"):
        assert name in hs._lib.EXPORTS
    with open(os.path.join(os.path.dirname(hs._lib.CSRC), "..", "include", "hs_solver.h")) as f:
        hdr = f.read()
    assert "int hs_condest(hs_handle* F, int p, int64_t t" in hdr
    for name in ("opnorm", "opnormestinv", "condest", "ldiv_refine"):
        assert callable(getattr(hs, name))
    with pytest.raises(ValueError, match="ArgumentError"):
        hs.solver._pcode(2)
