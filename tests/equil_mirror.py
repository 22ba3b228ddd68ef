"""NumPy restatement of the sweep rule of hs_options.equilibrate (csrc/kernels_equil.hip; include/hs_solver.h).

``A_s = 2^er A 2^ec`` with integer exponents found by Ruiz sweeps in the infinity norm.  One sweep: the row maxima ``r_i`` and column
maxima ``c_j`` of ``ldexp(|a|, er[row] + ec[col])`` (``|a| = fabs``, ``|re| + |im|`` for complex entries); with ``frexp(m) = (f, e)``,
``f`` in ``[0.5, 1)``, ``floor(log2 m) + 1 = e`` and the exponent moves by ``-floor(e / 2)``; a zero (or non-finite) maximum moves
nothing; rows and columns move together, from the same maxima.  The first sweep that moves nothing ends the sweeps, ``MAX_SWEEPS`` at
most.  ldexp by an integer is exact and a maximum does not depend on the order it is taken in, so the device's exponents equal these."""
import numpy as np
import scipy.sparse as sp

MAX_SWEEPS = 16


def magnitudes(A):
    """(rows, cols, |a|) of the stored entries of ``A`` in CSC order."""
    A = sp.csc_matrix(A)
    A.sort_indices()
    n = A.shape[1]
    cols = np.repeat(np.arange(n), np.diff(A.indptr))
    rows = A.indices.astype(np.int64)
    d = A.data
    mag = np.abs(d.real) + np.abs(d.imag) if np.iscomplexobj(d) else np.abs(d)
    return rows, cols, mag.astype(np.float64)


def step(m):
    """The change of an exponent whose row / column maximum is ``m`` (arrays)."""
    ok = np.isfinite(m) & (m > 0.0)
    _, e = np.frexp(np.where(ok, m, 1.0))
    return np.where(ok, -(e.astype(np.int64) // 2), 0)


def maxima(rows, cols, mag, er, ec, n):
    """Row and column maxima of the scaled magnitudes (0 for a row / column without a positive entry; NaN never enters)."""
    m = np.ldexp(mag, (er[rows] + ec[cols]).astype(np.int32))
    m = np.where(m > 0.0, m, 0.0)  # (drops NaN)
    rmax = np.zeros(n)
    cmax = np.zeros(n)
    np.maximum.at(rmax, rows, m)
    np.maximum.at(cmax, cols, m)
    return rmax, cmax


def equilibrate(A):
    """``(er, ec, sweeps)``: int32 exponents and the number of sweeps run (the one that moved nothing included)."""
    n = A.shape[0]
    rows, cols, mag = magnitudes(A)
    er = np.zeros(n, dtype=np.int64)
    ec = np.zeros(n, dtype=np.int64)
    sweeps = 0
    for _ in range(MAX_SWEEPS):
        rmax, cmax = maxima(rows, cols, mag, er, ec, n)
        dr, dc = step(rmax), step(cmax)
        sweeps += 1
        if not dr.any() and not dc.any():
            break
        er += dr
        ec += dc
    return er.astype(np.int32), ec.astype(np.int32), sweeps


def scaled(A, er, ec):
    """``2^er A 2^ec`` with A's pattern (explicit zeros kept), entry by entry with ldexp."""
    A = sp.csc_matrix(A)
    A.sort_indices()
    rows, cols, _ = magnitudes(A)
    s = (er[rows].astype(np.int64) + ec[cols]).astype(np.int32)
    d = A.data
    v = np.ldexp(d.real, s) + 1j * np.ldexp(d.imag, s) if np.iscomplexobj(d) else np.ldexp(d, s)
    return sp.csc_matrix((v, A.indices.copy(), A.indptr.copy()), shape=A.shape)


def scale_rows(B, e):
    """``2^e B`` row by row (vector or block), with ldexp."""
    B = np.asarray(B)
    s = e.astype(np.int32).reshape((-1,) + (1,) * (B.ndim - 1))
    if np.iscomplexobj(B):
        return np.ldexp(B.real, s) + 1j * np.ldexp(B.imag, s)
    return np.ldexp(B, s)


def badly_scaled(A, seed, span):
    """``D1 A D2`` with seeded random power-of-two diagonals, exponents uniform in ``[-span, span]``; also returns the two exponent vectors."""
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    e1 = rng.integers(-span, span + 1, n).astype(np.int32)
    e2 = rng.integers(-span, span + 1, n).astype(np.int32)
    return scaled(A, e1, e2), e1, e2
