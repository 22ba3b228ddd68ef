"""NumPy statement of the solves with A1 = A + U V^H from solves with A (csrc/hs_mod.hip, hs_mod_*) and of the summation order of its
inner-product kernel (csrc/kernels_mod.hip: mod_inner).

With Z = A^-1 U, W = A^-H V and C = I + V^H Z:

  A1^-1 B = Y - Z C^-1 (V^H Y),            Y = A^-1 B
  A1^-H B = Y - W C^-H (U^H Y),            Y = A^-H B
  A1^-T B = Y - conj(W) C^-T (U^T Y),      Y = A^-T B

`solve(X, trans)` stands for the stored factorization: op(A)^-1 X for trans in "N", "T", "H"."""
from fractions import Fraction

import numpy as np

SLAB = 2048  # HS_MOD_SLAB


class Modified:
    def __init__(self, solve, U, V):
        self.solve, self.U, self.V = solve, U, V
        self.k = U.shape[1]
        self.Z = solve(U, "N")
        self.C = np.eye(self.k, dtype=self.Z.dtype) + V.conj().T @ self.Z
        self.W = None  # built by the first transposed call, serves "T" and "H"

    def ldiv(self, B, trans="N"):
        Y = self.solve(B, trans)
        if self.k == 0:
            return Y
        if trans == "N":
            return Y - self.Z @ np.linalg.solve(self.C, self.V.conj().T @ Y)
        if self.W is None:
            self.W = self.solve(self.V, "H")
        if trans == "H":
            return Y - self.W @ np.linalg.solve(self.C.conj().T, self.U.conj().T @ Y)
        return Y - self.W.conj() @ np.linalg.solve(self.C.T, self.U.T @ Y)


def fma(a, b, c):
    """round(a * b + c) with one rounding (float(Fraction) rounds correctly)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _chain(acc, a, y, rows, order):
    for r0 in range(0, len(rows), 4):  # one MFMA: four k-slots
        grp = rows[r0 : r0 + 4]
        for q in order:
            if q < len(grp) and grp[q] is not None:
                acc = fma(a[grp[q]], y[grp[q]], acc)
    return acc


def inner(P, Y, conj=False, order=(0, 1, 2, 3)):
    """T = op(P)^H Y in the order of mod_inner: per slab of SLAB rows a chain of fused multiply-adds from zero, then the slabs added in
    order.  Float64: steps of 8 rows, first rows 0 2 4 6 of the step (one MFMA, k-slot g holds row 2 g), then rows 1 3 5 7.  ComplexF64: steps
    of 4 rows; the real part takes re(a) re(y) of the four rows, then -im(a) im(y), the imaginary part re(a) im(y), then im(a) re(y), with
    a = conj(P) (conj=False: T = P^H Y) or P (conj=True: T = P^T Y).  `order`: the k-slots of one MFMA in the order they are added."""
    n, k = P.shape
    m = Y.shape[1]
    cx = np.iscomplexobj(P) or np.iscomplexobj(Y)
    T = np.zeros((k, m), dtype=np.complex128 if cx else np.float64)
    for i in range(k):
        for c in range(m):
            tot = None
            for s0 in range(0, n, SLAB):
                s1 = min(n, s0 + SLAB)
                if not cx:
                    acc = 0.0
                    for rb in range(s0, s1, 8):
                        for half in (0, 1):
                            rows = [rb + 2 * g + half if rb + 2 * g + half < s1 else None for g in range(4)]
                            acc = _chain(acc, P[:, i], Y[:, c], rows, order)
                    part = acc
                else:
                    a = P[:, i] if conj else P[:, i].conj()
                    ar, ai, yr, yi = a.real, a.imag, Y[:, c].real, Y[:, c].imag
                    re = im = 0.0
                    for rb in range(s0, s1, 4):
                        rows = [rb + g if rb + g < s1 else None for g in range(4)]
                        re = _chain(re, ar, yr, rows, order)
                        re = _chain(re, -ai, yi, rows, order)
                        im = _chain(im, ar, yi, rows, order)
                        im = _chain(im, ai, yr, rows, order)
                    part = complex(re, im)
                tot = part if tot is None else tot + part
            T[i, c] = tot
    return T
