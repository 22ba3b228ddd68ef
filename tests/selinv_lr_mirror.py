"""NumPy statement of what hs_selinv_lr (csrc/hs_selinv.hip) computes: the selected-inversion recurrence of tests/selinv_mirror.py run
through the LOW-RANK Gauss transforms of a compressed factorization, over a tree of oracle FactorNodes (oracle/hs_oracle_lr.py).

A compressed front keeps R = D^-1 Aib ~= W Z_R and L = Abi D^-1 ~= C_L Y as LowRankMatrix objects (A = U V'):
    R = U V'  ->  W = U (ni x rR),  Z_R = V' (rR x nb);        L = U V'  ->  C_L = U (nb x rL),  Y = V' (rL x ni).
With Zbb = Z[bnd, bnd] known, in the order the device issues the products:
    T1 = -Z_R Zbb (rR x nb),   T2 = -Zbb C_L (nb x rL),   T3 = T1 C_L (rR x rL)
    Z[int, bnd] = W T1,   Z[bnd, int] = T2 Y,   Z[int, int] = D^-1 - (W T3) Y
No product has an nb-wide or (ni + nb)-tall operand except T1, T2 and the writes into Z.  A transform of rank 0 drops its terms.  A front
whose L, R are dense matrices runs the dense recurrence.  On the device W = U^-1 G and Y = Z_L' L^-1 P come out of the blocked
substitutions on rR columns and ni + rL rows; the flop counts of both forms below follow the device's 256-blocks."""
import numpy as np

from selinv_mirror import _dense, dense_d, nodes_of, root_schur


def _is_lr(M):
    return hasattr(M, "U") and hasattr(M, "V")


def selinv_lr(F, n):
    """Dense n x n array holding (F^-1)[i, j] wherever the recurrence produces it and NaN elsewhere; also the number of fronts served
    through low-rank transforms and the largest rank met."""
    cplx = any(np.iscomplexobj(dense_d(x.D)) for x in nodes_of(F))
    Z = np.full((n, n), np.nan, dtype=np.complex128 if cplx else np.float64)
    lowrank, maxrank = 0, 0
    if len(F.bnd):
        b = F.bnd - 1
        Z[np.ix_(b, b)] = np.linalg.inv(root_schur(F))
    for x in nodes_of(F):  # parents first
        i, b = x.int - 1, x.bnd - 1
        Dinv = np.linalg.inv(dense_d(x.D)) if len(i) else np.zeros((0, 0))
        if len(b) == 0:
            Z[np.ix_(i, i)] = Dinv
            continue
        Zbb = Z[np.ix_(b, b)]
        assert not np.isnan(Zbb).any(), "a front's boundary block must come complete from its ancestors"
        if not (_is_lr(x.R) or _is_lr(x.L)):
            R, L = _dense(x.R), _dense(x.L)
            Z[np.ix_(i, b)] = -R @ Zbb
            Z[np.ix_(b, i)] = -Zbb @ L
            Z[np.ix_(i, i)] = Dinv + R @ Zbb @ L
            continue
        assert _is_lr(x.R) and _is_lr(x.L)
        W, ZR = x.R.U, x.R.V.conj().T
        CL, Y = x.L.U, x.L.V.conj().T
        lowrank += 1
        maxrank = max(maxrank, W.shape[1], CL.shape[1])
        T1 = -ZR @ Zbb
        T2 = -Zbb @ CL
        T3 = T1 @ CL
        Z[np.ix_(i, b)] = W @ T1
        Z[np.ix_(b, i)] = T2 @ Y
        Z[np.ix_(i, i)] = Dinv - (W @ T3) @ Y
    return Z, lowrank, maxrank


def _blocks(ni):
    for kb in range((ni + 255) // 256 - 1, -1, -1):
        k0 = kb * 256
        yield k0, min(256, ni - k0)


def dense_form_flops(ni, nb, cplx=False):
    """Real flops of the products hs_selinv issues for one dense front (csrc/hs_selinv.hip, dense_form_flops): the two m-sized products and,
    per 256-block of the interior, the product with the inverse diagonal block and the update of both substitutions."""
    m = ni + nb
    f = ni * nb * nb + m * ni * nb
    for k0, wk in _blocks(ni):
        f += wk * nb * wk + wk * (ni - k0) * wk + k0 * nb * wk + k0 * (ni - k0) * wk
        f += m * wk * wk + m * k0 * wk
    return (8.0 if cplx else 2.0) * f


def lr_form_flops(ni, nb, rL, rR, cplx=False):
    """Real flops of the products hs_selinv_lr issues for one low-rank front."""
    f = rR * nb * nb + nb * rL * nb + rR * rL * nb           # T1, T2, T3
    for k0, wk in _blocks(ni):
        f += wk * rR * wk + wk * (ni - k0) * wk + k0 * rR * wk + k0 * (ni - k0) * wk   # U^-1 [Vi | Vg]
        f += (ni + rL) * wk * wk + (ni + rL) * k0 * wk                                 # [Tm; Z_L'] L^-1
    f += ni * nb * rR + ni * rL * rR                          # W T1, W T3
    f += nb * ni * rL + (ni * ni * rL if rR > 0 else 0)       # T2 Y', (W T3) Y'
    return (8.0 if cplx else 2.0) * f


def tree_flops(F):
    """(rank-structured form, dense form) summed over the fronts of an oracle tree."""
    lr = dn = 0.0
    for x in nodes_of(F):
        ni, nb = len(x.int), len(x.bnd)
        cplx = np.iscomplexobj(dense_d(x.D))
        d = dense_form_flops(ni, nb, cplx)
        dn += d
        if nb and ni and _is_lr(x.R) and _is_lr(x.L):
            lr += lr_form_flops(ni, nb, x.L.U.shape[1], x.R.U.shape[1], cplx)
        else:
            lr += d
    return lr, dn
