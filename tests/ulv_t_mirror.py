"""NumPy statement of the transposed / adjoint ULV solve of an HSS matrix on the oracle's factors (oracle.hs_hss.rs_factor), and of the
front-level formulas hs_ldiv_ulv_* applies around it.  Not a test module: tests/test_ulv_t_host.py checks it against dense solves; the
device implementation (csrc/hs_hss.hip, csrc/kernels_ulv_t.hip, csrc/hs_api.hip) follows the same steps.

Every non-root node keeps ONE skeleton for rows and columns, so with E = [I -T; 0 I] and F = [I 0; -T^T I] (front order [R; S]) E^T = F,
and the local matrix M = E^-1 X F^-1 has M^T = E^-1 X^T F^-1: the transposed elimination is the same tree walk with the blocks of X read
along their other index.  In the oracle's storage (Lc = X_SR X_RR^-1, Rc = X_RR^-1 X_RS, lu = LU of X_RR):

  forward, leaves to root:   b_R -= op(T) b_S;   z = op(X_RR)^-T b_R;   b_S -= op(Rc)^T b_R   (b_R before the solve)
  root:                      op(M0)^-T
  backward, root to leaves:  x_R = z - op(Lc)^T x_S;   x_S -= op(T)^T x_R

op = identity (transpose) or conj (adjoint)."""
import numpy as np
import scipy.linalg as sla


def rs_solve_t(F, B, adjoint=False):
    """X = H^-T B (adjoint: H^-H B) through the skeletonization factors of `rs_factor`."""
    H, nodes = F.H, F.H.nodes
    op = np.conj if adjoint else (lambda a: a)
    tr = 2 if adjoint else 1
    B2 = B.reshape(H.n, -1).astype(np.result_type(H.dtype, B.dtype))
    bh, zR = {}, {}
    for lv in range(H.nlevels - 1, 0, -1):
        for i in H.level(lv):
            x = nodes[i]
            loc = B2[x.lo : x.hi] if x.left < 0 else np.vstack([bh[x.left], bh[x.right]])
            bS, bR = loc[x.p[: x.r]], loc[x.p[x.r :]]
            bR = bR - op(x.T) @ bS
            zR[i] = sla.lu_solve(F.lu[i], bR, trans=tr, check_finite=False) if F.lu[i] is not None else bR
            bh[i] = bS - (op(F.Rc[i]).T @ bR if bR.shape[0] else 0)
    x = nodes[0]
    loc = B2 if x.left < 0 else np.vstack([bh[x.left], bh[x.right]])
    xs = {0: sla.lu_solve(F.root_lu, loc, trans=tr, check_finite=False)}
    X = np.zeros_like(B2)
    for lv in range(0, H.nlevels):
        for i in H.level(lv):
            x = nodes[i]
            if i == 0:
                loc = xs[0]
            else:
                xS = xs[i]
                xR = zR[i] - op(F.Lc[i]).T @ xS
                loc = np.empty((x.m, B2.shape[1]), B2.dtype)
                loc[x.p[x.r :]] = xR
                loc[x.p[: x.r]] = xS - op(x.T).T @ xR
            if x.left < 0:
                X[x.lo : x.hi] = loc
            else:
                rl = nodes[x.left].r
                xs[x.left], xs[x.right] = loc[:rl], loc[rl:]
    return X.reshape(B.shape)


# ---- one front [D Aib; Abi Abb] with Abi = C_L Z_L, Aib = C_R Z_R, W = D^-1 C_R; `dsolve(b, trans)` applies op(D)^-1 (trans 0) or op(D)^-T --

def front_forward(trans, dsolve, W, ZR, CL, ZL, bi, bb):
    """The front's step of the sweep leaves -> root: returns (what stays in B[int], the updated B[bnd])."""
    op = np.conj if trans == 2 else (lambda a: a)
    if trans == 0:
        t = dsolve(bi, 0)
        return t, bb - CL @ (ZL @ t)
    return bi, bb - op(ZR).T @ (op(W).T @ bi)


def front_backward(trans, dsolve, W, ZR, CL, ZL, ti, xb):
    """The front's step of the sweep root -> leaves: the solution on the interior rows, given B[int] of the forward step and x on bnd."""
    op = np.conj if trans == 2 else (lambda a: a)
    if trans == 0:
        return ti - W @ (ZR @ xb)
    return dsolve(ti - op(ZL).T @ (op(CL).T @ xb), trans)


def block_dsolve_t(trans, a11solve, s22solve, W12, Z12, C21, Z21, n1):
    """op(D)^-T for D = [A11 C12 Z12; C21 Z21 A22] from A11, S22 = A22 - A21 A11^-1 A12, W12 = A11^-1 C12 (`*solve(b)` apply op(.)^-T)."""
    op = np.conj if trans == 2 else (lambda a: a)

    def solve(b):
        b1, b2 = b[:n1], b[n1:]
        b2 = b2 - op(Z12).T @ (op(W12).T @ b1)
        x2 = s22solve(b2)
        b1 = b1 - op(Z21).T @ (op(C21).T @ x2)
        return np.vstack([a11solve(b1), x2])

    return solve
