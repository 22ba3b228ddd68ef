"""NumPy restatement of the optimistic LU of a dense front (csrc/kernels_panel.hip, csrc/hs_sched.h): the elimination order and the growth
check the kernels implement, so a test can compare the device's pivots, factors and growth flag with it.

  * 32-column panels, right-looking: the trailing columns and the rows below are brought up to date before a panel is factored;
  * the pivot candidates of a panel are its own w = min(32, ni - c0) diagonal-block rows, never a row below the block;
  * the pivot key is abs1 (|x| for Float64, |re| + |im| for ComplexF64) with the low 8 bits of its IEEE bit pattern cleared; equal keys
    go to the lowest row, counted by its position at the START of the panel (the kernels keep one row per lane and permute implicitly,
    so a row that an earlier step of the same panel displaced keeps its lane);
  * multipliers for every row below the pivot, down to the last row of the front (rows >= ni are the Abi * U^-1 part of LF);
  * the growth flag (NodeDesc::growth) rises when a multiplier of a row < ni exceeds HS_GROWTH_MAX = 4 in abs1, when such a multiplier
    is NaN, or when a diagonal-block column has no nonzero candidate left on its own rows.  Rows >= ni never raise it.

Where the kernels differ from each other the mirror follows the default ones: in a column with no nonzero candidate, panel_pivot_opt_kernel
(Float64) and panel_pivot_opt_z_kernel (ComplexF64) both take the first row still in play as the pivot and eliminate nothing (multipliers
0); the general panel_pivot_kernel (HS_PANEL_OPT=0 / HS_PANEL_OPT_Z=0) leaves the row where it is instead.  The flag rises either way and
the level is redone, so the factors of such a front are not compared.  Float64 multiplies by the reciprocal of the pivot, ComplexF64
divides (Smith's algorithm); the mirror divides -- the difference is a rounding error, far inside the tolerances of the tests."""
import numpy as np

PB = 32
GROWTH_MAX = 4.0


def abs1(x):
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return np.abs(x.real) + np.abs(x.imag)
    return np.abs(x)


def pivot_key(x):
    """The 64-bit key of the kernels' pivot search, without the lane bits: abs1 bits with the low 8 bits cleared."""
    a = np.ascontiguousarray(abs1(x), dtype=np.float64)
    return a.view(np.uint64) & np.uint64(~0xFF & ((1 << 64) - 1))


def optimistic_lu(F, ni):
    """Optimistic LU of the interior block of a front F (m x m, front order [int; bnd]).

    Returns a dict: rperm (P*Aii = L*U, (P x)[i] = x[rperm[i]]), L (ni x ni unit lower), U (ni x ni upper), Lbi (nb x ni, Abi * U^-1),
    lmax (largest abs1 multiplier over rows < ni, NaN if one was NaN), flag (the growth flag), bad (a column without a candidate),
    gap (smallest relative margin between the winning pivot and the runner-up over all steps; 1.0 if no step had two candidates)."""
    F = np.asarray(F)
    m = F.shape[0]
    A = np.array(F[:, :ni], dtype=np.complex128 if np.iscomplexobj(F) else np.float64)
    rperm = np.arange(ni)
    bad = False
    lmax, nan = 0.0, False
    gap = 1.0
    for c0 in range(0, ni, PB):
        w = min(PB, ni - c0)
        c1 = c0 + w
        alive = np.ones(w, dtype=bool)
        order = []
        P = A[c0:, c0:c1]  # the panel: the block rows (lanes 0..w-1, panel-start order) and every row below
        for k in range(w):
            keys = np.where(alive, pivot_key(P[:w, k]), np.uint64(0))
            best = keys.max()
            if best == 0:  # nothing left on the block's own rows
                bad = True
                win = int(np.flatnonzero(alive)[0])
                order.append(win)
                alive[win] = False
                continue
            win = int(np.flatnonzero(keys == best)[0])  # lowest lane among equal keys
            a = abs1(P[:w, k])
            rest = a[alive & (np.arange(w) != win)]
            if rest.size:
                gap = min(gap, (a[win] - rest.max()) / a[win])
            order.append(win)
            alive[win] = False
            piv = P[win, k]
            rows = np.concatenate([np.flatnonzero(alive), np.arange(w, P.shape[0])])
            l = P[rows, k] / piv
            P[rows, k] = l
            P[np.ix_(rows, np.arange(k + 1, w))] -= np.outer(l, P[win, k + 1:w])
            below_ni = rows + c0 < ni
            if below_ni.any():
                lb = abs1(l[below_ni])
                if np.isnan(lb).any():
                    nan = True
                else:
                    lmax = max(lmax, float(lb.max()))
        order = np.asarray(order)
        A[c0:c1] = A[c0 + order]  # position c0+k takes the row that won step k
        rperm[c0:c1] = rperm[c0 + order]
        if c1 < ni:  # trailing update: U12 = L11^-1 * (P A12), A22 -= L21 * U12
            L11 = np.tril(A[c0:c1, c0:c1], -1) + np.eye(w)
            A[c0:c1, c1:] = np.linalg.solve(L11, A[c0:c1, c1:]) if w > 1 else A[c0:c1, c1:]
            A[c1:, c1:] -= A[c1:, c0:c1] @ A[c0:c1, c1:]
    L = np.tril(A[:ni], -1) + np.eye(ni)
    U = np.triu(A[:ni])
    if nan:
        lmax = float("nan")
    flag = bool(bad or nan or lmax > GROWTH_MAX)
    return dict(rperm=rperm, L=L, U=U, Lbi=A[ni:].copy(), lmax=lmax, flag=flag, bad=bad, gap=gap)


def good_front(rng, ni, nb, cplx, scale=None):
    """A front on which optimistic pivoting succeeds and still swaps rows: Gaussian 32 x 32 diagonal blocks of Aii scaled by
    ~10 sqrt(ni), O(1) entries everywhere else."""
    m = ni + nb

    def rnd(*shape):
        a = rng.standard_normal(shape)
        return a + 1j * rng.standard_normal(shape) if cplx else a

    F = rnd(m, m)
    s = 10.0 * np.sqrt(max(ni, 1)) if scale is None else scale
    for c0 in range(0, ni, PB):
        c1 = min(ni, c0 + PB)
        F[c0:c1, c0:c1] = s * rnd(c1 - c0, c1 - c0)
    return F


def find_good_front(rng, ni, nb, cplx, lmax_max=3.0, gap_min=1e-10, tries=20):
    """good_front with the margins the kernel tests need: the mirror's largest multiplier <= lmax_max and no two pivot candidates within
    gap_min relative.  Returns (F, mirror result)."""
    for _ in range(tries):
        F = good_front(rng, ni, nb, cplx)
        r = optimistic_lu(F, ni)
        if not r["flag"] and r["lmax"] <= lmax_max and r["gap"] >= gap_min:
            return F, r
    raise AssertionError(f"no front with margins found for ni={ni}, nb={nb}")
