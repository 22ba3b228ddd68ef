"""NumPy restatement of the symmetric schedule (Sched::sym, csrc/hs_sched.h; hs_options.symmetric), on top of lu_mirror.optimistic_lu.

A front F == F.T (plain transpose) is eliminated block column by block column.  Under optimistic pivoting every row swap stays inside a
32-row diagonal block and the update a block column k applies to the blocks right of and below it is A_ik A_kk^-1 A_kj whatever P_k is, so
the trailing matrix stays symmetric: only its lower strips are updated, and the blocks above the diagonal are rebuilt by transposition
just before they are needed.

Invariant (the one csrc/hs_sched.h keeps): when a column range [c0, c1) is about to be factored its diagonal square is whole and the rows
below it are up to date; the blocks of the trailing interior strictly above the diagonal are never read as matrix entries, only written as
U.  sym_schedule_lu poisons with NaN everything the invariant says is never read; a NaN in its result means the schedule read one.

schedule_flops restates the plain updates (Sched::gemm calls) of the production schedule of a lone Float64 front, with and without the
strips, so the executed-flop ratio of a shape can be counted on the host."""
import numpy as np

from lu_mirror import PB, optimistic_lu

SYM_STRIP = 256                   # HS_SYM_STRIP (csrc/hs_common.h): unit of the column strips of the lower-triangle updates
LA_MIN = {False: 1536, True: 1200}  # Sched::factor_fronts: look-ahead from this many interior columns on ...
LA_NB = {False: 1024, True: 512}    # ... in block columns of this width (Float64, ComplexF64)


def sym_front(rng, ni, nb, cplx):
    """A symmetric front (plain transpose, also when complex) on which optimistic pivoting succeeds and still swaps rows:
    F = G + G.T with G Gaussian, every 32-block of the interior diagonal replaced by 10 sqrt(ni) (B + B.T)."""
    m = ni + nb

    def rnd(k):
        a = rng.standard_normal((k, k))
        return a + 1j * rng.standard_normal((k, k)) if cplx else a

    G = rnd(m)
    F = G + G.T
    s = 10.0 * np.sqrt(max(ni, 1))
    for c0 in range(0, ni, PB):
        c1 = min(ni, c0 + PB)
        B = rnd(c1 - c0)
        F[c0:c1, c0:c1] = s * (B + B.T)
    return F


def find_sym_front(rng, ni, nb, cplx, lmax_max=1.93, gap_min=3.7e-5, tries=20):
    """sym_front with the margins the kernel tests need, like lu_mirror.find_good_front: no growth flag, the mirror's largest multiplier
    <= lmax_max and no two pivot candidates within gap_min relative.  Draws again from the same generator until they hold (the first draw
    of default_rng(9300) for (300, 300) real has a gap of 3.68e-5).  Returns (F, mirror result)."""
    for _ in range(tries):
        F = sym_front(rng, ni, nb, cplx)
        r = optimistic_lu(F, ni)
        if not r["flag"] and r["lmax"] <= lmax_max and r["gap"] >= gap_min:
            return F, r
    raise AssertionError(f"no symmetric front with margins found for ni={ni}, nb={nb}")


def sym_schedule_lu(F, ni, nbcol, strip):
    """The symmetric schedule with block columns of `nbcol` and lower strips of `strip` columns (strip divides nbcol, both multiples of 32).
    Returns rperm, LF (m x ni: L\\U over Lbi), UR (L^-1 P Aib) and S, as the device stores them."""
    F = np.asarray(F)
    m = F.shape[0]
    nb = m - ni
    assert nbcol % strip == 0 and strip % PB == 0
    A = np.array(F, dtype=np.complex128 if np.iscomplexobj(F) else np.float64)
    # poison: the strictly upper strip-blocks of the interior and of Abb
    for j0 in range(0, ni, strip):
        A[:j0, j0:min(j0 + strip, ni)] = np.nan
    for j0 in range(0, nb, strip):
        A[ni:ni + j0, ni + j0:ni + min(j0 + strip, nb)] = np.nan
    rperm = np.arange(ni)
    for c0 in range(0, ni, nbcol):
        c1 = min(c0 + nbcol, ni)
        w = c1 - c0
        # whole diagonal square (strictly upper from strictly lower) and the future U row block, by transposition
        D = A[c0:c1, c0:c1]
        A[c0:c1, c0:c1] = np.tril(D) + np.tril(D, -1).T
        A[c0:c1, c1:ni] = A[c1:ni, c0:c1].T
        r = optimistic_lu(A[c0:, c0:c1], w)  # the block column: pivots among its own 32-row blocks, multipliers down to the last row
        lp = r["rperm"]
        A[c0:c1, c0:c1] = np.tril(r["L"], -1) + r["U"]
        A[c1:, c0:c1] = r["Lbi"]
        rperm[c0:c1] = c0 + lp
        A[c0:c1, :c0] = A[c0 + lp, :c0]        # left swaps
        A[c0:c1, c1:] = np.linalg.solve(r["L"], A[c0 + lp, c1:])  # U12 and the rows of UR = L^-1 P Aib
        for j0 in range(c1, ni, strip):        # trailing interior: lower strips, each from its own first row down to the end of the front
            j1 = min(j0 + strip, ni)
            A[j0:, j0:j1] -= A[j0:, c0:c1] @ A[c0:c1, j0:j1]
        A[c1:ni, ni:] -= A[c1:ni, c0:c1] @ A[c0:c1, ni:]
    for j0 in range(0, nb, strip):             # Schur complement: lower strips, then one mirror
        j1 = min(j0 + strip, nb)
        A[ni + j0:, ni + j0:ni + j1] -= A[ni + j0:, :ni] @ A[:ni, ni + j0:ni + j1]
    S = A[ni:, ni:]
    S = np.tril(S) + np.tril(S, -1).T
    return dict(rperm=rperm, LF=A[:, :ni].copy(), UR=A[:ni, ni:].copy(), S=S)


def sym_strip(extent, tiles_m, bn):
    """Sched::sym_strip: the strip width of a lower-triangle update of `extent` columns whose launches span `tiles_m` tile rows over the
    batch (bn: tile columns) -- at most 16 strips, widened until a launch carries about 1024 tiles, never to fewer than 4 strips."""
    lo = SYM_STRIP * max(1, -(-extent // (16 * SYM_STRIP)))
    hi = max(lo, extent // 4 // SYM_STRIP * SYM_STRIP)
    units = -(-1024 * bn // (SYM_STRIP * max(1, tiles_m)))
    return min(hi, max(lo, SYM_STRIP * units))


class _Count:
    """The Sched::gemm calls of one lone front with solve descriptors (the production default, hsk_front_batch mode 2): flops of the plain
    updates, each clipped to the front as the kernels clip it."""

    def __init__(self, ni, nb, sym, cplx=False):
        self.ni, self.nb, self.m, self.sym, self.cplx = ni, nb, ni + nb, sym, cplx
        self.flops = 0.0

    def gemm(self, cmat, r0, r1, c0, c1, k0, k1):
        rows = {"LF": self.m, "UR": self.ni, "SB": self.nb}[cmat]
        cols = self.ni if cmat == "LF" else self.nb
        M, N, K = min(r1, rows) - r0, min(c1, cols) - c0, min(k1, self.ni) - k0
        if M > 0 and N > 0 and K > 0:
            self.flops += 2.0 * M * N * K * (4.0 if self.cplx else 1.0)

    def gemm_lower(self, cmat, c0, c1, k0, k1):
        """Sched::gemm_lower; returns False when one strip covers the range (the full update)."""
        c1 = min(c1, self.ni if cmat == "LF" else self.nb)
        if c1 <= c0:
            return False
        rows = self.m if cmat == "LF" else self.nb
        W = sym_strip(c1 - c0, max(0, rows - c0 + 127) // 128, 64 if self.cplx else 128)
        for j0 in range(c0, c1, W):
            self.gemm(cmat, j0, 1 << 30, j0, min(c1, j0 + W), k0, k1)
        return c1 - c0 > W

    def trsm_rec(self, mat, r0, r1, c0, c1):
        if r0 >= self.ni or r1 - r0 <= 256:  # 256-row base case: products with the stored inverses (not plain updates)
            return
        mid = (r0 + r1) // 2
        self.trsm_rec(mat, r0, mid, c0, c1)
        if mid < self.ni:
            self.gemm(mat, mid, r1, c0, c1, r0, mid)
            self.trsm_rec(mat, mid, r1, c0, c1)

    def lu_rec(self, c0, c1):
        if c0 >= self.ni or c1 - c0 <= 256:  # one 256-column group: the panel chain and the in-place products below it
            return
        mid = (c0 + c1) // 2
        self.lu_rec(c0, mid)
        if mid < self.ni:
            self.trsm_rec("LF", c0, mid, mid, c1)
            if self.sym and c1 - mid >= 256:
                self.gemm_lower("LF", mid, c1, c0, mid)
            else:
                self.gemm("LF", mid, 1 << 30, mid, c1, c0, mid)
            self.lu_rec(mid, c1)

    def schur(self):
        if self.sym:
            self.gemm_lower("SB", 0, 1 << 30, 0, 1 << 30)
        else:
            self.gemm("SB", 0, 1 << 30, 0, 1 << 30, 0, 1 << 30)

    def run(self, lookahead=True):
        ni, BIG = self.ni, 1 << 30
        NB = LA_NB[self.cplx]
        if lookahead and ni >= LA_MIN[self.cplx] and ni > NB:
            self.lu_rec(0, NB)
            for c0 in range(0, ni, NB):
                c1, c2 = c0 + NB, c0 + 2 * NB
                if c1 < ni:
                    self.trsm_rec("LF", c0, c1, c1, c2)
                    self.gemm("LF", c1, BIG, c1, c2, c0, c1)
                    self.lu_rec(c1, c2)
                    self.trsm_rec("LF", c0, c1, c2, BIG)
                    if self.sym:
                        self.gemm_lower("LF", c2, BIG, c0, c1)
                    else:
                        self.gemm("LF", c1, BIG, c2, BIG, c0, c1)
                if self.nb > 0:
                    self.trsm_rec("UR", c0, c1, 0, BIG)
                    self.gemm("UR", c1, BIG, 0, BIG, c0, c1)
            if self.nb > 0:
                self.schur()
        else:
            P2 = PB
            while P2 < ni:
                P2 *= 2
            self.lu_rec(0, P2)
            if self.nb > 0:
                self.trsm_rec("UR", 0, P2, 0, BIG)
                self.schur()
        return self.flops


def schedule_flops(ni, nb, sym, cplx=False, lookahead=True):
    """Flops of the plain updates the production schedule launches for a lone front (lookahead=False: the recursive schedule at any size)."""
    return _Count(ni, nb, sym, cplx).run(lookahead)
