"""The balanced tile order of the enveloped plain updates (GemmOp::order, csrc/kernels_gemm.hip; DESIGN.md section 4 "Branch fronts") against
the same process with the order switched off (hsk_env_order_enable), leaf and branch envelopes on in both.  The order changes which
workgroup runs a tile, never the tile: every stored block and the solution must be EQUAL, not close, and the kernels' own flop count still
equals the host's.  Also one synthetic batch whose Schur tilings hit the edges of the permutation in one launch."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import prepare

pytestmark = pytest.mark.gpu


class env_order:
    """with env_order(hs, on): ... -- leaf and branch envelopes on, the tile order on / off; the previous settings come back afterwards"""

    def __init__(self, hs, on):
        self.L, self.on = hs._lib.lib(), on

    def __enter__(self):
        self.prev_leaf = self.L.hsk_envelope_enable(1)
        self.prev_branch = self.L.hsk_branch_envelope_enable(1)
        self.prev = self.L.hsk_env_order_enable(1 if self.on else 0)

    def __exit__(self, *a):
        self.L.hsk_env_order_enable(self.prev)
        self.L.hsk_branch_envelope_enable(self.prev_branch)
        self.L.hsk_envelope_enable(self.prev_leaf)


def _walk(nd):
    out, stack = [], [nd]
    while stack:
        x = stack.pop()
        out.append(x)
        stack += [c for c in (x.left, x.right) if c is not None]
    return out


def _odd_cube(hs):
    """The odd_cube of tests/test_branch_envelope_gpu.py, rebuilt: a 23 x 24 x 25 Poisson box with one DOF of a level-2 separator taken out
    of the matrix and of the tree, so that branch front has an odd ni and its Schur update runs the shifted edge route."""
    A, b, nd = hs.problems.make_problem((23, 24, 25), kind="poisson", nmax=1024, rhs="randn")
    g = int(np.asarray(nd.left.int)[0])  # 1-based
    keep = np.r_[0 : g - 1, g : A.shape[0]]
    A = sp.csc_matrix(A)[keep][:, keep]
    for x in _walk(nd):
        for name in ("int", "bnd"):
            v = np.asarray(getattr(x, name), dtype=np.int64)
            v = v[v != g]
            setattr(x, name, np.where(v > g, v - 1, v))
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    Ap = sp.csc_matrix(A[perm - 1][:, perm - 1])
    nd = hs.permuted(nd, hs.invperm(perm))
    assert [len(x.int) for x in _walk(nd) if x.left is not None and len(x.int) % 2], "no branch front with an odd ni"
    return dict(A=Ap, nd=nd, nd_loc=nd_loc, b=b[keep][perm - 1])


def _factor_counted(hs, P, on):
    """factorization with the device flop count on: (F, device flops)"""
    L = hs._lib.lib()
    with env_order(hs, on):
        assert L.hsk_op_flops_mode(1) == 0
        try:
            F = hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0)
            out = C.c_double()
            assert L.hsk_op_flops(C.byref(out)) == 0
        finally:
            L.hsk_op_flops_mode(0)
    return F, out.value


@pytest.mark.parametrize("name", ["poisson3d_32", "odd_cube", "helmholtz3d_32"])
def test_order_on_equals_off_bitwise(hs, name):
    """poisson3d_32: the root (ni = 2048) on the look-ahead schedule, level 2 on the recursive one; odd_cube: the shifted edge route;
    helmholtz3d_32: the 128 x 64 complex tile.  The launches route as before (same counters on and off)."""
    P = _odd_cube(hs) if name == "odd_cube" else prepare(hs, name, rhs="randn")
    L = hs._lib.lib()
    Fs, routes = [], []
    for on in (True, False):
        L.hsk_gemm_lds_launches(1), L.hsk_gemm_lds_edge_launches(1), L.hsk_gemm_reg_launches(1)
        with env_order(hs, on):
            Fs.append(hs.factor(P["A"], P["nd"], P["nd_loc"], swlevel=0, keep_schur=True))
        routes.append((L.hsk_gemm_lds_launches(1), L.hsk_gemm_lds_edge_launches(1), L.hsk_gemm_reg_launches(1)))
    F1, F0 = Fs
    assert routes[0] == routes[1], routes
    if name != "helmholtz3d_32":
        assert routes[0][1] > 0, routes  # enveloped Float64 updates ran (gemm_op_env_lds_kernel is counted with the edge kernel)
    assert F1.nnodes == F0.nnodes
    for k in range(F1.nnodes):
        b1, b0 = F1.node_blocks(k, with_schur=True), F0.node_blocks(k, with_schur=True)
        for blk in ("LU", "Lbi", "Uib", "S", "rperm"):
            assert np.array_equal(b1[blk], b0[blk]), (k, blk, F1.node_info(k))
    x1, x0 = hs.ldiv(F1, P["b"]), hs.ldiv(F0, P["b"])
    assert np.array_equal(x1, x0)
    assert np.all(np.isfinite(x1))
    F1.free()
    F0.free()
    # the kernels' own count of the K-steps they ran, with the order on, is the host's
    Fc, dev = _factor_counted(hs, P, True)
    host = Fc.stats()["gemm_flops"]
    print(f"[env tile order] {name}: gemm_flops host {host:.17g} device {dev:.17g}")
    assert dev == host
    Fc.free()


# ---- one synthetic batch with caller-made two-block tables: the Schur tilings at the edges of the permutation -----------------------------------

ALIGNED = 4  # bit 2 of the hook's mode: Sched::aligned16, as hs_numeric runs a level


def _two_block_front(ni, nb, seed):
    """Child 1 = positions < ni1 and ni <= p < ni + nb1, child 2 the rest: two dense diagonal blocks plus a diagonal coupling int1 <-> int2
    and bnd1 <-> bnd2, strongly diagonally dominant.  The tables are written down directly (32-blocks, hs_envelope.h): a block that meets
    child 1 starts at column / row 0, a block of child 2 alone at ni1 rounded down to 32."""
    rng = np.random.default_rng(seed)
    m, ni1, nb1 = ni + nb, ni // 2 + 1, nb // 2
    p = np.arange(m)
    side = np.where(p < ni, p >= ni1, p - ni >= nb1)
    F = np.where(side[:, None] == side[None, :], rng.standard_normal((m, m)), 0.0)
    for lo, n1, n in ((0, ni1, ni), (ni, nb1, nb)):
        k = np.arange(min(n1, n - n1))
        F[lo + k, lo + n1 + k] = rng.standard_normal(k.size)
        F[lo + n1 + k, lo + k] = rng.standard_normal(k.size)
    F[p, p] += 4.0 * m
    first = []
    for lo, n, n1 in ((0, ni, ni1), (ni, nb, nb1)):
        for b0 in range(0, n, 32):
            rows = lo + np.arange(b0, min(b0 + 32, n))
            # first interior column with an entry in these rows (the pattern is symmetric: the same table serves firstL and firstU)
            cols = np.flatnonzero(np.any(F[rows, :ni] != 0, axis=0))
            first.append((cols[0] // 32) * 32 if cols.size else 1 << 30)
    first = np.asarray(first, dtype=np.int32)
    return F, np.concatenate([first, first])


def _batch(hs, Fs, nis, envs):
    L = hs._lib.lib()
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    ni = np.asarray(nis, dtype=np.int64)
    ms = np.asarray([F.shape[0] for F in Fs], dtype=np.int64)
    nb = ms - ni
    Fp = np.concatenate([np.asarray(F, dtype=np.float64).ravel(order="F") for F in Fs])
    out = dict(LF=np.zeros(int((ms * ni).sum()) + 1), UR=np.zeros(int((ni * nb).sum()) + 1), SB=np.zeros(int((nb * nb).sum()) + 1))
    rp = np.zeros(int(ni.sum()) + 1, dtype=np.int64)
    info, growth = np.zeros(len(Fs), dtype=np.int64), np.zeros(len(Fs), dtype=np.int64)
    e = np.ascontiguousarray(np.concatenate(envs), dtype=np.int32)
    hs._lib.check(L.hsk_front_batch_env_d(len(Fs), ni.ctypes.data_as(pi), nb.ctypes.data_as(pi), 2 | ALIGNED, Fp.ctypes.data_as(pd),
                                          e.ctypes.data_as(C.POINTER(C.c_int32)), out["LF"].ctypes.data_as(pd), out["UR"].ctypes.data_as(pd),
                                          out["SB"].ctypes.data_as(pd), rp.ctypes.data_as(pi), info.ctypes.data_as(pi), growth.ctypes.data_as(pi)))
    assert not info.any() and not growth.any(), (info, growth)
    out["rperm"] = rp
    return out


def test_synthetic_batch_at_the_edges_of_the_permutation(hs):
    """Schur tilings (128 x 128 tiles of nb x nb) in one level-wide launch: 21 x 21 with a ragged last tile (the grid: 441 workgroups per
    front, no multiple of 8, so the fronts sit at different XCD shifts), 20 x 20 with a ragged last tile, 9 x 9 (the smallest tiling that
    is permuted) and 3 x 3 (fewer than 8 tile rows: left alone); the last three have fewer tiles than the grid."""
    shapes = [(256, 2600), (256, 2450), (256, 1100), (256, 300)]
    assert [-(-nb // 128) for _, nb in shapes] == [21, 20, 9, 3]
    fronts = [_two_block_front(ni, nb, 200 + nb) for ni, nb in shapes]
    Fs, envs, nis = [f for f, _ in fronts], [e for _, e in fronts], [ni for ni, _ in shapes]
    L = hs._lib.lib()
    res = []
    for on in (True, False):
        L.hsk_gemm_lds_edge_launches(1)
        with env_order(hs, on):
            res.append(_batch(hs, Fs, nis, envs))
        assert L.hsk_gemm_lds_edge_launches(1) > 0  # the clipped updates ran the enveloped kernel
    for name in ("LF", "UR", "SB", "rperm"):
        assert np.array_equal(res[0][name], res[1][name]), name
    # and the Schur complement is the Schur complement: a skipped tile would keep F's own block (no comparison of on with off shows a tile
    # that both orders skip)
    k = 2  # the 9 x 9 front
    ni, nb = shapes[k]
    off = sum(n * n for _, n in shapes[:k])
    S = res[0]["SB"][off : off + nb * nb].reshape((nb, nb), order="F")
    F = Fs[k]
    Sref = F[ni:, ni:] - F[ni:, :ni] @ np.linalg.solve(F[:ni, :ni], F[:ni, ni:])
    assert np.max(np.abs(S - Sref)) <= 1e-12 * np.max(np.abs(Sref))
