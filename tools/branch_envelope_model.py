"""usage (no GPU): python tools/branch_envelope_model.py [WORKLOAD] -- flops of the branch fronts eliminated inside their block envelope
(csrc/hs_envelope.h: hs_branch_envelope) against the dense count, per tree level, on the tree bench.py prepares (default poisson3d_128).

Every entry C[r, c] of a front takes the products k in [max(firstL[block of r], firstU[block of c]), min(r, c, ni)).  The tables are the
library's own (hsk_branch_envelope, host only).  Two counts: `env 32` clips per 32-block pair, which is what the tables allow; `env T` clips
per tile of T x T positions (T = 128, or the environment variable T), a tile starting at the smallest start of its 32-blocks -- what a GEMM
tile of that size can skip (an estimate: the real tiles are aligned to their launch, not to the front).  Leaves are not counted.

A second table takes the level-wide Schur launch of every branch level -- the longest plain update of a level -- tile by tile: the K-steps
each of the 8 XCDs runs under the dense tile order, the balanced one and the K-sorted one (GemmOp::order, HS_ENV_ORDER; the block id -> tile map is the
library's own, hsk_env_tile_order), as heaviest XCD over mean.  The other plain updates of a level (panel and block-column updates inside
the interior part) are not modelled: they follow the blocked LU schedule, which this tool does not restate."""
import ctypes as C
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hsamd  # noqa: E402

G = 32
NONE = 1 << 30


def tables(L, colptr, rowval, n, idx, ni, ni1, nb1):
    m = len(idx)
    nblk = (ni + G - 1) // G + (m - ni + G - 1) // G
    fL = np.empty(nblk, dtype=np.int32)
    fU = np.empty(nblk, dtype=np.int32)
    fidx = np.ascontiguousarray(idx, dtype=np.int32)
    p64, p32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    rc = L.hsk_branch_envelope(n, colptr.ctypes.data_as(p64), rowval.ctypes.data_as(p64), fidx.ctypes.data_as(p32), ni, m - ni, ni1, nb1,
                               fL.ctypes.data_as(p32), fU.ctypes.data_as(p32))
    assert rc == 0
    return fL.astype(np.int64), fU.astype(np.int64)


def coarsen(f, nbi, t):
    """the start a tile of t 32-blocks sees: the smallest of its blocks (interior and boundary blocks grouped separately)"""
    out = f.copy()
    for lo, hi in ((0, nbi), (nbi, len(f))):
        for b in range(lo, hi, t):
            out[b : min(b + t, hi)] = f[b : min(b + t, hi)].min()
    return out


def front_macs(ni, nb, fL, fU):
    """multiply-adds of one front: sum over (r, c) of max(0, min(r, c, ni) - max(firstL[r], firstU[c])), by 32-block pairs; None: dense"""
    m = ni + nb
    nbi = (ni + G - 1) // G
    start = np.concatenate([np.arange(nbi) * G, ni + np.arange((nb + G - 1) // G) * G])
    size = np.minimum(np.concatenate([np.full(nbi, ni), np.full(len(start) - nbi, m)]) - start, G)
    pos = np.concatenate([np.arange(nbi), np.full(len(start) - nbi, nbi)])  # elimination order of the blocks: the boundary comes last, all alike
    # sum over the block's positions of min(p, ni), and the value a block's positions have at least
    rs = np.where(start < ni, size * start + size * (size - 1) // 2, size * ni).astype(np.float64)
    ustart = np.minimum(start, ni)
    if fL is None:
        lo = np.zeros((len(start), len(start)))
    else:
        lo = np.maximum(fL[:, None], fU[None, :]).astype(np.float64)
    sz = size.astype(np.float64)
    upper_is_row = (pos[:, None] < pos[None, :]) | ((pos[:, None] == nbi) & (pos[None, :] == nbi))  # min(r, c, ni) is decided by the row
    upper_is_col = pos[:, None] > pos[None, :]
    a = np.where(lo <= ustart[:, None], (rs[:, None] - lo * sz[:, None]) * sz[None, :], 0.0)
    b = np.where(lo <= ustart[None, :], (rs[None, :] - lo * sz[None, :]) * sz[:, None], 0.0)
    macs = np.where(upper_is_row, a, 0.0).sum() + np.where(upper_is_col, b, 0.0).sum()
    # interior diagonal blocks: sum of min(r, c) - lo, lo <= the block's start
    d = np.arange(nbi)
    s = size[d].astype(np.float64)
    mins = s * s * start[d] + (s - 1) * s * (2 * s - 1) / 6.0
    macs += (mins - np.diagonal(lo)[:nbi] * s * s).sum()
    return macs


XCDS = 8
BM = 128  # the Float64 tile (TileCfg<double>: 128 x 128, BK = 16)
BK = 16


def xcd_remap_shift(bid, nwg, shift):
    """csrc/kernels_gemm.hip restated: block `bid` of a front sits on XCD (bid + shift) & 7; XCD x owns a contiguous chunk of tile ids"""
    x = (bid + shift) & 7
    first = (np.arange(XCDS) - shift) & 7
    cnt = np.where(first < nwg, (nwg - first + 7) >> 3, 0)
    base = np.concatenate([[0], np.cumsum(cnt)])[x]
    return base + ((bid - ((x - shift) & 7)) >> 3)


def tile_of_id(L, tiles, order):
    """tile id t -> (tm, tn) under the dense (0) or the balanced (1) order, from the library's own hsk_env_tile_order (which answers per
    block id of an unshifted front: undo its remap)"""
    nt = tiles * tiles
    tm, tn = np.empty(nt, dtype=np.int32), np.empty(nt, dtype=np.int32)
    p32 = C.POINTER(C.c_int32)
    assert L.hsk_env_tile_order(tiles, tiles, order, tm.ctypes.data_as(p32), tn.ctypes.data_as(p32)) == 0
    t = xcd_remap_shift(np.arange(nt), nt, 0)
    om, on = np.empty(nt, dtype=np.int64), np.empty(nt, dtype=np.int64)
    om[t], on[t] = tm, tn
    return om, on


MIN_TILES = int(os.environ.get("HS_ENV_ORDER_MIN_TILES", "2048"))  # fronts with fewer tiles keep the balanced order under order 2 (kernels_gemm.hip)


def schur_xcd_load(L, fronts, order):
    """K-steps every XCD runs in the level-wide Schur launch SB -= LF[ni.., 0:ni) * UR of a batch (one workgroup per tile, grid.x = the tiles
    of the largest front; the hardware deals workgroups to the XCDs round-robin over blockIdx.x + gridDim.x * blockIdx.y).  The fronts are
    taken in tree order, which need not be the batch order of the library: the shifts of the single fronts are an estimate.  order 2: the
    K-sorted order, from the library's own hsk_env_phase_order.  Also returns the share of the tiles that sit among the 64 consecutive
    block ids of their XCD (the workgroups it holds at a time) with a single K start."""
    gx = max(-(-nb // BM) ** 2 for _, nb, _, _ in fronts)
    load = np.zeros(XCDS)
    cache = {}
    single = total = 0
    p32 = C.POINTER(C.c_int32)
    for y, (ni, nb, fL, fU) in enumerate(fronts):
        tiles = -(-nb // BM)
        if tiles == 0:
            continue
        nbi = (ni + G - 1) // G
        pad = np.full(tiles * (BM // G) - (len(fL) - nbi), NONE)
        rmin = np.concatenate([fL[nbi:], pad]).reshape(tiles, BM // G).min(axis=1)
        cmin = np.concatenate([fU[nbi:], pad]).reshape(tiles, BM // G).min(axis=1)
        steps = -(-np.maximum(ni - np.maximum(rmin[:, None], cmin[None, :]), 0) // BK)  # [tm, tn]
        nt = tiles * tiles
        shift = (gx * y) & 7 if gx & 7 else 0
        bid = np.arange(nt)
        if order == 2 and nt >= MIN_TILES and tiles <= 512:
            kr = np.ascontiguousarray(np.clip(rmin, 0, ni), dtype=np.int32)
            kc = np.ascontiguousarray(np.clip(cmin, 0, ni), dtype=np.int32)
            tm, tn = np.empty(nt, dtype=np.int32), np.empty(nt, dtype=np.int32)
            assert L.hsk_env_phase_order(tiles, tiles, kr.ctypes.data_as(p32), kc.ctypes.data_as(p32), shift, tm.ctypes.data_as(p32),
                                         tn.ctypes.data_as(p32), None) == 0
        else:
            o = min(order, 1)
            if (tiles, o) not in cache:
                cache[(tiles, o)] = tile_of_id(L, tiles, o)
            om, on = cache[(tiles, o)]
            t = xcd_remap_shift(bid, nt, shift)
            tm, tn = om[t], on[t]
        st = steps[tm, tn]
        load += np.bincount((bid + shift) & 7, weights=st.astype(np.float64), minlength=XCDS)
        for x in range(XCDS):
            mine = st[((bid + shift) & 7) == x]
            for lo in range(0, mine.size, 64):
                c = mine[lo : lo + 64]
                single += c.size if np.all(c == c[0]) else 0
        total += nt
    return load, single / max(total, 1)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "poisson3d_128"
    T = int(os.environ.get("T", "128")) // G
    hs = hsamd.load()
    L = hs._lib.lib()
    t0 = time.time()
    A, b, nd = hs.problems.make_problem(name, rhs="randn")
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    Ap = sp.csc_matrix(A[perm - 1][:, perm - 1])
    nd = hs.permuted(nd, hs.invperm(perm))
    n = Ap.shape[0]
    colptr = np.ascontiguousarray(Ap.indptr, dtype=np.int64) + 1
    rowval = np.ascontiguousarray(Ap.indices, dtype=np.int64) + 1
    lev = {}
    stack = [(nd, 1)]
    while stack:
        x, lv = stack.pop()
        if x.left is None and x.right is None:
            continue
        stack += [(c, lv + 1) for c in (x.left, x.right) if c is not None]
        it, bd = np.asarray(x.int) - 1, np.asarray(x.bnd) - 1
        ni, nb = len(it), len(bd)
        if ni == 0:
            continue
        lb = np.asarray(x.left.bnd) - 1 if x.left is not None else np.zeros(0, np.int64)
        ni1, nb1 = int(np.isin(it, lb).sum()), int(np.isin(bd, lb).sum())
        fL, fU = tables(L, colptr, rowval, n, np.concatenate([it, bd]), ni, ni1, nb1)
        nbi = (ni + G - 1) // G
        r = lev.setdefault(lv, dict(fronts=0, ni=0, nb=0, dense=0.0, e32=0.0, eT=0.0, fr=[]))
        r["fronts"] += 1
        r["fr"].append((ni, nb, fL, fU))
        r["ni"], r["nb"] = max(r["ni"], ni), max(r["nb"], nb)
        r["dense"] += 2.0 * front_macs(ni, nb, None, None)
        r["e32"] += 2.0 * front_macs(ni, nb, fL, fU)
        r["eT"] += 2.0 * front_macs(ni, nb, coarsen(fL, nbi, T), coarsen(fU, nbi, T))
    print("# %s, n = %d: flops of the branch fronts, dense and inside the block envelope (%.1f s)" % (name, n, time.time() - t0))
    print("| level | fronts | max (ni, nb) | dense | env 32 | ratio | env %d | ratio |" % (T * G))
    print("|---|---|---|---|---|---|---|---|")
    tot = np.zeros(3)
    for lv in sorted(lev):
        r = lev[lv]
        tot += [r["dense"], r["e32"], r["eT"]]
        print("| %d | %d | %d, %d | %.4g | %.4g | %.3f | %.4g | %.3f |" % (lv, r["fronts"], r["ni"], r["nb"], r["dense"], r["e32"], r["e32"] / r["dense"],
                                                                     r["eT"], r["eT"] / r["dense"]))
    print("| all | | | %.4g | %.4g | %.3f | %.4g | %.3f |" % (tot[0], tot[1], tot[1] / tot[0], tot[2], tot[2] / tot[0]))
    print()
    print("# level-wide Schur launches: K-steps of the heaviest XCD over the mean, dense tile order (HS_ENV_ORDER=0), balanced order (1) and")
    print("# K-sorted order (2; fronts below %d tiles keep order 1); K-steps run / dense = the share of the dense launch's K-steps that the" % MIN_TILES)
    print("# clipped tiles run; single start = share of the tiles whose 64 co-resident block ids of their XCD have one K start, orders 0 / 1 / 2")
    print("| level | fronts | tile rows (largest front) | K-steps run / dense | heaviest / mean, order 0 | order 1 | order 2 | single start 0 / 1 / 2 |")
    print("|---|---|---|---|---|---|---|---|")
    for lv in sorted(lev):
        fr = [f for f in lev[lv]["fr"] if f[1] > 0]
        if not fr:
            continue
        (l0, s0), (l1, s1), (l2, s2) = (schur_xcd_load(L, fr, o) for o in (0, 1, 2))
        dense = sum((-(-nb // BM)) ** 2 * -(-ni // BK) for ni, nb, _, _ in fr)
        assert l0.sum() == l1.sum() == l2.sum()
        print("| %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.2f / %.2f / %.2f |" % (lv, len(fr), max(-(-nb // BM) for _, nb, _, _ in fr), l0.sum() / dense,
                                                                            l0.max() / l0.mean(), l1.max() / l1.mean(), l2.max() / l2.mean(), s0, s1, s2))


if __name__ == "__main__":
    main()
