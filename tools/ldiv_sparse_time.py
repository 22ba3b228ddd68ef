"""Time the sparse-right-hand-side solve (hs_ldiv_sparse_dev_*) against the block solve of the expanded block (hs_ldiv_block_dev_*) on the
same handle, in one process.

    python tools/ldiv_sparse_time.py [--n 5] [--k 32] [--host] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_128 and helmholtz3d_64:swlevel=4,tol=1e-4).  k unit
sources that are (a) all inside one leaf front, (b) spread uniformly over the unknowns; wanted rows that are (i) all, (ii) one grid plane,
(iii) k points spread uniformly.  Device arrays; both paths are timed by the library's own event pair (hs_ldiv_sparse_info /
hs_ldiv_block_info: device seconds around the launches) and by the wall clock around the call (the sparse call builds its closure and index
lists on the host and waits for its stream; the block call is asynchronous, so its wall time includes a stream synchronisation).  One
warm-up of each path, then N rounds in which the two alternate; medians.  One JSON line per (workload, sources, rows): times, the visit
counts, the model bytes, and whether the wanted rows carry the bits of the block solve.  --host adds the host-array entry points
(hs_ldiv_sparse_* against hs_ldiv_block_*) for case (a)(iii), wall clock."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import hsamd
from ldiv_t_time import parse


def one_leaf(nd):
    """0-based interior rows of the first leaf of the (permuted) elimination tree."""
    x = nd
    while x.left is not None:
        x = x.left
    return np.asarray(x.int, dtype=np.int64) - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="timed rounds (after one warm-up)")
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_128", "helmholtz3d_64:swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    hs = hsamd.load()
    L = hs._lib.lib()
    E = hs._lib
    dev = torch.device("cuda:0")
    for spec in args.workloads:
        name, kw = parse(spec)
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        nd = hs.permuted(nd, hs.invperm(perm))
        F = hs.factor(A, nd, nd_loc, **kw)
        n, k = A.shape[0], args.k
        cplx = F.dtype.kind == "c"
        fblk = L.hs_ldiv_block_dev_z if cplx else L.hs_ldiv_block_dev_d
        fsp = L.hs_ldiv_sparse_dev_z if cplx else L.hs_ldiv_sparse_dev_d
        s = torch.cuda.current_stream(dev)
        st = C.c_void_p(s.cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())
        rng = np.random.default_rng(k)
        leaf = one_leaf(nd)
        side = round(n ** (1.0 / 3.0))
        plane = np.flatnonzero((perm - 1) // (side * side) == side // 2) if side**3 == n else np.arange(n)[:: max(1, round(n ** (1.0 / 3.0)))]
        srcs = {"one_leaf": rng.choice(leaf, size=min(k, len(leaf)), replace=False), "uniform": np.linspace(0, n - 1, k).astype(np.int64)}
        rowsets = {"all": None, "plane": plane.astype(np.int64), "points": np.linspace(n // 7, n - 1 - n // 9, k).astype(np.int64)}
        for sname, src in srcs.items():
            kk = len(src)
            B = sp.csc_matrix((np.ones(kk, dtype=F.dtype), src, np.arange(kk + 1)), shape=(n, kk))
            cp = np.ascontiguousarray(B.indptr, dtype=np.int64) + 1
            rv = np.ascontiguousarray(B.indices, dtype=np.int64) + 1
            dv = torch.from_numpy(np.ascontiguousarray(B.data)).to(dev)
            dB = torch.zeros((kk, n), dtype=dv.dtype, device=dev)  # row j = column j of the expanded block
            dB[torch.arange(kk), torch.from_numpy(src)] = 1
            dC = torch.empty_like(dB)

            def dense():
                t0 = time.perf_counter()
                E.check(fblk(F._h, 0, p(dC), n, p(dB), n, n, kk, st))
                s.synchronize()
                return time.perf_counter() - t0, hs.ldiv_block_info(F)

            for rname, rows in rowsets.items():
                nout = n if rows is None else len(rows)
                r1 = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64) + 1
                dX = torch.empty((kk, nout), dtype=dv.dtype, device=dev)

                def sparse():
                    t0 = time.perf_counter()
                    E.check(fsp(F._h, 0, n, kk, cp.ctypes.data_as(E.p_i64), rv.ctypes.data_as(E.p_i64), p(dv), None if r1 is None else r1.ctypes.data_as(E.p_i64),
                                0 if r1 is None else len(r1), p(dX), nout, st))
                    return time.perf_counter() - t0, hs.ldiv_sparse_info(F)

                dense(), sparse()
                td, ts, wd, ws = [], [], [], []
                for _ in range(args.n):
                    w, i = dense()
                    td.append(i["seconds"]), wd.append(w)
                    w, info = sparse()
                    ts.append(info["seconds"]), ws.append(w)
                same = bool(torch.equal(dX, dC if rows is None else dC[:, torch.from_numpy(rows).to(dev)]))
                t_d, t_s = float(np.median(td)), float(np.median(ts))
                print(json.dumps(dict(
                    workload=spec, n=n, dtype=F.dtype.name, k=kk, sources=sname, rows=rname, nrows=nout, chunk_cols=hs.solver._block_cols(),
                    t_sparse=t_s, t_sparse_all=ts, t_dense=t_d, t_dense_all=td, dense_over_sparse=t_d / t_s, wall_sparse=float(np.median(ws)),
                    wall_dense=float(np.median(wd)), visits_forward=info["visits_forward"], visits_backward=info["visits_backward"],
                    visits_dense=info["visits_dense"], model_bytes=info["factor_bytes"], dense_model_bytes=i["factor_bytes"],
                    model_TBps=info["factor_bytes"] / t_s / 1e12, same_bits=same)), flush=True)
            if args.host and sname == "one_leaf":
                rows = rowsets["points"]
                Bh = np.asfortranarray(B.toarray())
                hs.ldiv_sparse(F, B, rows), hs.ldiv_block(F, Bh)
                wh, wb = [], []
                for _ in range(args.n):
                    t0 = time.perf_counter()
                    hs.ldiv_block(F, Bh)
                    wb.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    hs.ldiv_sparse(F, B, rows)
                    wh.append(time.perf_counter() - t0)
                print(json.dumps(dict(workload=spec, host=True, sources=sname, rows="points", wall_sparse=float(np.median(wh)), wall_dense=float(np.median(wb)),
                                      values_moved=hs.ldiv_sparse_info(F)["values_moved"], dense_values_moved=2 * n * kk)), flush=True)
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
