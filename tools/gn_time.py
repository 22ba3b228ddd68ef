"""Time the tangent-linear solve, the Gauss-Newton Hessian-vector product and its diagonal (hs_tangent_dev_*, hs_gn_hessvec_dev_*,
hs_gn_diag_dev_*) on device arrays, the block solve alone, and the host composition the calls replace, in one process.

    python tools/gn_time.py [--n 5] [--k 32] [--rows 64] [--no-host] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_64 and helmholtz3d_64:swlevel=4,tol=1e-4).  k dense
random sources, `rows` random distinct receiver rows, a random direction on the pattern.  One JSON line per workload and measurement:

  device  the library's event pairs (hs_gn_info, hs_ldiv_block_info), medians of N calls after one warm-up: hs_gn_hessvec_dev_* without and
          with the fields supplied, hs_tangent_dev_*, hs_gn_diag_dev_*, one hs_ldiv_block_dev_t_* of the same k columns, the split of the
          product with fields (tangent solve, adjoint solve, products) and its ratio to two block solves
  host    what a user composes without the calls, from host arrays: hs.ldiv_block_t, a SciPy product with E, hs.ldiv_block_t, hs.sensitivity
          (which solves for the fields again), wall clock, median of N"""
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
from sens_time import rand


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="timed rounds (after one warm-up)")
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_64", "helmholtz3d_64:swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    hs = hsamd.load()
    E = hs._lib
    L = E.lib()
    dev = torch.device("cuda:0")
    for spec in args.workloads:
        name, kw = parse(spec)
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        A.sort_indices()
        nd = hs.permuted(nd, hs.invperm(perm))
        F = hs.factor(A, nd, nd_loc, **kw)
        n, k, nr = A.shape[0], args.k, args.rows
        cplx = F.dtype.kind == "c"
        sfx = "_z" if cplx else "_d"
        base = dict(workload=spec, n=n, nnz=int(A.nnz), dtype=F.dtype.name, k=k, rows=nr, chunk_cols=hs.solver._block_cols())
        B, Ev = rand(n, k, cplx, 1), rand(A.nnz, 1, cplx, 2)[:, 0].copy()
        rows = np.random.default_rng(3).choice(n, size=nr, replace=False)
        rows1 = np.ascontiguousarray(rows, dtype=np.int64) + 1
        pr = rows1.ctypes.data_as(E.p_i64)

        s = torch.cuda.current_stream(dev)
        up = lambda M: torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)  # row j = column j of the column-major block
        dB, dE = up(B), torch.from_numpy(Ev).to(dev)
        dX, dD, dC = torch.zeros_like(dB), torch.zeros_like(dB), torch.zeros_like(dB)
        dHE = torch.zeros(A.nnz, dtype=dB.dtype, device=dev)
        dHd = torch.zeros(A.nnz, dtype=torch.float64, device=dev)
        bB = E.hs_block_arg(dB.data_ptr(), n, None, None, None)
        hv, tg, dg, bs = (getattr(L, f + sfx) for f in ("hs_gn_hessvec_dev", "hs_tangent_dev", "hs_gn_diag_dev", "hs_ldiv_block_dev_t"))
        calls = {
            "hessvec": lambda: hv(F._h, 0, n, k, C.byref(bB), None, 0, dE.data_ptr(), 0, 0, pr, nr, dHE.data_ptr(), None, nr, dX.data_ptr(), n, s.cuda_stream),
            "hessvec_with_fields": lambda: hv(F._h, 0, n, k, None, dX.data_ptr(), n, dE.data_ptr(), 0, 0, pr, nr, dHE.data_ptr(), None, nr, None, n, s.cuda_stream),
            "tangent": lambda: tg(F._h, 0, n, k, C.byref(bB), None, 0, dE.data_ptr(), 0, 0, None, 0, dD.data_ptr(), n, None, n, s.cuda_stream),
            "diag": lambda: dg(F._h, 0, n, k, C.byref(bB), None, 0, pr, nr, 0, 0, dHd.data_ptr(), None, None, s.cuda_stream),
            "block_solve": lambda: bs(F._h, 0, dC.data_ptr(), n, dB.data_ptr(), n, n, k, s.cuda_stream),
        }
        res, split = {}, {}
        for what, call in calls.items():
            rounds = []
            for it in range(args.n + 1):
                E.check(call())
                if it > 0:
                    rounds.append(hs.ldiv_block_info(F) if what == "block_solve" else hs.gn_info(F))
            res[what] = float(np.median([r["seconds"] for r in rounds]))
            if what != "block_solve":
                split[what] = {key: float(np.median([r[key] for r in rounds])) for key in ("seconds_forward", "seconds_tangent", "seconds_adjoint", "seconds_products")}
                split[what].update(groups=rounds[-1]["groups"], block_solves=rounds[-1]["block_solves"], workspace_bytes=rounds[-1]["workspace_bytes"])
        print(json.dumps(dict(base, what="device", seconds=res, split=split, hessvec_with_fields_over_two_block_solves=res["hessvec_with_fields"] / (2 * res["block_solve"]),
                              hessvec_over_three_block_solves=res["hessvec"] / (3 * res["block_solve"]))), flush=True)
        HE_dev = dHE.cpu().numpy()
        del dB, dX, dD, dC, dHE, dHd

        if not args.no_host:
            Em = sp.csc_matrix((Ev, A.indices, A.indptr), shape=A.shape).tocsr()
            hs.ldiv_block_t(F, B[:, :1])
            walls = []
            for it in range(args.n):
                t0 = time.perf_counter()
                X = hs.ldiv_block_t(F, B)
                D = hs.ldiv_block_t(F, np.asfortranarray(-(Em @ X)))
                t1 = time.perf_counter()
                W = np.zeros_like(D)
                W[rows] = D[rows]
                G = hs.sensitivity(F, B, W)
                t2 = time.perf_counter()
                walls.append((t1 - t0, t2 - t1, t2 - t0))
            med = [float(np.median([w[i] for w in walls])) for i in range(3)]
            scale = float(np.abs(G).max())
            print(json.dumps(dict(base, what="host", wall_tangent=med[0], wall_sensitivity=med[1], wall_hessvec=med[2],
                                  max_diff_to_device=float(np.abs(G - HE_dev).max()) / scale)), flush=True)
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
