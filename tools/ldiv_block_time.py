"""Time the block solve (hs_ldiv_block_*) against k looped single-vector solves of the same handle, in the same process.

    python tools/ldiv_block_time.py [--n N] [--k 1,4,8,16,32,64,128] [--swlevel L --tol T] [WORKLOAD ...]

WORKLOAD is a problems.NAMED entry (default poisson3d_64).  Both paths run on device arrays (hs_ldiv_block_dev_* / hs_ldiv_dev_*), timed with
a HIP event pair around the call on the handle's own side of the device (torch events on one stream), so no host transfer is in the
numbers.  Per k: one warm-up of each path, then N alternating pairs (block, loop); medians.  The looped time for k > 8 is measured with 8
columns and scaled by k / 8 (it is k single-vector solves by construction; `loop_measured_cols` says what ran).  One JSON line per (workload,
k): t_block, t_loop, their ratio, t_block over the single-vector solve, factor bytes per second and matrix-pipe TF/s (executed and useful)
from hs_ldiv_block_info, the chunk width, the worst column's difference between the two paths, the residual of the block solve's first
column.  The chunk width is HS_LDIV_BLOCK_COLS of the environment (read once per process)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hsamd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="timed pairs per k (after one warm-up)")
    ap.add_argument("--k", default="1,4,8,16,32,64,128")
    ap.add_argument("--swlevel", type=int, default=0)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--loop-cols", type=int, default=8, help="columns the looped path really solves (scaled to k beyond that)")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_64"])
    args = ap.parse_args()
    hs = hsamd.load()
    L = hs._lib.lib()
    dev = torch.device("cuda:0")
    for name in args.workloads:
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        nd = hs.permuted(nd, hs.invperm(perm))
        fopts = dict(swlevel=0) if args.swlevel == 0 else dict(swlevel=args.swlevel, swsize=8, atol=args.tol, rtol=args.tol)
        F = hs.factor(A, nd, nd_loc, **fopts)
        n = A.shape[0]
        cplx = F.dtype.kind == "c"
        fblk = L.hs_ldiv_block_dev_z if cplx else L.hs_ldiv_block_dev_d
        floop = L.hs_ldiv_dev_z if cplx else L.hs_ldiv_dev_d
        s = torch.cuda.current_stream(dev)
        sp = C.c_void_p(s.cuda_stream)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        d1 = torch.randn((1, n), dtype=torch.complex128 if cplx else torch.float64, generator=torch.Generator(device="cpu").manual_seed(0)).to(dev)
        y1 = torch.empty_like(d1)
        run_1 = lambda: hs._lib.check(floop(F._h, C.c_void_p(y1.data_ptr()), n, C.c_void_p(d1.data_ptr()), n, n, 1, sp))
        timed(run_1)
        t_single = float(np.median([timed(run_1) for _ in range(args.n)]))  # the yardstick: one single-vector solve of this handle
        for k in [int(v) for v in args.k.split(",")]:
            g = torch.Generator(device="cpu").manual_seed(k)
            dB = torch.randn((k, n), dtype=torch.complex128 if cplx else torch.float64, generator=g).to(dev)  # row r = column r, ld n
            dX, dY = torch.empty_like(dB), torch.empty_like(dB)
            kl = min(k, args.loop_cols)
            run_b = lambda: hs._lib.check(fblk(F._h, 0, C.c_void_p(dX.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, k, sp))
            run_l = lambda: hs._lib.check(floop(F._h, C.c_void_p(dY.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, kl, sp))
            timed(run_b), timed(run_l)  # warm-up (the first block solve also takes the work blocks)
            tb, tl, tinfo = [], [], []
            for _ in range(args.n):
                tb.append(timed(run_b))
                tinfo.append(hs.ldiv_block_info(F)["seconds"])
                tl.append(timed(run_l) * k / kl)
            info = hs.ldiv_block_info(F)
            Xh, Yh, Bh = dX[:kl].cpu().numpy(), dY[:kl].cpu().numpy(), dB[:kl].cpu().numpy()
            diff = float(max(np.linalg.norm(Xh[j] - Yh[j]) / np.linalg.norm(Yh[j]) for j in range(kl)))
            resid = float(np.linalg.norm(A @ Xh[0] - Bh[0]) / np.linalg.norm(Bh[0]))  # of the block solve's first column, on the host
            t_block, t_loop = float(np.median(tb)), float(np.median(tl))
            print(json.dumps(dict(
                workload=name, n=n, dtype=F.dtype.name, swlevel=args.swlevel, tol=args.tol if args.swlevel else 0.0, k=k,
                chunk_cols=int(os.environ.get("HS_LDIV_BLOCK_COLS", "32") or 32), chunks=info["chunks"],
                t_block=t_block, t_block_all=tb, t_block_info=float(np.median(tinfo)), t_loop=t_loop, t_loop_all=tl, loop_measured_cols=kl,
                loop_over_block=t_loop / t_block, t_single=t_single, block_over_single=t_block / t_single,
                model_multiple=1.0 + k / 32.0,
                factor_bytes=info["factor_bytes"], factor_TBps=info["factor_bytes"] / t_block / 1e12,
                pipe_tflops_executed=info["flops_executed"] / t_block / 1e12, pipe_tflops_useful=info["flops_useful"] / t_block / 1e12,
                workspace_bytes=info["workspace_bytes"], worst_col_block_vs_loop=diff, residual_col0=resid)), flush=True)
            del dB, dX, dY
        F.free()


if __name__ == "__main__":
    main()
