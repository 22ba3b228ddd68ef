"""Time lockstep GMRES on a block (hs_gmres_block_*) against k looped single-vector solves (hs_gmres_*) of the same handle, in the same process.

    python tools/gmres_block_time.py [--summarize FILE] [--n N] [--k 1,8,32,64] [--swlevel L --tol T] [--reltol R] [--restart M] [--maxiter I] [--loop-cols C] [WORKLOAD ...]

WORKLOAD is a problems.NAMED entry (default helmholtz3d_64).  Both paths take device arrays (where = 1) on the current torch stream and are
timed with the host clock around the call (both return only after their last device read: they synchronise every iteration).  The looped
path is k calls of hs_gmres_* one after the other, each of which converts and uploads A again, as a caller of the single-vector ABI pays it.
Per k: one warm-up of each path, then N alternating pairs (block, loop); medians.  `--loop-cols C` (default 0: all k) lets the looped path
solve only the first C columns and scales its time by k / C (`loop_measured_cols` says what ran).  The right-hand sides are random vectors
with a point source every fourth column.  One JSON line per (workload, k): t_block, t_loop, their ratio, the device seconds and the other
figures of hs_gmres_block_info, per-column iteration counts of both paths, the worst column difference between them and the worst residual
of the block solve."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="timed pairs per k (after one warm-up)")
    ap.add_argument("--k", default="1,8,32,64")
    ap.add_argument("--swlevel", type=int, default=0)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--reltol", type=float, default=1e-8)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--loop-cols", type=int, default=0, help="columns the looped path really solves (0: all; else scaled to k)")
    ap.add_argument("--summarize", metavar="FILE", help="no GPU: print a table of the JSON lines of FILE and exit")
    ap.add_argument("workloads", nargs="*", default=["helmholtz3d_64"])
    args = ap.parse_args()
    if args.summarize:
        print("| workload | k | block (ms) | loop (ms) | x loop | iterations (block) | block applications | column-applications |")
        print("|---|---|---|---|---|---|---|---|")
        for line in open(args.summarize):
            if line.startswith("{"):
                d = json.loads(line)
                it = d["iters_block"]
                print(f"| {d['workload']} | {d['k']} | {d['t_block'] * 1e3:.1f} | {d['t_loop'] * 1e3:.1f} | {d['loop_over_block']:.2f} | {min(it)}-{max(it)} | "
                      f"{d['info']['prec_calls']} | {d['info']['column_applications']} |")
        return
    import torch

    import hsamd

    hs = hsamd.load()
    from hierarchicalsolvers_jl_amd.gmres import _csc_fields

    L = hs._lib.lib()
    dev = torch.device("cuda:0")
    pi, pf = hs._lib.p_i64, hs._lib.p_f64
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
        dt = np.complex128 if cplx else np.float64
        colptr, rowval, nz = _csc_fields(A, dt)
        fblk = L.hs_gmres_block_z if cplx else L.hs_gmres_block_d
        fone = L.hs_gmres_z if cplx else L.hs_gmres_d
        sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        head = (F._h, n, colptr.ctypes.data_as(pi), rowval.ctypes.data_as(pi), nz.ctypes.data_as(C.c_void_p))
        mi = args.maxiter
        for k in [int(v) for v in args.k.split(",")]:
            g = torch.Generator(device="cpu").manual_seed(k)
            Bh = torch.randn((k, n), dtype=torch.complex128 if cplx else torch.float64, generator=g)  # row r = column r, ld n
            for c in range(3, k, 4):
                Bh[c] = 0
                Bh[c, (c * 7919) % n] = 1
            dB = Bh.to(dev)
            dX, dY = torch.zeros_like(dB), torch.zeros_like(dB)
            kl = k if args.loop_cols <= 0 else min(k, args.loop_cols)
            hist_b = np.zeros((mi + 1, k), order="F")
            it_b, cv_b = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int32)
            hist_l = np.zeros(mi + 2)
            it_l, cv_l = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int32)

            def run_b():
                hs._lib.check(fblk(*head, C.c_void_p(dB.data_ptr()), n, C.c_void_p(dX.data_ptr()), n, k, 1, 0, args.reltol, 0.0, args.restart, mi,
                                   hist_b.ctypes.data_as(pf), it_b.ctypes.data_as(pi), cv_b.ctypes.data_as(C.POINTER(C.c_int)), sp))

            def run_l():
                esz = dB.element_size()
                for c in range(kl):
                    it, cv = hs._lib.i64(0), C.c_int(0)
                    hs._lib.check(fone(*head, C.c_void_p(dB.data_ptr() + c * n * esz), C.c_void_p(dY.data_ptr() + c * n * esz), 1, 0, args.reltol, 0.0,
                                       args.restart, mi, hist_l.ctypes.data_as(pf), C.byref(it), C.byref(cv), sp))
                    it_l[c], cv_l[c] = it.value, cv.value

            def timed(fn):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                return time.perf_counter() - t0

            timed(run_b), timed(run_l)  # warm-up (the first block solve also takes the work blocks of the handle)
            tb, tl, tdev = [], [], []
            for _ in range(args.n):
                tb.append(timed(run_b))
                tdev.append(hs.gmres_block_info()["seconds"])
                tl.append(timed(run_l) * k / kl)
            info = hs.gmres_block_info()
            Xh, Yh, Bn = dX.cpu().numpy(), dY.cpu().numpy(), Bh.numpy()
            diff = float(max(np.linalg.norm(Xh[j] - Yh[j]) / np.linalg.norm(Yh[j]) for j in range(kl)))
            resid = float(max(np.linalg.norm(A @ Xh[j] - Bn[j]) / np.linalg.norm(Bn[j]) for j in range(min(k, 8))))
            t_block, t_loop = float(np.median(tb)), float(np.median(tl))
            print(json.dumps(dict(
                workload=name, n=n, dtype=F.dtype.name, swlevel=args.swlevel, tol=args.tol if args.swlevel else 0.0, reltol=args.reltol, restart=args.restart,
                maxiter=mi, k=k, t_block=t_block, t_block_all=tb, t_block_device=float(np.median(tdev)), t_loop=t_loop, t_loop_all=tl, loop_measured_cols=kl,
                loop_over_block=t_loop / t_block, iters_block=[int(v) for v in it_b], converged_block=int(cv_b.sum()), iters_loop=[int(v) for v in it_l[:kl]],
                converged_loop=int(cv_l[:kl].sum()), info=info, worst_col_block_vs_loop=diff, worst_residual_block=resid)), flush=True)
            del dB, dX, dY
        F.free()


if __name__ == "__main__":
    main()
