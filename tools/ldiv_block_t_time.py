"""Time the transposed / adjoint block solve (hs_ldiv_block_dev_t_*) against the forward block solve (hs_ldiv_block_dev_*) and the looped
single-vector transposed solve (hs_ldiv_dev_t_*) of the same handle, in one process.

    python tools/ldiv_block_t_time.py [--n N] [--k 32] [--loop-cols 4] [--once] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_128 and helmholtz3d_64:swlevel=4,tol=1e-4).  All
paths run on device arrays; the block solves are timed by the library's own event pair (hs_ldiv_block_info: device seconds), the looped
solve by a torch event pair on the same stream.  One warm-up of each path, then N rounds in which the paths alternate; medians.  The
looped time is measured with --loop-cols columns and scaled to k (it is k single-vector solves by construction).  One JSON line per
(workload, trans): times, the ratio to the forward block solve of the same run, the executed- and useful-flop rates on the matrix pipe, the
worst column against the looped path.  The looking order of the triangular sweeps is HS_LDIV_BLOCK_T_LOOK of the environment (read once
per process).  --once: one transposed block solve per workload and nothing else (for a kernel trace)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hsamd
from ldiv_t_time import parse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="timed rounds (after one warm-up)")
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--loop-cols", type=int, default=4, help="columns the looped path really solves (scaled to k)")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_128", "helmholtz3d_64:swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    hs = hsamd.load()
    L = hs._lib.lib()
    dev = torch.device("cuda:0")
    look = "left" if (os.environ.get("HS_LDIV_BLOCK_T_LOOK", "") or "r")[0] in "lL" else "right"
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
        fblk_t = L.hs_ldiv_block_dev_t_z if cplx else L.hs_ldiv_block_dev_t_d
        floop_t = L.hs_ldiv_dev_t_z if cplx else L.hs_ldiv_dev_t_d
        s = torch.cuda.current_stream(dev)
        sp = C.c_void_p(s.cuda_stream)
        dB = torch.randn((k, n), dtype=torch.complex128 if cplx else torch.float64, generator=torch.Generator(device="cpu").manual_seed(k)).to(dev)
        dX, dY = torch.empty_like(dB), torch.empty_like(dB)
        p = lambda t: C.c_void_p(t.data_ptr())

        def block(trans):
            fn = fblk_t if trans else fblk
            hs._lib.check(fn(F._h, trans, p(dX), n, p(dB), n, n, k, sp))
            return hs.ldiv_block_info(F)

        if args.once:
            block(1)
            print(json.dumps(dict(workload=spec, k=k, once=True, seconds=hs.ldiv_block_info(F)["seconds"])), flush=True)
            F.free()
            continue
        kl = min(k, args.loop_cols)

        def loop(trans):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            hs._lib.check(floop_t(F._h, trans, p(dY), n, p(dB), n, n, kl, sp))
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 * k / kl

        transes = (1, 2) if cplx else (1,)
        block(0)
        for t in transes:
            block(t), loop(t)
        tf, tb, tl = [], {t: [] for t in transes}, {t: [] for t in transes}
        info = {}
        for _ in range(args.n):
            tf.append(block(0)["seconds"])
            for t in transes:
                info[t] = block(t)
                tb[t].append(info[t]["seconds"])
                tl[t].append(loop(t))
        t_fwd = float(np.median(tf))
        for t in transes:
            block(t), loop(t)
            Xh, Yh = dX[:kl].cpu().numpy(), dY[:kl].cpu().numpy()
            diff = float(max(np.linalg.norm(Xh[j] - Yh[j]) / np.linalg.norm(Yh[j]) for j in range(kl)))
            t_blk, t_loop = float(np.median(tb[t])), float(np.median(tl[t]))
            print(json.dumps(dict(
                workload=spec, n=n, dtype=F.dtype.name, k=k, trans=t, look=look, chunk_cols=int(os.environ.get("HS_LDIV_BLOCK_COLS", "32") or 32),
                t_block_t=t_blk, t_block_t_all=tb[t], t_block_fwd=t_fwd, t_block_fwd_all=tf, t_over_fwd=t_blk / t_fwd,
                t_loop_t=t_loop, loop_measured_cols=kl, loop_over_block=t_loop / t_blk,
                factor_TBps=info[t]["factor_bytes"] / t_blk / 1e12, pipe_tflops_executed=info[t]["flops_executed"] / t_blk / 1e12,
                pipe_tflops_useful=info[t]["flops_useful"] / t_blk / 1e12, worst_col_block_vs_loop=diff)), flush=True)
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
