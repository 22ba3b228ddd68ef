"""Time hs_selinv (diag + pattern) and hs_logabsdet against the factorization of the same handle.

    python tools/selinv_time.py [--n N] [--budget BYTES] [WORKLOAD ...]

WORKLOAD is a problems.NAMED entry (default: poisson3d_64), factored exactly (swlevel = 0).  Per workload: 1 warm-up + N timed calls of each
function; hs_selinv's seconds are the HIP-event time the library measures around its own launches (hs_selinv_info), next to the wall time of
the call (host-side list building of the first call excluded by the warm-up); hs_logabsdet is wall time of the blocking call.  One JSON
line per workload: seconds (median and all), hs_selinv_info's flops, TF/s, peak scratch, batches, and the factorization's t_total and
flops_factor (hs_stats) of the same handle, so the ratio selinv / factor can be read off."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import hsamd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3, help="timed calls per function (after one warm-up)")
    ap.add_argument("--budget", type=int, default=0, help="hs_selinv budget_bytes (0: derived from the free device memory)")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_64"])
    args = ap.parse_args()
    hs = hsamd.load()
    for name in args.workloads:
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        nd = hs.permuted(nd, hs.invperm(perm))
        F = hs.factor(A, nd, nd_loc, swlevel=0)
        st = F.stats()
        sel_dev, sel_wall, det_wall, info = [], [], [], None
        for it in range(args.n + 1):
            t0 = time.perf_counter()
            d, Z = hs.selinv(F, budget=args.budget)
            t1 = time.perf_counter()
            info = hs.selinv_info(F)
            t2 = time.perf_counter()
            la, sign = hs.logabsdet(F)
            t3 = time.perf_counter()
            if it:  # the first call is the warm-up (it also builds the per-front entry lists of A's pattern)
                sel_dev.append(info["seconds"])
                sel_wall.append(t1 - t0)
                det_wall.append(t3 - t2)
        # a cheap end-to-end check of what was timed: trace(A^-1 A) = n from the pattern values, diag against a solve with e_0
        e0 = np.zeros(A.shape[0])
        e0[0] = 1.0
        chk_tr = abs((hs.selinv(hs.transpose(F), diag=False)[1].data * A.data).sum() / A.shape[0] - 1.0)
        chk_d0 = abs(F.solve(e0)[0] - d[0]) / abs(d[0])
        sec = float(np.median(sel_dev))
        print(json.dumps(dict(
            workload=name, n=A.shape[0], nnz=A.nnz, dtype=F.dtype.name,
            selinv_seconds=sec, selinv_seconds_all=sel_dev, selinv_wall_seconds=float(np.median(sel_wall)),
            selinv_flops=info["flops"], selinv_tflops=info["flops"] / sec / 1e12, selinv_peak_scratch_bytes=info["peak_bytes"],
            selinv_batches=info["batches"], budget_bytes=args.budget,
            logabsdet_wall_seconds=float(np.median(det_wall)), logabsdet_wall_seconds_all=det_wall, logabs=la, sign=sign,
            factor_seconds=st["t_total"], factor_flops=st["flops_factor"], factor_tflops=st["flops_factor"] / st["t_total"] / 1e12,
            selinv_over_factor_seconds=sec / st["t_total"], selinv_over_factor_flops=info["flops"] / st["flops_factor"],
            check_trace_rel=chk_tr, check_diag0_rel=chk_d0)), flush=True)
        F.free()


if __name__ == "__main__":
    main()
