"""Time hs_selinv_lr on a compressed factorization against hs_selinv on the exact factorization of the same matrix.

    python tools/selinv_lr_time.py [--n N] [--swlevel L] [--tol T] [--mf M] [WORKLOAD ...]

WORKLOAD is a problems.NAMED entry (default: poisson3d_64).  Per workload, in one process: the matrix is factored with compression
(swlevel, atol = rtol = tol) and exactly (swlevel = 0); after one warm-up, N calls (default 5) of hs_selinv_lr on the compressed handle and
of hs_selinv on the exact one (diag + pattern), medians reported.  The clocks are the library's own event pairs (hs_selinv_lr_info,
hs_selinv_info).  Also one 32-column hs_ldiv_block_t on the compressed handle (wall time of the blocking call, after a warm-up), the only
route to diag(F^-1) without hs_selinv_lr: n / 32 such solves, reported as an EXTRAPOLATION, never run.  Two JSON lines per workload: the
compressed handle's figures, then the exact handle's ("Not run" with the reason when it does not fit next to what the first left behind)."""
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
    ap.add_argument("--n", type=int, default=5, help="timed calls per function (after one warm-up)")
    ap.add_argument("--swlevel", type=int, default=4)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--mf", type=int, default=0)
    ap.add_argument("--no-exact", action="store_true", help="skip the exact handle (when both factorizations do not fit the device)")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_64"])
    args = ap.parse_args()
    hs = hsamd.load()
    for name in args.workloads:
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        nd = hs.permuted(nd, hs.invperm(perm))
        n = A.shape[0]
        out = dict(workload=name, n=n, nnz=A.nnz, swlevel=args.swlevel, tol=args.tol, mf=args.mf)

        F = hs.factor(A, nd, nd_loc, swlevel=args.swlevel, atol=args.tol, rtol=args.tol, mf=args.mf)
        st = F.stats()
        secs, info = [], None
        for it in range(args.n + 1):
            d, Z = hs.selinv_lr(F)
            info = hs.selinv_lr_info(F)
            if it:
                secs.append(info["seconds"])
        sec = float(np.median(secs))
        # what was timed, checked end to end: one diagonal entry against a solve with a unit vector
        e0 = np.zeros(n, dtype=F.dtype)
        e0[n // 2] = 1.0
        chk = abs(F.solve(e0)[n // 2] - d[n // 2]) / abs(d[n // 2])
        B = np.zeros((n, 32), dtype=F.dtype, order="F")
        B[np.arange(32) * (n // 32), np.arange(32)] = 1.0
        blk = []
        for it in range(3):
            t0 = time.perf_counter()
            hs.ldiv_block_t(hs.transpose(F), B)
            blk.append(time.perf_counter() - t0)
        blk_sec = float(np.median(blk[1:]))
        out.update(dtype=F.dtype.name, maxrank=hs.maxrank(F), selinv_lr_seconds=sec, selinv_lr_seconds_all=secs, selinv_lr_flops=info["flops"],
                   flops_dense_form=info["flops_dense_form"], selinv_lr_tflops=info["flops"] / sec / 1e12, selinv_lr_peak_scratch_bytes=info["peak_bytes"],
                   selinv_lr_batches=info["batches"], lowrank_fronts=info["lowrank_fronts"], max_rank=info["max_rank"],
                   factor_seconds=st["t_total"], selinv_lr_over_factor_seconds=sec / st["t_total"], check_diag_rel=chk,
                   ldiv_block_t_32_wall_seconds=blk_sec, diag_by_block_solves_seconds_EXTRAPOLATED=blk_sec * n / 32)
        F.free()

        print(json.dumps(out), flush=True)  # (the compressed handle's figures are out before the exact handle is tried)

        out = dict(workload=name, n=n)
        if args.no_exact:
            out.update(selinv_exact_seconds="Not run")
        else:
            try:
                Fe = hs.factor(A, nd, nd_loc, swlevel=0)
                ste = Fe.stats()
                secs_e, info_e = [], None
                for it in range(args.n + 1):
                    hs.selinv(Fe)
                    info_e = hs.selinv_info(Fe)
                    if it:
                        secs_e.append(info_e["seconds"])
                sec_e = float(np.median(secs_e))
                out.update(selinv_exact_seconds=sec_e, selinv_exact_seconds_all=secs_e, selinv_exact_flops=info_e["flops"],
                           selinv_exact_tflops=info_e["flops"] / sec_e / 1e12, selinv_exact_peak_scratch_bytes=info_e["peak_bytes"],
                           factor_exact_seconds=ste["t_total"], selinv_lr_over_exact_seconds=sec / sec_e, selinv_lr_over_exact_flops=info["flops"] / info_e["flops"])
                Fe.free()
            except (hs.DeviceError, MemoryError) as e:  # e.g. both handles' leftovers do not fit the device in one process
                out.update(selinv_exact_seconds=f"Not run: {e}")
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
