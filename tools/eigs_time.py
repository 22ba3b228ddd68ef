"""Time shift-invert eigenpairs from the stored factors (hs_eigs_*) over the block width.

    python tools/eigs_time.py [--n N] [--nev 10] [--block 1,8,16,32] [--ncv 0] [--tol 1e-10] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_64 and helmholtz3d_64:swlevel=4,tol=1e-4); sigma = 0,
the factorization of the matrix itself.  Per block width: one warm-up and N hs_eigs_* calls with the vectors returned into a device array
(where = 1), ncv the library's default for that width unless --ncv is given.  Reported: the median of the device seconds between the call's
own two HIP events (hs_eigs_info), block solves, restarts, the worst true residual, and the host-clock split of one further call with hsk_eigs_phase_timing on
(block solves / orthogonalisation / restarts / Ritz vectors and residuals; it adds one synchronisation per block solve).  One JSON line per
(workload, block); the last line per workload names the fastest width."""
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
    ap.add_argument("--n", type=int, default=5, help="timed calls (after one warm-up)")
    ap.add_argument("--nev", type=int, default=10)
    ap.add_argument("--block", default="1,8,16,32")
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--ncv", type=int, default=0, help="basis columns (0: the library's default for each width)")
    ap.add_argument("--maxrestart", type=int, default=100)
    ap.add_argument("workloads", nargs="*", default=["poisson3d_64", "helmholtz3d_64:swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    hs = hsamd.load()
    L = hs._lib.lib()
    dev = torch.device("cuda:0")
    for spec in args.workloads:
        name, kw = parse(spec)
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        nd = hs.permuted(nd, hs.invperm(perm))
        F = hs.factor(A, nd, nd_loc, **kw)
        n, nev = A.shape[0], args.nev
        cplx = F.dtype.kind == "c"
        fn = getattr(L, "hs_eigs_z" if cplx else "hs_eigs_d")
        s = torch.cuda.current_stream(dev)
        sp = C.c_void_p(s.cuda_stream)
        dX = torch.zeros((nev + 1, n), dtype=torch.complex128 if cplx else torch.float64, device=dev)  # row i = column i of the column-major block
        lam, res, est = np.zeros(2 * (nev + 1)), np.zeros(nev + 1), np.zeros(nev + 1)
        nout, nconv = C.c_int64(), C.c_int64()
        pf = lambda a: a.ctypes.data_as(hs._lib.p_f64)  # noqa: E731
        best = None
        for blk in [int(v) for v in args.block.split(",")]:

            def call():
                hs._lib.check(fn(F._h, 0, n, nev, args.ncv, blk, 0.0, 0.0, args.tol, args.maxrestart, None, n, 0, 1, pf(lam), C.c_void_p(dX.data_ptr()), n, pf(res), pf(est),
                                 C.byref(nout), C.byref(nconv), sp))
                return hs.eigs_info()

            call()
            infos = [call() for _ in range(args.n)]
            t = float(np.median([i["seconds"] for i in infos]))
            L.hsk_eigs_phase_timing(1)
            call()
            L.hsk_eigs_phase_timing(0)
            ph = np.zeros(4)
            hs._lib.check(L.hsk_eigs_phases(pf(ph)))
            i0 = infos[0]
            print(json.dumps(dict(
                workload=spec, n=n, dtype=F.dtype.name, nev=nev, block=blk, ncv=i0["ncv"], tol=args.tol, t_eigs=t, t_all=[i["seconds"] for i in infos],
                block_solves=i0["block_solves"], column_applications=i0["column_applications"], restarts=i0["restarts"], orth_passes=i0["orth_passes"],
                replaced=i0["replaced"], nconv=int(nconv.value), nout=int(nout.value), resid_max=float(res[:nout.value].max()), est_max=float(est[:nout.value].max()),
                workspace_bytes=i0["workspace_bytes"], t_solve=float(ph[0]), t_orth=float(ph[1]), t_restart=float(ph[2]), t_finish=float(ph[3]),
                lam_first=[float(lam[0]), float(lam[1])])), flush=True)
            if nconv.value == nout.value and (best is None or t < best[1]):
                best = (blk, t)
        print(json.dumps(dict(workload=spec, fastest_block=best[0] if best else None, t_eigs=best[1] if best else None)), flush=True)
        del dX
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
