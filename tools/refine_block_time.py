"""Time the lockstep refined solves (hs_refine_block.hip) against the looped ones and against the block solves they are made of.

    python tools/refine_block_time.py [--n N] [--nrhs K] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_128, helmholtz3d_112:swlevel=4,tol=1e-4).
Per workload, on a device block of K right-hand sides (default 32) and after one warm-up call of each path: the wall time (median of N calls)
of hs_ldiv_refine_block_dev_* and of the looped hs_ldiv_refine_dev_* on the same handle and block, with and without ferr; the block solves,
column applications and corrections of the lockstep call (hs_ldiv_refine_block_info); the time per lockstep correction -- (wall with
corrections - wall with itmax = 0) / corrections -- against one hs_ldiv_block_dev_t_* of the same column count (hs_ldiv_block_info of
the same run); and the bytes one fused residual pass over K columns moves, to be divided by the resid_block_kernel time of a kernel-trace
profile of the same run, with the device copy bandwidth (torch, read + write) as the yardstick."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import hsamd
from condest_time import copy_bandwidth, parse


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="calls per measurement")
    ap.add_argument("--nrhs", type=int, default=32)
    ap.add_argument("--trans", type=int, default=0)
    ap.add_argument("workloads", nargs="*", default=["poisson3d_128", "helmholtz3d_112:swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    hs = hsamd.load()
    L = hs._lib.lib()
    pf, pi = hs._lib.p_f64, hs._lib.p_i64
    print(f"refine_block_time: median of {args.n} calls after a warm-up; device copy bandwidth {copy_bandwidth():.0f} GB/s (read + write)")
    for spec in args.workloads:
        name, kw = parse(spec)
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        nd = hs.permuted(nd, hs.invperm(perm))
        F = hs.factor(A, nd, nd_loc, **kw)
        n, nnz, k = A.shape[0], A.nnz, args.nrhs
        cplx = F.dtype.kind == "c"
        esz = F.dtype.itemsize
        print(f"\n{spec}: n = {n}, nnz = {nnz}, {F.dtype.name}, options {kw}, nrhs = {k}, trans = {args.trans}; factor {F.stats()['t_total']:.2f} s")
        rng = np.random.default_rng(5)
        B = rng.standard_normal((k, n)) + (1j * rng.standard_normal((k, n)) if cplx else 0.0)  # row j = right-hand side j
        dB = torch.from_numpy(np.ascontiguousarray(B.astype(F.dtype))).to("cuda:0")
        dX = torch.zeros_like(dB)
        be, fe, st = np.zeros(k), np.zeros(k), np.zeros(k, dtype=np.int64)
        sfx = "z" if cplx else "d"
        blk = getattr(L, "hs_ldiv_refine_block_dev_" + sfx)
        loop = getattr(L, "hs_ldiv_refine_dev_" + sfx)
        bsolve = getattr(L, "hs_ldiv_block_dev_t_" + sfx)

        def run(fn, itmax, ferr):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hs._lib.check(fn(F._h, args.trans, C.c_void_p(dX.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, k, itmax, be.ctypes.data_as(pf),
                             fe.ctypes.data_as(pf) if ferr else None, st.ctypes.data_as(pi), None))
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def med(fn, itmax, ferr):
            run(fn, itmax, ferr)
            return float(np.median([run(fn, itmax, ferr) for _ in range(args.n)]))

        # one block solve of k columns (device seconds)
        tt = []
        for _ in range(args.n + 1):
            hs._lib.check(bsolve(F._h, args.trans, C.c_void_p(dX.data_ptr()), n, C.c_void_p(dB.data_ptr()), n, n, k, None))
            tt.append(hs.ldiv_block_info(F)["seconds"])
        t_bs = float(np.median(tt[1:]))
        print(f"  one block solve of {k} columns        {1e3 * t_bs:9.2f} ms (device)")
        for ferr in (False, True):
            tb0 = med(blk, 0, ferr)
            tb = med(blk, 5, ferr)
            info = hs.ldiv_refine_block_info()
            steps_b, berr_b = st.copy(), be.copy()
            tl = med(loop, 5, ferr)
            steps_l = st.copy()
            corr = int(steps_b.max())
            per = (tb - tb0) / corr if corr else float("nan")
            tag = "with ferr" if ferr else "no ferr  "
            print(f"  {tag}: lockstep {1e3 * tb:9.2f} ms wall ({1e3 * info['seconds']:.2f} ms device), looped {1e3 * tl:9.2f} ms wall: looped / lockstep {tl / tb:.2f}")
            print(f"             steps {steps_b.min()}..{steps_b.max()} (looped {steps_l.min()}..{steps_l.max()}), berr max {berr_b.max():.1e}" +
                  (f", ferr max {fe.max():.1e}" if ferr else "") +
                  f"; {info['block_solves']} block solves, {info['column_applications']} column applications "
                  f"({info['estimator_column_applications']} by the estimators), {info['residual_launches']} residual passes, "
                  f"workspace {info['workspace_bytes'] / 2**20:.0f} MiB")
            if not ferr:
                print(f"             lockstep correction: ({1e3 * tb:.2f} - {1e3 * tb0:.2f}) ms / {corr} = {1e3 * per:.2f} ms = {per / t_bs:.3f} x one block solve of {k} columns")
        cb = 4 if cplx else 8
        passes = -(-k // cb)
        byt = passes * (8 * (n + 1) + 4 * nnz + esz * nnz) + k * (esz * n * 3 + 8 * n)  # the row tile once per CB columns; x once, b, r, w per column
        print(f"  fused residual pass over {k} columns: {byt / 1e6:.1f} MB (rowptr, colind, values {passes} times; x once, b, r, w per column)")
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
