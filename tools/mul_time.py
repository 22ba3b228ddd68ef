"""Time the product with the stored factorization (hs_mul_dev_*) against the block solve (hs_ldiv_block_dev_t_*) of the same handle, in one
process.

    python tools/mul_time.py [--n 5] [--k 1,16,32] [--trans 0,1] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_64, poisson3d_128 and
helmholtz3d_64:swlevel=4,tol=1e-4).  Both paths run on device arrays and are timed by the library's own event pairs (hs_mul_info,
hs_ldiv_block_info: device seconds).  One warm-up of each, then N rounds in which the two alternate; medians.  One JSON line per
(workload, trans, k): the two times and their ratio, the factor bytes the model says a call reads (the same for both: chunks x sum over
fronts of (ni^2 + 2 ni nb) sizeof(T)) and the rates they give, the executed flops of both.  The output of a run is kept in
profiles/mul_time.txt."""
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
    ap.add_argument("--k", default="1,16,32")
    ap.add_argument("--trans", default="0,1")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_64", "poisson3d_128", "helmholtz3d_64:swlevel=4,tol=1e-4"])
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
        n = A.shape[0]
        cplx = F.dtype.kind == "c"
        fsolve = L.hs_ldiv_block_dev_t_z if cplx else L.hs_ldiv_block_dev_t_d
        fmul = L.hs_mul_dev_z if cplx else L.hs_mul_dev_d
        s = torch.cuda.current_stream(dev)
        sp = C.c_void_p(s.cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())
        for k in [int(x) for x in args.k.split(",")]:
            dB = torch.randn((k, n), dtype=torch.complex128 if cplx else torch.float64, generator=torch.Generator(device="cpu").manual_seed(k)).to(dev)
            dX = torch.empty_like(dB)
            for trans in [int(x) for x in args.trans.split(",")]:

                def solve():
                    hs._lib.check(fsolve(F._h, trans, p(dX), n, p(dB), n, n, k, sp))
                    return hs.ldiv_block_info(F)

                def mul():
                    hs._lib.check(fmul(F._h, trans, p(dX), n, p(dB), n, n, k, sp))
                    return hs.mul_info(F)

                solve(), mul()
                ts, tm = [], []
                for _ in range(args.n):
                    si = solve()
                    mi = mul()
                    ts.append(si["seconds"])
                    tm.append(mi["seconds"])
                t_solve, t_mul = float(np.median(ts)), float(np.median(tm))
                print(json.dumps(dict(
                    workload=spec, n=n, dtype=F.dtype.name, k=k, trans=trans, chunk_cols=int(os.environ.get("HS_LDIV_BLOCK_COLS", "32") or 32),
                    t_mul=t_mul, t_mul_all=tm, t_solve=t_solve, t_solve_all=ts, mul_over_solve=t_mul / t_solve,
                    factor_bytes=mi["factor_bytes"], mul_factor_TBps=mi["factor_bytes"] / t_mul / 1e12, solve_factor_TBps=si["factor_bytes"] / t_solve / 1e12,
                    mul_flops_executed=mi["flops_executed"], solve_flops_executed=si["flops_executed"])), flush=True)
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
