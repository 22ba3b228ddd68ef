"""Time ldiv!(F, b) against ldiv!(transpose(F), b) and ldiv!(adjoint(F), b) on the same factors.

    python tools/ldiv_t_time.py [--n N] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_128, helmholtz3d_64, helmholtz3d_64:swlevel=4,tol=1e-4).
Each workload is factored once; then N calls of each solve (stats.t_solve: device time of one hs_ldiv*) are timed, and the median is
printed in ms and in GB/s against hs_get_stats().bytes_solve (the factor bytes one solve reads), with the residual of each solve."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import hsamd


def parse(spec):
    name, _, opt = spec.partition(":")
    kw = dict(swlevel=0)
    for item in filter(None, opt.split(",")):
        k, v = item.split("=")
        if k == "tol":
            kw.update(atol=float(v), rtol=float(v))
        else:
            kw[k] = int(v)
    if kw["swlevel"] > 0:
        kw.setdefault("swsize", 8)
    return name, kw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10, help="calls per solve kind")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_128", "helmholtz3d_64", "helmholtz3d_64:swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    hs = hsamd.load()
    print(f"ldiv_t_time: {args.n} calls per solve kind, median device time (stats.t_solve)")
    for spec in args.workloads:
        name, kw = parse(spec)
        t0 = time.perf_counter()
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        nd = hs.permuted(nd, hs.invperm(perm))
        b = b[perm - 1]
        t1 = time.perf_counter()
        F = hs.factor(A, nd, nd_loc, **kw)
        st = F.stats()
        gb = st["bytes_solve"] / 1e9
        print(f"\n{spec}: n = {A.shape[0]}, {F.dtype.name}, options {kw}; setup {t1 - t0:.1f} s, factor {st['t_total']:.2f} s, "
              f"bytes_solve {gb:.2f} GB, maxrank {hs.maxrank(F)}")
        res = {}
        for label, op, M in (("ldiv", F, A), ("transpose", hs.transpose(F), A.T), ("adjoint", hs.adjoint(F), A.conj().T)):
            ts = []
            for _ in range(args.n):
                x = hs.ldiv(op, b)
                ts.append(F.stats()["t_solve"])
            ms = 1e3 * float(np.median(ts))
            res[label] = ms
            r = np.linalg.norm(M @ x - b) / np.linalg.norm(b)
            print(f"  {label:<9s} {ms:9.2f} ms  (min {1e3 * min(ts):8.2f})  {gb / (ms * 1e-3):8.0f} GB/s   residual {r:.1e}")
        print(f"  ratio transpose / ldiv = {res['transpose'] / res['ldiv']:.2f}, adjoint / ldiv = {res['adjoint'] / res['ldiv']:.2f}")
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
