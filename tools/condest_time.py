"""Time the accuracy tools (hs_condest.hip) against the solves they are made of.

    python tools/condest_time.py [--n N] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_128, helmholtz3d_112:swlevel=4,tol=1e-4).
Per workload: one F \\ b and one F' \\ b (median stats.t_solve of N calls); hs_condest wall time (p = 1 and Inf) with the solves it made and
the sum of their times; ldiv_refine steps and wall time per step against one solve; the bytes one fused residual pass (r = b - A x,
w = |b| + |A||x|) moves, to be divided by the resid_kernel time of a kernel-trace profile of the same run; and the device copy bandwidth
(torch, read + write) as the yardstick for it."""
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


def copy_bandwidth():
    import torch

    x = torch.empty(1 << 27, dtype=torch.float64, device="cuda")  # 1 GiB
    y = torch.empty_like(x)
    y.copy_(x)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(5):
        e0.record()
        y.copy_(x)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return 2 * x.numel() * 8 / min(ts) / 1e9


def wall(f, reps):
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="calls per measurement")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_128", "helmholtz3d_112:swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    hs = hsamd.load()
    print(f"condest_time: median of {args.n} calls; device copy bandwidth {copy_bandwidth():.0f} GB/s (read + write)")
    for spec in args.workloads:
        name, kw = parse(spec)
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        nd = hs.permuted(nd, hs.invperm(perm))
        b = b[perm - 1]
        F = hs.factor(A, nd, nd_loc, **kw)
        n, nnz = A.shape[0], A.nnz
        esz = F.dtype.itemsize
        print(f"\n{spec}: n = {n}, nnz = {nnz}, {F.dtype.name}, options {kw}; factor {F.stats()['t_total']:.2f} s, maxrank {hs.maxrank(F)}")
        ts = {}
        for label, op in (("F", F), ("F'", hs.adjoint(F))):
            tt = []
            for _ in range(args.n):
                hs.ldiv(op, b)
                tt.append(F.stats()["t_solve"])
            ts[label] = float(np.median(tt))
            print(f"  one {label:<2s} \\ b    {1e3 * ts[label]:8.2f} ms (device)")
        hs.opnorm(F, np.inf)  # builds the CSR map once
        for p, pn in ((1, "1"), (np.inf, "Inf")):
            op = F if p == 1 else hs.transpose(F)
            _, (est, ns) = wall(lambda: hs.opnormestinv(op, nsolves=True), 1)
            tw, cond = wall(lambda: hs.condest(F, p), args.n)
            tsum = ns / 2 * (ts["F"] + ts["F'"])  # half of the columns go through op(F)^-1, half through its adjoint
            print(f"  condest p={pn:<3s} {1e3 * tw:8.2f} ms wall, {ns} solves ({1e3 * tsum:.2f} ms of solves): ratio {tw / tsum:.3f}   "
                  f"cond ~ {cond:.3e}, ||F^-1|| ~ {est:.3e}")
        t0, (x0, be0, _, _) = wall(lambda: hs.ldiv_refine(F, b, itmax=0, ferr=False), args.n)
        t1, (x1, be1, _, st) = wall(lambda: hs.ldiv_refine(F, b, ferr=False), args.n)
        per = (t1 - t0) / st if st else float("nan")
        print(f"  refine: berr {be0:.1e} -> {be1:.1e} in {st} steps; wall {1e3 * t0:.2f} ms (itmax=0) / {1e3 * t1:.2f} ms: {1e3 * per:.2f} ms per step "
              f"= {per / ts['F']:.3f} x one F \\ b")
        tf, (_, _, fe, _) = wall(lambda: hs.ldiv_refine(F, b, itmax=0), 1)
        print(f"  refine with ferr: {1e3 * tf:.2f} ms wall, ferr {fe:.1e}")
        byt = 8 * (n + 1) + 4 * nnz + esz * nnz + esz * n * 3 + 8 * n  # rowptr, colind, values, x (each once), b, r, w
        print(f"  fused residual pass: {byt / 1e6:.1f} MB (rowptr, colind, values, x once, b, r, w)")
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
