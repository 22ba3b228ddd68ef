"""Time the block solve on Float32-stored factors (hs_f32_ldiv_dev_*) against the FP64 block solve (hs_ldiv_block_dev_t_*) of the handle the
copy was demoted from, in one process, and report what the copy holds.

    python tools/f32_time.py [--n N] [--k 1,16,32] [--gmres-cols 4] [--out FILE] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_64, poisson3d_128 and
helmholtz3d_64:swlevel=4,tol=1e-4).  Both solves run on device arrays and are timed by the library's own event pairs (hs_f32_info,
hs_ldiv_block_info: device seconds).  Per column count and trans (N, C): one warm-up of each, then N alternating pairs; medians.  Per workload:
the demotion seconds, the Float32 value bytes against hs_get_stats().bytes_factors, and the GMRES iterations to a relative residual of
1e-8 with Pr=G against Pr=F on --gmres-cols host columns.  One JSON line per (workload, k, trans) and one per workload; --out appends them
to FILE as well."""
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
    ap.add_argument("--n", type=int, default=5, help="timed pairs (after one warm-up)")
    ap.add_argument("--k", default="1,16,32")
    ap.add_argument("--gmres-cols", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("workloads", nargs="*", default=["poisson3d_64", "poisson3d_128", "helmholtz3d_64:swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    hs = hsamd.load()
    L = hs._lib.lib()
    dev = torch.device("cuda:0")

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for spec in args.workloads:
        name, kw = parse(spec)
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        nd = hs.permuted(nd, hs.invperm(perm))
        F = hs.factor(A, nd, nd_loc, **kw)
        G = hs.demote(F)
        n = A.shape[0]
        cplx = F.dtype.kind == "c"
        f64 = L.hs_ldiv_block_dev_t_z if cplx else L.hs_ldiv_block_dev_t_d
        f32 = L.hs_f32_ldiv_dev_z if cplx else L.hs_f32_ldiv_dev_d
        s = torch.cuda.current_stream(dev)
        sp = C.c_void_p(s.cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        gi, st = G.info(), F.stats()
        for k in [int(v) for v in args.k.split(",")]:
            dB = torch.randn((k, n), dtype=torch.complex128 if cplx else torch.float64, generator=torch.Generator(device="cpu").manual_seed(k)).to(dev)
            dX, dY = torch.empty_like(dB), torch.empty_like(dB)

            def run32(t):
                hs._lib.check(f32(G._h, t, p(dX), n, p(dB), n, n, k, sp))
                return G.info()["solve_seconds"]

            def run64(t):
                hs._lib.check(f64(F._h, t, p(dY), n, p(dB), n, n, k, sp))
                return hs.ldiv_block_info(F)["seconds"]

            for t in (0, 2):
                run32(t), run64(t)
                a, c = [], []
                for _ in range(args.n):
                    a.append(run32(t))
                    c.append(run64(t))
                diff = float((torch.linalg.vector_norm(dX - dY, dim=1) / torch.linalg.vector_norm(dY, dim=1)).max().item())
                emit(dict(workload=spec, n=n, dtype=F.dtype.name, k=k, trans="NTC"[t], t_f32=float(np.median(a)), t_f32_all=a, t_f64=float(np.median(c)), t_f64_all=c,
                          f32_over_f64=float(np.median(a) / np.median(c)), worst_col_f32_vs_f64=diff))
            del dB, dX, dY
        its = {}
        kc = args.gmres_cols
        Bh = np.random.default_rng(1).standard_normal((n, kc)).astype(F.dtype)
        for t in ("N", "C"):
            for label, Pr in (("G", G), ("F", F)):
                X, ch = hs.gmres_block(A, Bh, Pr=Pr, trans=t, reltol=1e-8, restart=30, maxiter=60, log=True)
                Aop = A if t == "N" else A.conj().T
                res = max(float(np.linalg.norm(Bh[:, j] - Aop @ X[:, j]) / np.linalg.norm(Bh[:, j])) for j in range(kc))
                its[f"{t}_{label}"] = dict(iters=[c["iters"] for c in ch], converged=all(c["isconverged"] for c in ch), worst_true_residual=res)
        emit(dict(workload=spec, n=n, dtype=F.dtype.name, demote_seconds=gi["demote_seconds"], f32_value_bytes=gi["value_bytes"], f32_other_bytes=gi["index_bytes"],
                  f32_flushed=gi["flushed"], bytes_factors=st["bytes_factors"], value_bytes_over_bytes_factors=gi["value_bytes"] / st["bytes_factors"], gmres_to_1e_8=its))
        G.free()
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
