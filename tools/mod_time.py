"""Time solves with a rank-k modification of A through the stored factorization (hs_mod_*) against the block solve of the same handle and
against refactoring.

    python tools/mod_time.py [--n N] [--k 8,64,256] [--cols 32] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_128 and helmholtz3d_64:swlevel=4,tol=1e-4).  U, V are
random device blocks (U scaled by 1 / n, so that C stays near the identity).  Per k: hs_mod_create_dev_* (build seconds of hs_mod_info: one
block solve with k columns, the inner product, LU and rcond of C), one warm-up and N hs_mod_ldiv_dev_* calls of `cols` columns alternating
with hs_ldiv_block_dev_* on the same block (device seconds: hs_mod_info and hs_ldiv_block_info, medians), the first transposed solve
(which builds W) and a later one, and the residual of two columns against A + U V^H on the host.  After the last k the handle is freed and
the matrix factored again: the refactorization a modified solve replaces.  One JSON line per (workload, k)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hsamd
from ldiv_t_time import parse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="timed rounds (after one warm-up)")
    ap.add_argument("--k", default="8,64,256")
    ap.add_argument("--cols", type=int, default=32)
    ap.add_argument("workloads", nargs="*", default=["poisson3d_128", "helmholtz3d_64:swlevel=4,tol=1e-4"])
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
        t0 = time.perf_counter()
        F = hs.factor(A, nd, nd_loc, **kw)
        t_factor_wall = time.perf_counter() - t0
        t_factor = F.stats()["t_total"]
        n, m = A.shape[0], args.cols
        cplx = F.dtype.kind == "c"
        sfx = "_z" if cplx else "_d"
        dt = torch.complex128 if cplx else torch.float64
        s = torch.cuda.current_stream(dev)
        sp = C.c_void_p(s.cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        gen = torch.Generator(device="cpu").manual_seed(1)
        dB = torch.randn((m, n), dtype=dt, generator=gen).to(dev)  # row i of the tensor = column i of the column-major block
        dX = torch.empty_like(dB)
        fblk = getattr(L, "hs_ldiv_block_dev" + sfx)
        fmod = getattr(L, "hs_mod_ldiv_dev" + sfx)
        for k in [int(v) for v in args.k.split(",")]:
            dU = (torch.randn((k, n), dtype=dt, generator=gen) / n).to(dev)
            dV = torch.randn((k, n), dtype=dt, generator=gen).to(dev)
            h = C.c_void_p()
            hs._lib.check(getattr(L, "hs_mod_create_dev" + sfx)(F._h, n, k, p(dU), n, p(dV), n, sp, C.byref(h)))
            M = hs.ModifiedFactor(h, F, k)
            build = M.info()

            def mod(trans):
                hs._lib.check(fmod(M._h, trans, p(dX), n, p(dB), n, n, m, sp))
                return M.info()["solve_seconds"]

            def block():
                hs._lib.check(fblk(F._h, 0, p(dX), n, p(dB), n, n, m, sp))
                return hs.ldiv_block_info(F)["seconds"]

            mod(0), block()
            tm, tb = [], []
            for _ in range(args.n):
                tm.append(mod(0))
                tb.append(block())
            t0 = time.perf_counter()
            mod(1)
            s.synchronize()
            t_first_t = time.perf_counter() - t0  # builds W
            tt = [mod(1) for _ in range(args.n)]
            mod(0)
            Xh = dX[:2].cpu().numpy().T
            Bh = dB[:2].cpu().numpy().T
            Uh, Vh = dU.cpu().numpy().T, dV.cpu().numpy().T
            R = Bh - A @ Xh - Uh @ (Vh.conj().T @ Xh)
            res = float(max(np.linalg.norm(R[:, j]) / np.linalg.norm(Bh[:, j]) for j in range(2)))
            info = M.info()
            print(json.dumps(dict(
                workload=spec, n=n, dtype=F.dtype.name, k=k, cols=m, chunk_cols=int(os.environ.get("HS_LDIV_BLOCK_COLS", "32") or 32),
                t_build=build["build_seconds"], rcond=build["rcond"], t_mod=float(np.median(tm)), t_mod_all=tm, t_block=float(np.median(tb)), t_block_all=tb,
                mod_over_block=float(np.median(tm) / np.median(tb)), t_mod_trans_first_wall=t_first_t, t_mod_trans=float(np.median(tt)),
                bytes_held=info["bytes"], residual_2cols=res, t_factor=t_factor, t_factor_wall=t_factor_wall)), flush=True)
            M.free()
            del dU, dV
        F.free()
        hs.trim()
        t0 = time.perf_counter()
        F = hs.factor(A, nd, nd_loc, **kw)
        print(json.dumps(dict(workload=spec, n=n, refactor=True, t_refactor=F.stats()["t_total"], t_refactor_wall=time.perf_counter() - t0)), flush=True)
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
