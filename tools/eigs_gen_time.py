"""Time the generalized shift-invert eigenpairs (hs_eigs_gen_*) next to the standard call on the same handle.

    python tools/eigs_gen_time.py [--n N] [--nev 10] [--block 16] [--ncv 0] [--tol 1e-10] [WORKLOAD]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_64).  A is factored once, sigma = 0; the pencil is
(A, M = I + A/4), whose eigenvectors are those of A.  Three cases in one process on that handle: hs_eigs_* (the eigenpairs of A), then
hs_eigs_gen_* with the Euclidean and with the op(M) inner product.  Per case: one warm-up and N calls with the vectors returned into a
device array (where = 1); the median of the device seconds between the call's own two HIP events (hs_eigs_info), block solves, restarts,
the products with M and the columns they multiplied (hs_eigs_gen_info), the worst true residual, and from one further call with
hsk_eigs_phase_timing on the host-clock seconds of the products with M (hsk_eigs_gen_mprod_seconds) and of the whole call: their quotient
is the share of the products.  One JSON line per case, then one with the ratios to the standard call."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import hsamd
from ldiv_t_time import parse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="timed calls (after one warm-up)")
    ap.add_argument("--nev", type=int, default=10)
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--ncv", type=int, default=0, help="basis columns (0: the library's default)")
    ap.add_argument("--maxrestart", type=int, default=100)
    ap.add_argument("workload", nargs="?", default="poisson3d_64")
    args = ap.parse_args()
    hs = hsamd.load()
    L = hs._lib.lib()
    dev = torch.device("cuda:0")
    name, kw = parse(args.workload)
    A, b, nd = hs.problems.make_problem(name, rhs="randn")
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    A = A[perm - 1][:, perm - 1].tocsc()
    nd = hs.permuted(nd, hs.invperm(perm))
    F = hs.factor(A, nd, nd_loc, **kw)
    n, nev = A.shape[0], args.nev
    cplx = F.dtype.kind == "c"
    M = (sp.identity(n, dtype=F.dtype, format="csc") + A / 4).tocsc()
    M.sort_indices()
    mcp, mrv = M.indptr.astype(np.int64) + 1, M.indices.astype(np.int64) + 1
    mnz = np.ascontiguousarray(M.data, dtype=F.dtype)
    std, gen = getattr(L, "hs_eigs_z" if cplx else "hs_eigs_d"), getattr(L, "hs_eigs_gen_z" if cplx else "hs_eigs_gen_d")
    spt = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    dX = torch.zeros((nev + 1, n), dtype=torch.complex128 if cplx else torch.float64, device=dev)  # row i = column i of the column-major block
    lam, res, est = np.zeros(2 * (nev + 1)), np.zeros(nev + 1), np.zeros(nev + 1)
    nout, nconv = C.c_int64(), C.c_int64()
    pf = lambda a: a.ctypes.data_as(hs._lib.p_f64)  # noqa: E731
    pi = lambda a: a.ctypes.data_as(hs._lib.p_i64)  # noqa: E731
    tail = (nev, args.ncv, args.block, 0.0, 0.0, args.tol, args.maxrestart, None, n, 0, 1, pf(lam), C.c_void_p(dX.data_ptr()), n, pf(res), pf(est), C.byref(nout),
            C.byref(nconv), spt)
    t_std = None
    out = []
    for case, inner in (("standard", None), ("euclid", 0), ("M", 1)):

        def call():
            if inner is None:
                hs._lib.check(std(F._h, 0, n, *tail))
            else:
                hs._lib.check(gen(F._h, 0, n, pi(mcp), pi(mrv), mnz.ctypes.data_as(C.c_void_p), inner, *tail))
            return hs.eigs_info(), hs.eigs_gen_info()

        call()
        infos = [call() for _ in range(args.n)]
        t = float(np.median([i[0]["seconds"] for i in infos]))
        L.hsk_eigs_phase_timing(1)
        w0 = time.perf_counter()
        call()
        wall = time.perf_counter() - w0
        L.hsk_eigs_phase_timing(0)
        t_mprod = float(L.hsk_eigs_gen_mprod_seconds())
        i0, g0 = infos[0]
        t_std = t if t_std is None else t_std
        out.append(dict(case=case, t_eigs=t, ratio_to_standard=t / t_std, mprod_share=t_mprod / wall))
        print(json.dumps(dict(
            workload=args.workload, case=case, n=n, dtype=F.dtype.name, nev=nev, block=args.block, ncv=i0["ncv"], tol=args.tol, t_eigs=t,
            t_all=[i[0]["seconds"] for i in infos], block_solves=i0["block_solves"], restarts=i0["restarts"], orth_passes=i0["orth_passes"], replaced=i0["replaced"],
            m_products=g0["m_products"], m_columns=g0["m_columns"], m_bytes=g0["m_bytes"], nnz_M=int(M.nnz), workspace_bytes=i0["workspace_bytes"], nconv=int(nconv.value),
            nout=int(nout.value), resid_max=float(res[:nout.value].max()), est_max=float(est[:nout.value].max()), t_mprod_timed=t_mprod, t_call_timed=wall,
            lam_first=[float(lam[0]), float(lam[1])])), flush=True)
    print(json.dumps(dict(workload=args.workload, summary=out)), flush=True)
    del dX
    F.free()
    hs.trim()


if __name__ == "__main__":
    main()
