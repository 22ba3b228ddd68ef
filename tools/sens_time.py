"""Time the adjoint-state sensitivities (hs_sens_dev_*) on device arrays, both forms of the reduction kernel, and the host composition the
call replaces, in one process.

    python tools/sens_time.py [--n 3] [--k 32] [--itmax 0] [--no-host] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_128 and helmholtz3d_64:swlevel=4,tol=1e-4).  k dense
random sources and cotangents.  One JSON line per workload and measurement:

  phases  hs_sens_dev_* on device blocks: the four phases of hs_sens_info (HIP events of the library), medians of N calls after one warm-up
  kernel  the reduction kernel alone on the handle's pattern and blocks of the same shape (hsk_sddmm_*, median of three launches after a
          warm-up, HIP events): form 0 = one lane per stored entry reading the column-major blocks, form 1 = the blocks transposed into
          row-major work blocks first (the two transpositions are in the time), and whether the two forms return the same bits
  host    what a user composes without the call: two host-array block solves (hs_ldiv_block_t_*) and the NumPy reduction over the pattern,
          wall clock, once"""
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


def rand(n, k, cplx, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, k))
    return np.asfortranarray(M + 1j * rng.standard_normal((n, k)) if cplx else M)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3, help="timed rounds (after one warm-up)")
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--itmax", type=int, default=0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_128", "helmholtz3d_64:swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    hs = hsamd.load()
    E = hs._lib
    L = E.lib()
    dev = torch.device("cuda:0")
    for spec in args.workloads:
        name, kw = parse(spec)
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        A.sort_indices()
        nd = hs.permuted(nd, hs.invperm(perm))
        F = hs.factor(A, nd, nd_loc, **kw)
        n, k = A.shape[0], args.k
        cplx = F.dtype.kind == "c"
        base = dict(workload=spec, n=n, nnz=int(A.nnz), dtype=F.dtype.name, k=k, chunk_cols=hs.solver._block_cols())
        B, W = rand(n, k, cplx, 1), rand(n, k, cplx, 2)

        # ---- the four phases, device arrays
        s = torch.cuda.current_stream(dev)
        up = lambda M: torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)  # row j = column j of the column-major block
        dB, dW = up(B), up(W)
        dG = torch.zeros(A.nnz, dtype=dB.dtype, device=dev)
        bB, bW = E.hs_block_arg(dB.data_ptr(), n, None, None, None), E.hs_block_arg(dW.data_ptr(), n, None, None, None)
        fdev = L.hs_sens_dev_z if cplx else L.hs_sens_dev_d
        rounds, walls = [], []
        for it in range(args.n + 1):
            t0 = time.perf_counter()
            E.check(fdev(F._h, 0, n, k, C.byref(bB), C.byref(bW), args.itmax, 0, dG.data_ptr(), None, n, None, n, s.cuda_stream))
            w = time.perf_counter() - t0
            if it > 0:
                rounds.append(hs.sens_info(F))
                walls.append(w)
        med = lambda key: float(np.median([r[key] for r in rounds]))
        print(json.dumps(dict(base, what="phases", itmax=args.itmax, seconds=med("seconds"), forward=med("seconds_forward"), adjoint=med("seconds_adjoint"),
                              reduce=med("seconds_reduce"), wall=float(np.median(walls)), groups=rounds[-1]["groups"], workspace_bytes=rounds[-1]["workspace_bytes"],
                              seconds_all=[r["seconds"] for r in rounds])), flush=True)
        G_dev = dG.cpu().numpy()
        del dB, dW, dG

        # ---- both forms of the kernel on the same pattern
        cp = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
        rv = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
        fk = L.hsk_sddmm_z if cplx else L.hsk_sddmm_d
        out = {}
        for form in (0, 1):
            G = np.zeros(A.nnz, dtype=F.dtype)
            sec = C.c_double(0.0)
            E.check(fk(n, cp.ctypes.data_as(E.p_i64), rv.ctypes.data_as(E.p_i64), k, W.ctypes.data, n, B.ctypes.data, n, 0, 0, 1, 0, form, G.ctypes.data, C.byref(sec)))
            out[form] = (sec.value, G)
        esz = 16 if cplx else 8
        model = 2.0 * n * k * esz + A.nnz * (2 * esz + 8)  # both blocks once, G read and written, the two index arrays
        print(json.dumps(dict(base, what="kernel", t_direct=out[0][0], t_row_staged=out[1][0], same_bits=bool(np.array_equal(out[0][1], out[1][1])),
                              model_bytes=model, direct_model_TBps=model / out[0][0] / 1e12)), flush=True)

        # ---- the host composition
        if not args.no_host:
            hs.ldiv_block_t(F, B[:, :1])
            t0 = time.perf_counter()
            X = hs.ldiv_block_t(F, B)
            Lam = hs.ldiv_block_t(hs.adjoint(F), W)
            t1 = time.perf_counter()
            i = A.indices
            j = np.repeat(np.arange(n), np.diff(A.indptr))
            G = np.zeros(A.nnz, dtype=F.dtype)
            for c0 in range(0, k, 8):
                G -= (Lam[i, c0:c0 + 8] * np.conj(X[j, c0:c0 + 8])).sum(axis=1)
            t2 = time.perf_counter()
            scale = float(np.abs(G).max())
            print(json.dumps(dict(base, what="host", wall_two_solves=t1 - t0, wall_numpy_reduction=t2 - t1, wall=t2 - t0, values_moved=4 * n * k,
                                  max_diff_to_device=(float(np.abs(G - G_dev).max()) / scale) if args.itmax == 0 else None)), flush=True)
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
