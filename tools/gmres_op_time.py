"""Time GMRES on op(A) (hs_gmres_block_t_*, hs_gmres_t_*) with the handle's own A against the same call with A passed as host CSC arrays, per
trans, in one process.

    python tools/gmres_op_time.py [--summarize FILE] [--n N] [--k 1,8,32] [--reltol R] [--restart M] [--maxiter I] [WORKLOAD ...]

WORKLOAD is NAME[:kind=K,swlevel=L,tol=T] with NAME a problems.NAMED entry whose matrix kind K replaces (default: poisson3d_128 and
helmholtz3d_64:kind=convdiff_helmholtz,swlevel=4,tol=1e-4).  Every call takes device arrays (where = 1) on the current torch stream.  Per
(workload, k, trans): one warm-up of each path, then N alternating pairs (own A, explicit A); medians.  The host clock runs around the call
(it returns after its last device read); the device part is the library's own event pair (hs_gmres_block_info: from the first kernel of the
iteration to the last, after A is on the device), so host - device is what a call spends before and after the iteration: the conversion and
upload of A, the workspace, the result arrays.  The explicit-A call with trans = 0 is hs_gmres_block_*, the path without this tool's
subject.  For k = 1 the single-vector entry point hs_gmres_t_* is timed as well (host clock only:
hs_gmres_block_info reports block calls alone).  One JSON line per (workload, k, trans): both paths' times with all samples, their spreads, the ratio of the device part to that of trans = 0 of the same k,
iteration counts, whether the two paths returned the same bits, and the worst residual of op(A) x = b."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def parse(spec):
    name, _, opt = spec.partition(":")
    kind, kw = None, dict(swlevel=0)
    for item in filter(None, opt.split(",")):
        k, v = item.split("=")
        if k == "kind":
            kind = v
        elif k == "tol":
            kw.update(atol=float(v), rtol=float(v))
        else:
            kw[k] = int(v)
    if kw["swlevel"] > 0:
        kw.setdefault("swsize", 8)
    return name, kind, kw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="timed pairs (after one warm-up)")
    ap.add_argument("--k", default="1,8,32")
    ap.add_argument("--reltol", type=float, default=1e-8)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--summarize", metavar="FILE", help="no GPU: print a table of the JSON lines of FILE and exit")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_128", "helmholtz3d_64:kind=convdiff_helmholtz,swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    if args.summarize:
        print("| workload | k | trans | own A: host (ms) | device (ms) | explicit A: host (ms) | device (ms) | gap own / explicit (ms) | device own - explicit (ms) | spread of the pairs (ms) | device / trans 0 | iterations | same bits |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        for line in open(args.summarize):
            if line.startswith("{"):
                d = json.loads(line)
                if d.get("entry") != "block":
                    continue
                it = d["iters"]
                print(f"| {d['workload']} | {d['k']} | {d['trans']} | {d['t_own'] * 1e3:.1f} | {d['t_own_device'] * 1e3:.1f} | {d['t_explicit'] * 1e3:.1f} | {d['t_explicit_device'] * 1e3:.1f} | "
                      f"{(d['t_own'] - d['t_own_device']) * 1e3:.1f} / {(d['t_explicit'] - d['t_explicit_device']) * 1e3:.1f} | {d['device_own_minus_explicit'] * 1e3:+.2f} | "
                      f"{d['device_pair_spread'] * 1e3:.2f} | {d['device_over_trans0']:.2f} | {min(it)}-{max(it)} | {d['same_bits']} |")
        return
    import torch

    import hsamd

    hs = hsamd.load()
    from hierarchicalsolvers_jl_amd.gmres import _csc_fields

    L = hs._lib.lib()
    dev = torch.device("cuda:0")
    pi, pf = hs._lib.p_i64, hs._lib.p_f64
    mi = args.maxiter
    for spec in args.workloads:
        name, kind, fopts = parse(spec)
        A, b, nd = hs.problems.make_problem(name, kind=kind, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        nd = hs.permuted(nd, hs.invperm(perm))
        F = hs.factor(A, nd, nd_loc, **fopts)
        n = A.shape[0]
        cplx = F.dtype.kind == "c"
        dt = np.complex128 if cplx else np.float64
        colptr, rowval, nz = _csc_fields(A, dt)
        fblk = L.hs_gmres_block_t_z if cplx else L.hs_gmres_block_t_d
        fone = L.hs_gmres_t_z if cplx else L.hs_gmres_t_d
        sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        explicit = (colptr.ctypes.data_as(pi), rowval.ctypes.data_as(pi), nz.ctypes.data_as(C.c_void_p))
        own = (None, None, None)
        ops = {0: A, 1: A.T.tocsr(), 2: A.conj().T.tocsr()}

        def timed(fn):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0

        for k in [int(v) for v in args.k.split(",")]:
            g = torch.Generator(device="cpu").manual_seed(k)
            Bh = torch.randn((k, n), dtype=torch.complex128 if cplx else torch.float64, generator=g)  # row r = column r, ld n
            for c in range(3, k, 4):
                Bh[c] = 0
                Bh[c, (c * 7919) % n] = 1
            dB = Bh.to(dev)
            dX, dY = torch.zeros_like(dB), torch.zeros_like(dB)
            hist = np.zeros((mi + 1, k), order="F")
            dev0 = None
            for trans in (0, 1, 2) if cplx else (0, 1):
                res = {}

                def run(a3, dOut, entry="block"):
                    it, cv = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int32)
                    if entry == "block":
                        hs._lib.check(fblk(F._h, trans, n, *a3, C.c_void_p(dB.data_ptr()), n, C.c_void_p(dOut.data_ptr()), n, k, 1, 0, args.reltol, 0.0, args.restart, mi,
                                           hist.ctypes.data_as(pf), it.ctypes.data_as(pi), cv.ctypes.data_as(C.POINTER(C.c_int)), sp))
                    else:
                        hs._lib.check(fone(F._h, trans, n, *a3, C.c_void_p(dB.data_ptr()), C.c_void_p(dOut.data_ptr()), 1, 0, args.reltol, 0.0, args.restart, mi,
                                           hist.ctypes.data_as(pf), it.ctypes.data_as(pi), cv.ctypes.data_as(C.POINTER(C.c_int)), sp))
                    res["it"], res["cv"] = it, cv

                for entry in ("block", "single") if k == 1 else ("block",):
                    timed(lambda: run(own, dX, entry)), timed(lambda: run(explicit, dY, entry))  # warm-up (work blocks of the handle, the CSR map)
                    to, te, do, de = [], [], [], []
                    for _ in range(args.n):
                        to.append(timed(lambda: run(own, dX, entry)))
                        do.append(hs.gmres_block_info()["seconds"] if entry == "block" else 0.0)
                        te.append(timed(lambda: run(explicit, dY, entry)))
                        de.append(hs.gmres_block_info()["seconds"] if entry == "block" else 0.0)
                    info = hs.gmres_block_info() if entry == "block" else None
                    Xh, Yh, Bn = dX.cpu().numpy(), dY.cpu().numpy(), Bh.numpy()
                    resid = float(max(np.linalg.norm(ops[trans] @ Xh[j] - Bn[j]) / np.linalg.norm(Bn[j]) for j in range(min(k, 8))))
                    d_own, d_exp = float(np.median(do)), float(np.median(de))
                    if entry == "block" and trans == 0:
                        dev0 = d_own
                    pair = [a - b_ for a, b_ in zip(do, de)]
                    print(json.dumps(dict(
                        workload=spec, entry=entry, n=n, nnz=int(A.nnz), dtype=F.dtype.name, reltol=args.reltol, restart=args.restart, maxiter=mi, k=k, trans=trans,
                        t_own=float(np.median(to)), t_own_all=to, t_own_device=d_own, t_own_device_all=do,
                        t_explicit=float(np.median(te)), t_explicit_all=te, t_explicit_device=d_exp, t_explicit_device_all=de,
                        host_saved=float(np.median(te)) - float(np.median(to)), device_own_minus_explicit=float(np.median(pair)),
                        device_pair_spread=float(max(pair) - min(pair)), device_over_trans0=(d_own / dev0) if (entry == "block" and dev0) else None,
                        iters=[int(v) for v in res["it"]], converged=int(res["cv"].sum()), info=info, same_bits=bool(np.array_equal(Xh, Yh)), worst_residual=resid)), flush=True)
            del dB, dX, dY
        F.free()
        hs.trim()


if __name__ == "__main__":
    main()
