"""Cost and benefit of SolverOptions.equilibrate, in one process.

    python tools/equil_time.py [--n 5] [--out FILE] [--off-only] [--root DIR] [--no-benefit] [WORKLOAD ...]

Cost.  WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_128 exact and
helmholtz3d_64:swlevel=4,tol=1e-4).  Per workload and setting (option off, option on) one handle is analysed (dist.StagedSolver, as
bench.py does) and, after one warm-up, factored N times; then N 32-column solves with transpose(F) on device blocks
(hs_ldiv_block_dev_t_*).  Reported: medians of the wall time of a numeric factorization (hs_numeric_begin .. hs_numeric_end, the
scaling included; hs_stats.t_total starts after hs_numeric_begin and is printed next to it), of the device time of the solve, and
hs_equil_info.  --off-only times the option off alone and never names the option; with --root DIR the package is imported from another
checkout of the project: together they time the parent commit with the same script.

Benefit.  convdiff_helmholtz 24^3 as D1 A D2 with seeded random power-of-two diagonals (exponents in +-40), exact and at swlevel 2 /
1e-4, without and with the option: levels redone with tournament pivoting (the library's verbose line; a handle redoes at most one
level, then pivots by tournament for good), hs.maxrank, and berr of one plain solve (hs.ldiv_refine, itmax=0) for a right-hand side
b = B x with x standard normal.  One JSON line per measurement; --out appends them to FILE."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

NCOL = 32


class capture_stderr:
    """The library prints with fprintf(stderr): collect file descriptor 2 while the block runs."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


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


def ordered(hs, A, b, nd):
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    A = A[perm - 1][:, perm - 1].tocsc()
    A.sort_indices()
    return A, b[perm - 1], hs.permuted(nd, hs.invperm(perm)), nd_loc


def scaled(A, seed, span):
    """D1 A D2 with random power-of-two diagonals, entry by entry with ldexp (exact)."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    n = A.shape[0]
    e1, e2 = rng.integers(-span, span + 1, n), rng.integers(-span, span + 1, n)
    s = (e1[A.indices] + np.repeat(e2, np.diff(A.indptr))).astype(np.int32)
    d = A.data
    v = np.ldexp(d.real, s) + 1j * np.ldexp(d.imag, s) if np.iscomplexobj(d) else np.ldexp(d, s)
    return sp.csc_matrix((v, A.indices.copy(), A.indptr.copy()), shape=A.shape)


def cost(hs, torch, spec, settings, n, emit):
    name, kw = parse(spec)
    A, b, nd, nd_loc = ordered(hs, *hs.problems.make_problem(name, rhs="randn"))
    dev = torch.device("cuda:0")
    L = hs._lib.lib()
    N = A.shape[0]
    cplx = np.iscomplexobj(A.data)
    for on in settings:
        opt = {} if on is None else dict(equilibrate=on)
        St = hs.dist.StagedSolver(A, nd, nd_loc, device=dev, **kw, **opt)
        wall, ttot = [], []
        for it in range(n + 1):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            St.numeric()
            torch.cuda.synchronize(dev)
            if it:  # the first one warms up
                wall.append(time.perf_counter() - t0)
                ttot.append(St.stats()["t_total"])
        rng = np.random.default_rng(1)
        B = rng.standard_normal((NCOL, N)) + (1j * rng.standard_normal((NCOL, N)) if cplx else 0.0)
        dB = torch.from_numpy(np.ascontiguousarray(B)).to(dev)  # NCOL x N row-major == N x NCOL column-major
        dC = torch.empty_like(dB)
        fn = L.hs_ldiv_block_dev_t_z if cplx else L.hs_ldiv_block_dev_t_d
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        solve = []
        for it in range(n + 1):
            ev[0].record()
            hs._lib.check(fn(St.backend._h, 1, dC.data_ptr(), N, dB.data_ptr(), N, N, NCOL, torch.cuda.current_stream().cuda_stream))
            ev[1].record()
            torch.cuda.synchronize(dev)
            if it:
                solve.append(ev[0].elapsed_time(ev[1]) * 1e-3)
        out = dict(kind="cost", workload=spec, n=N, dtype=str(A.dtype), runs=n, equilibrate=on, numeric_wall_s=float(np.median(wall)),
                   t_total_s=float(np.median(ttot)), solve32_t_s=float(np.median(solve)), numeric_wall_all=wall, solve32_all=solve)
        if on is not None:
            out6 = (C.c_int64 * 6)()
            hs._lib.check(L.hs_equil_info(St.backend._h, out6))
            out["equil_info"] = list(out6)
        emit(json.dumps(out))
        del St, dB, dC
        hs.trim()


def benefit(hs, emit):
    A, b, nd, nd_loc = ordered(hs, *hs.problems.make_problem((24, 24, 24), kind="convdiff_helmholtz", rhs="randn"))
    B = scaled(A, 77, 40)
    rng = np.random.default_rng(2)
    x = rng.standard_normal(A.shape[0]) + 1j * rng.standard_normal(A.shape[0])
    rhs = B @ x
    for label, M in (("A (well scaled)", A), ("D1 A D2, exponents +-40", B)):
        for kw in (dict(swlevel=0), dict(swlevel=2, atol=1e-4, rtol=1e-4)):
            for on in (False, True):
                r = rhs if M is B else A @ x
                with capture_stderr() as cap:
                    try:
                        F = hs.factor(M, nd, nd_loc, verbose=True, equilibrate=on, **kw)
                    except Exception as e:  # noqa: BLE001
                        F, err = None, f"{type(e).__name__}: {e}"
                out = dict(kind="benefit", matrix=label, equilibrate=on, **kw)
                if F is None:
                    out["error"] = err
                else:
                    xs, berr, _, _ = hs.ldiv_refine(F, r, itmax=0, ferr=False)
                    ref = x
                    out.update(levels_redone=cap.text.count("redoing the level with tournament pivoting"), maxrank=hs.maxrank(F), berr=float(berr),
                               relerr_vs_x=float(np.linalg.norm(xs - ref) / np.linalg.norm(ref)), equil_info=hs.equil_info(F))
                    F.free()
                emit(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="timed runs per setting (after one warm-up)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--off-only", action="store_true", help="time the option off alone and never name it (a checkout without the option)")
    ap.add_argument("--root", default=None, help="import the package from this checkout of the project instead of the script's own")
    ap.add_argument("--no-benefit", action="store_true")
    ap.add_argument("workloads", nargs="*", default=["poisson3d_128", "helmholtz3d_64:swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    import hsamd

    hs = hsamd.load()

    def emit(text):
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")

    emit(f"# equil_time: medians of {args.n}; root {'(own)' if not args.root else 'another checkout'}; off-only {args.off_only}")
    for spec in args.workloads:
        cost(hs, torch, spec, (None,) if args.off_only else (False, True), args.n, emit)
    if not args.off_only and not args.no_benefit:
        benefit(hs, emit)


if __name__ == "__main__":
    main()
