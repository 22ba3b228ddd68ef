"""Time the numeric factorization with SolverOptions.symmetric off and on, in one process.

    python tools/sym_time.py [--n 5] [--out FILE] [WORKLOAD ...]

WORKLOAD is NAME[:swlevel=L,tol=T] with NAME a problems.NAMED entry (default: poisson3d_64, poisson3d_128, helmholtz3d_64 exact and
helmholtz3d_64:swlevel=4,tol=1e-4).  Per workload two handles are analysed once (option off, option on; dist.StagedSolver, as bench.py
does); then, after one warm-up of each, N alternating numeric factorizations on the same handles (one setting after the
other when the two factor arenas do not fit side by side: "alternating": false).  Reported: medians of hs_stats.t_total,
gemm_flops and bytes_factors, hs_sym_info, the relative difference of the two solutions, and the per-level wall times the library prints
under HS_VERBOSE_LEVELS=1 (medians per level, option off and on side by side).  One JSON line per workload, a table per workload on
stdout; --out appends both to FILE."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile

os.environ["HS_VERBOSE_LEVELS"] = "1"  # read by the library when the first level is factored
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hsamd
from ldiv_t_time import parse

LEVEL = re.compile(r"\[hs\] level\s+(\d+):\s+(\d+) fronts, max \(ni,nb\)=\((\d+),(\d+)\)\s+([0-9.]+) ms")


class capture_stderr:
    """The library prints the level times with fprintf(stderr): collect file descriptor 2 while the block runs."""

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5, help="timed factorizations per setting (after one warm-up)")
    ap.add_argument("--out", default=None)
    ap.add_argument("workloads", nargs="*", default=["poisson3d_64", "poisson3d_128", "helmholtz3d_64", "helmholtz3d_64:swlevel=4,tol=1e-4"])
    args = ap.parse_args()
    hs = hsamd.load()
    hsdist = hs.dist
    L = hs._lib.lib()

    def emit(text):
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")

    for spec in args.workloads:
        name, kw = parse(spec)
        A, b, nd = hs.problems.make_problem(name, rhs="randn")
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A[perm - 1][:, perm - 1].tocsc()
        A.sort_indices()
        nd = hs.permuted(nd, hs.invperm(perm))
        b = b[perm - 1]
        dev = torch.device("cuda:0")
        def numeric(St):
            with capture_stderr() as cap:
                St.numeric()
                torch.cuda.synchronize(dev)
            levels = {int(m.group(1)): (int(m.group(2)), int(m.group(3)), int(m.group(4)), float(m.group(5))) for m in LEVEL.finditer(cap.text)}
            return St.stats(), levels

        def setup(sym):  # analysis (hs_analyze) and one warm-up factorization
            with capture_stderr():
                St = hsdist.StagedSolver(A, nd, nd_loc, device=dev, symmetric=sym, **kw)
                St.numeric()
                torch.cuda.synchronize(dev)
            return St

        def finish(St, sym):
            xs[sym] = torch.from_numpy(np.ascontiguousarray(b)).to(dev)
            St.solve(xs[sym])
            if sym:
                hs._lib.check(L.hs_sym_info(St.backend._h, out4))

        runs, xs, out4 = {False: [], True: []}, {}, (C.c_int64 * 4)()
        S = {}
        try:
            for sym in (False, True):
                S[sym] = setup(sym)
            alternating = True
        except MemoryError:  # the two factor arenas do not fit side by side: one setting after the other
            S.clear()
            hs.trim()
            alternating = False
        if alternating:
            for _ in range(args.n):
                for sym in (False, True):
                    runs[sym].append(numeric(S[sym]))
            for sym in (False, True):
                finish(S[sym], sym)
            S.clear()
        else:
            for sym in (False, True):
                St = setup(sym)
                for _ in range(args.n):
                    runs[sym].append(numeric(St))
                finish(St, sym)
                del St
                hs.trim()
        med = lambda sym, key: float(np.median([st[key] for st, _ in runs[sym]]))  # noqa: E731
        info = dict(option=bool(out4[0]), fronts_lower=int(out4[1]), fronts_general=int(out4[2]))
        out = dict(workload=spec, n=A.shape[0], dtype=str(A.dtype), runs=args.n, alternating=alternating, sym_info=info,
                   solution_rel_diff=float((torch.linalg.vector_norm(xs[True] - xs[False]) / torch.linalg.vector_norm(xs[False])).item()))
        for key in ("t_total", "gemm_flops", "bytes_factors"):
            out[key + "_off"], out[key + "_on"] = med(False, key), med(True, key)
        out["t_total_on_over_off"] = out["t_total_on"] / out["t_total_off"]
        out["gemm_flops_on_over_off"] = out["gemm_flops_on"] / out["gemm_flops_off"]
        out["t_total_all_off"] = [st["t_total"] for st, _ in runs[False]]
        out["t_total_all_on"] = [st["t_total"] for st, _ in runs[True]]
        emit(json.dumps(out))
        emit(f"# {spec}: t_total off {out['t_total_off']:.4f} s  on {out['t_total_on']:.4f} s  ({out['t_total_on_over_off']:.3f});  gemm_flops on / off "
             f"{out['gemm_flops_on_over_off']:.3f};  fronts on their lower triangle {info['fronts_lower']}, as before {info['fronts_general']}")
        emit("# level  fronts  max(ni,nb)        off ms      on ms   on/off")
        for lv in sorted(runs[False][0][1], reverse=True):
            nf, ni, nb_, _ = runs[False][0][1][lv]
            t0 = float(np.median([lv_[lv][3] for _, lv_ in runs[False] if lv in lv_]))
            t1 = float(np.median([lv_[lv][3] for _, lv_ in runs[True] if lv in lv_]))
            emit(f"# {lv:5d}  {nf:6d}  ({ni:5d},{nb_:5d})  {t0:10.3f} {t1:10.3f}   {t1 / t0 if t0 > 0 else float('nan'):6.3f}")
        del xs
        hs.trim()


if __name__ == "__main__":
    main()
