"""Time the Schur-complement mode: hs_interface_matrix_* next to the project's FP64 GEMM, and the three phases next to one block solve.

    python tools/interface_time.py [--n N] [--cols K] [--out FILE] [CASE ...]

CASE is kind:size (default: poisson:64 helmholtz:64; poisson:128 is the third case of DESIGN.md section 4k), a size^3 grid factored exactly
(swlevel = 0) on a tree from problems.graph_nested_dissection whose interface is the interior grid plane x = size / 2 (nb = size^2).  Per
case, after one warm-up, the median of N calls:
  * hs.schur_complement(F, device=True): seconds and executed flops from hs_interface_info, TF/s; beside it an nb x nb x nb product of the
    project's GEMM kernel (hsk_gemm_*, ms per launch of `N` back-to-back launches) in the same process, and the ratio of the two times;
  * condense, interface_solve, expand on a device block of K columns (seconds from hs_interface_info) and one hs.ldiv_block_t of the same
    block (hs_ldiv_block_info), and (condense + solve + expand) / block solve.
One JSON line per case on stdout and appended to FILE (default profiles/interface_time.txt)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import hsamd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3, help="timed calls (after one warm-up)")
    ap.add_argument("--cols", type=int, default=32, help="columns of the block the phases run on")
    ap.add_argument("--nmax", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interface_time.txt"))
    ap.add_argument("cases", nargs="*", default=["poisson:64", "helmholtz:64"])
    args = ap.parse_args()
    import torch

    hs = hsamd.load()
    L = hs._lib.lib()
    for case in args.cases:
        kind, size = case.split(":")
        size = int(size)
        shape = (size, size, size)
        t0 = time.perf_counter()
        A0 = hs.problems.grid_matrix(shape, kind).tocsc()
        n = A0.shape[0]
        plane = np.arange(n, dtype=np.int64).reshape(shape, order="F")[size // 2].reshape(-1)
        nd = hs.problems.graph_nested_dissection(A0, args.nmax, interface=plane)
        nd, nd_loc = hs.symfact(nd)
        perm = hs.postorder(nd)
        A = A0[perm - 1][:, perm - 1].tocsc()
        nd = hs.permuted(nd, hs.invperm(perm))
        t_tree = time.perf_counter() - t0
        F = hs.factor(A, nd, nd_loc, swlevel=0)
        st = F.stats()
        cplx = F.dtype.kind == "c"
        nb = len(hs.interface_indices(F))
        mat_s, flops = [], 0.0
        for it in range(args.n + 1):
            S = hs.schur_complement(F, device=True)
            info = hs.interface_info(F)
            if it:
                mat_s.append(info["matrix_seconds"])
            flops = info["matrix_flops"]
        # the project's GEMM on an nb x nb x nb product in the same process
        rng = np.random.default_rng(0)
        mk = lambda: np.asfortranarray(rng.standard_normal((nb, nb)) + (1j * rng.standard_normal((nb, nb)) if cplx else 0))  # noqa: E731
        Ga, Gb, Gc = mk(), mk(), mk()
        ms = C.c_double(0.0)
        pf = hs._lib.p_f64
        hs._lib.check((L.hsk_gemm_z if cplx else L.hsk_gemm_d)(nb, nb, nb, Ga.ctypes.data_as(pf), nb, Gb.ctypes.data_as(pf), nb, Gc.ctypes.data_as(pf), nb, 1, args.n, C.byref(ms)))
        gemm_s = ms.value * 1e-3
        gemm_flops = 2.0 * nb**3 * (4 if cplx else 1)
        # the three phases against one block solve of the same block
        B = np.asfortranarray(rng.standard_normal((n, args.cols)) + (1j * rng.standard_normal((n, args.cols)) if cplx else 0))
        dB = torch.from_numpy(B.T.copy()).to("cuda")  # row c = column c of the block: its transpose is column-major n x cols
        ph = {"condense": [], "solve": [], "expand": []}
        blk = []
        for it in range(args.n + 1):
            ref = hs.ldiv_block_t(F, B)
            if it:
                blk.append(hs.ldiv_block_info(F)["seconds"])
            d = dB.clone().t()
            for name, fn in (("condense", hs.condense), ("solve", hs.interface_solve), ("expand", hs.expand)):
                fn(F, d)
                sec = hs.interface_info(F)[name + "_seconds"]
                if it:
                    ph[name].append(sec)
            same = bool(np.array_equal(d.cpu().numpy(), ref))
        med = lambda v: float(np.median(v))  # noqa: E731
        three = med(ph["condense"]) + med(ph["solve"]) + med(ph["expand"])
        line = json.dumps(dict(
            case=case, n=n, nb=nb, dtype=F.dtype.name, tree_seconds=t_tree, factor_seconds=st["t_total"],
            matrix_seconds=med(mat_s), matrix_seconds_all=mat_s, matrix_flops=flops, matrix_tflops=flops / med(mat_s) / 1e12,
            matrix_flops_over_full=flops / gemm_flops, gemm_seconds=gemm_s, gemm_tflops=gemm_flops / gemm_s / 1e12, matrix_over_gemm_seconds=med(mat_s) / gemm_s,
            cols=args.cols, condense_seconds=med(ph["condense"]), solve_seconds=med(ph["solve"]), expand_seconds=med(ph["expand"]),
            block_solve_seconds=med(blk), phases_over_block_solve=three / med(blk), phases_bits_equal=same))
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del S
        F.free()


if __name__ == "__main__":
    main()
