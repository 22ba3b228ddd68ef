"""Time the block solve that serves HSS interior blocks (hs_ldiv_ulv_*) and the transposed ULV solve of the HSS module (hs_hss_ldiv_t).

    python tools/ldiv_ulv_time.py [--n N] [--k 32] [--loop-cols 4] [--hss-n 8192] [--out profiles/ldiv_ulv_time.txt]

Part 1: 32 columns at Helmholtz 64^3, swlevel 4 / 1e-4, with mf = 2 (D of every matrix-free front one HSS matrix) and mf = 3 (the 2 x 2
block form), trans = 0 / 1 / 2: one hs.ldiv_ulv call against the looped hs.ldiv of the same handle (trans = 0; measured with
--loop-cols columns and scaled to k, it is k single-vector solves by construction; the existing entry points have no transposed solve
for these handles to compare with).  Part 2: H.ldiv(B) against H.ldiv(B, trans="T") for a kernel matrix of order --hss-n, k columns.
Host wall times (the calls return when the result is complete), one warm-up, then the median of N.  One JSON line per measurement,
printed and appended to --out."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import hsamd


def median_time(f, n):
    f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def kernel_matrix(n):
    x = np.sort(np.random.default_rng(0).random(n))
    d = np.abs(x[:, None] - x[None, :])
    return 1.0 / (1.0 + 40.0 * d) + 0.3 * np.sin(3.0 * x)[:, None] * np.cos(2.0 * x)[None, :] + n * 0.05 * np.eye(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--loop-cols", type=int, default=4)
    ap.add_argument("--hss-n", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join("profiles", "ldiv_ulv_time.txt"))
    args = ap.parse_args()
    hs = hsamd.load()
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    A, b, nd = hs.problems.make_problem("helmholtz3d_64", rhs="randn")
    nd, nd_loc = hs.symfact(nd)
    perm = hs.postorder(nd)
    A = A[perm - 1][:, perm - 1].tocsc()
    nd = hs.permuted(nd, hs.invperm(perm))
    n, k = A.shape[0], args.k
    rng = np.random.default_rng(1)
    B = rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))
    for mf in (2, 3):
        F = hs.factor(A, nd, nd_loc, swlevel=4, swsize=8, atol=1e-4, rtol=1e-4, mf=mf)
        t_loop = median_time(lambda: hs.ldiv(F, B[:, : args.loop_cols]), args.n) * k / args.loop_cols
        for trans, Fop in ((0, F), (1, hs.transpose(F)), (2, hs.adjoint(F))):
            t = median_time(lambda: hs.ldiv_ulv(Fop, B), args.n)
            emit({"workload": "helmholtz3d_64:swlevel=4,tol=1e-4", "mf": mf, "trans": trans, "k": k, "ldiv_ulv_s": t, "looped_ldiv_s": t_loop,
                  "speedup_vs_looped_forward": t_loop / t})
        F.free()
    K = kernel_matrix(args.hss_n)
    H = hs.hss.compress(K, leafsize=128, atol=1e-6, rtol=1e-6, kest=64)
    X = rng.standard_normal((args.hss_n, k))
    t_n = median_time(lambda: H.ldiv(X), args.n)
    t_t = median_time(lambda: H.ldiv(X, trans="T"), args.n)
    emit({"hss_n": args.hss_n, "k": k, "rank": int(H.rank), "ldiv_s": t_n, "ldiv_T_s": t_t, "ratio_T_over_N": t_t / t_n})
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
