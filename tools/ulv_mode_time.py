"""Time the lockstep drivers and hs.logabsdet on handles with HSS interior blocks, served through hs_ulv_mode (DESIGN.md 4d'-m).

    python tools/ulv_mode_time.py [--n 5] [--k 32] [--loop-cols K] [--out profiles/ulv_mode_time.txt]

Helmholtz 64^3, swlevel 4 / 1e-4, with mf = 2 (D of every matrix-free front one HSS matrix) and mf = 3 (the 2 x 2 block form), k = 32
sources, on one handle and in one process:

  * GMRES(30) to 1e-8: one mode-1 hs.gmres_block call against the looped hs.gmres of mode 0 (the only Krylov path such a handle had),
  * hs.ldiv_refine_block in mode 1 with and without ferr against the looped hs.ldiv_refine of mode 0 (trans = 0, no ferr: what it serves),
  * hs.logabsdet in mode 1.

The looped calls run over all k columns by default; --loop-cols C < k measures C columns and scales to k (they are k single-column calls
by construction), and every record says which it was ("loop_cols").  One warm-up, then the median of N.  Block calls report the
library's own event pair (gmres_block_info / ldiv_refine_block_info "seconds") next to the host wall time; the looped calls and hs.logabsdet are blocking calls timed on the host.  One JSON line per measurement, printed and
appended to --out."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import hsamd


def median_of(f, n):
    """f() -> (wall seconds measured inside, device seconds or None); one warm-up, medians of n."""
    f()
    w, d = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        dev = f()
        w.append(time.perf_counter() - t0)
        d.append(dev)
    return float(np.median(w)), (float(np.median(d)) if d[0] is not None else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--loop-cols", type=int, default=0, help="columns the looped calls are measured on (0: all k; fewer: scaled to k)")
    ap.add_argument("--out", default=os.path.join("profiles", "ulv_mode_time.txt"))
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
    lc = args.loop_cols if 0 < args.loop_cols < k else k
    rng = np.random.default_rng(1)
    B = rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))
    gm = dict(reltol=1e-8, restart=30, maxiter=30)
    wl = "helmholtz3d_64:swlevel=4,tol=1e-4"
    for mf in (2, 3):
        F = hs.factor(A, nd, nd_loc, swlevel=4, swsize=8, atol=1e-4, rtol=1e-4, mf=mf)
        base = {"workload": wl, "mf": mf, "k": k, "loop_cols": lc}

        # ---- GMRES
        its_loop = []

        def looped_gmres():
            its_loop.clear()
            for c in range(lc):
                _, ch = hs.gmres(A, B[:, c], Pr=F, log=True, **gm)
                its_loop.append(ch["iters"])

        t_loop, _ = median_of(looped_gmres, args.n)
        t_loop *= k / lc
        hs.ulv_mode(F, True)
        its_blk = []

        def block_gmres():
            _, chs = hs.gmres_block(A, B, Pr=F, log=True, **gm)
            its_blk[:] = [c["iters"] for c in chs]
            return hs.gmres_block_info()["seconds"]

        t_blk, d_blk = median_of(block_gmres, args.n)
        emit(dict(base, what="gmres", block_wall_s=t_blk, block_device_s=d_blk, looped_wall_s=t_loop, speedup_vs_looped=t_loop / t_blk,
                  block_iters=[min(its_blk), max(its_blk)], looped_iters=[min(its_loop), max(its_loop)]))

        # ---- refined solves
        hs.ulv_mode(F, False)
        t_rl, _ = median_of(lambda: hs.ldiv_refine(F, B[:, :lc], itmax=5, ferr=False) and None, args.n)
        t_rl *= k / lc
        hs.ulv_mode(F, True)
        for ferr in (False, True):
            def block_refine():
                hs.ldiv_refine_block(F, B, itmax=5, ferr=ferr)
                return hs.ldiv_refine_block_info()["seconds"]

            t_rb, d_rb = median_of(block_refine, args.n)
            emit(dict(base, what="ldiv_refine", ferr=ferr, block_wall_s=t_rb, block_device_s=d_rb, looped_wall_s_no_ferr=t_rl, speedup_vs_looped_no_ferr=t_rl / t_rb))

        # ---- determinant
        t_det, _ = median_of(lambda: hs.logabsdet(F) and None, args.n)
        la, sign = hs.logabsdet(F)
        emit(dict(base, what="logabsdet", wall_s=t_det, logabs=la, sign=[sign.real, sign.imag]))
        hs.ulv_mode(F, False)
        F.free()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
