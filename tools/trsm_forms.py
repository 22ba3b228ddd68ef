#!/usr/bin/env python3
"""usage (GPU box): python3 tools/trsm_forms.py [--workload NAME] [--strip 0|1] [--out FILE]

The in-place TRSM products of ONE profiled factorization (bench.py --full: per-launch HIP events on the stream each launch runs on), per tree
level, per form and per stream.  The library writes one line per profiled launch to $HS_LAUNCH_LOG (Profiler::collect, csrc/hs_sched.h):
level, category, form, stream (0 main, 1 look-ahead side stream), fronts, least bytes, ms.  Forms: GemmOp::ainv 1, 3, 4, 7, 8; 9 = the strip
kernel (3 + 4 in one launch); 11 = trsm_small (64 / 128 rows).  Least bytes: X read once over the rows a form reads, the rows it stores
written once; the inverse block (L2-resident) is not counted.  Per level also: wall time (HS_VERBOSE_LEVELS), the main stream's plain
updates, and the difference -- what the main stream spends outside its GEMMs.  An event pair around a launch on the side stream also
measures the time the launch waits for a workgroup slot beside the bulk update.
--strip 0 runs the two half products (HS_TRSM_STRIP=0)."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = ["gemm", "panel", "laswp", "trsm", "assemble"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="poisson3d_128")
    ap.add_argument("--strip", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    log = tempfile.NamedTemporaryFile(prefix="hs_launch_", suffix=".log", delete=False).name
    env = dict(os.environ, HS_LAUNCH_LOG=log, HS_VERBOSE_LEVELS="1", HS_TRSM_STRIP=str(a.strip))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", a.workload, "--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline",
           "--no-oneshot", "--metric-workload", ""]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        return r.returncode
    # the LAST block of level lines belongs to the profiled step
    lev = collections.OrderedDict()
    for m in re.finditer(r"\[hs\] level\s+(\d+):\s+(\d+) fronts, max \(ni,nb\)=\((\d+),(\d+)\)\s+([0-9.]+) ms", r.stderr):
        lev[int(m.group(1))] = (int(m.group(2)), int(m.group(3)), int(m.group(4)), float(m.group(5)))
    rows = collections.defaultdict(lambda: [0, 0.0, 0.0])  # (level, cat, form, side) -> launches, ms, bytes
    for line in open(log):
        t, c, f, s, nb, by, ms = line.split()
        k = (int(t), int(c), int(f), int(s))
        rows[k][0] += 1
        rows[k][1] += float(ms)
        rows[k][2] += float(by)
    os.unlink(log)
    out = []
    out.append("# %s   HS_TRSM_STRIP=%d" % (" ".join(["python3", "tools/trsm_forms.py", "--workload", a.workload, "--strip", str(a.strip)]), a.strip))
    out.append("# bench line: " + r.stdout.strip().splitlines()[-1][:400])
    tot = collections.defaultdict(lambda: [0, 0.0, 0.0])
    wall_all = gemm_main_all = 0.0
    for t in sorted(lev, reverse=True):
        nf, mni, mnb, wall = lev[t]
        gm = sum(v[1] for k, v in rows.items() if k[0] == t and k[1] == 0 and k[3] == 0)
        wall_all += wall
        gemm_main_all += gm
        out.append("level %2d: %4d fronts, max (ni, nb) = (%d, %d): wall %9.3f ms, main-stream updates %9.3f ms, wall - updates %8.3f ms" % (t, nf, mni, mnb, wall, gm, wall - gm))
        for k in sorted(k for k in rows if k[0] == t and k[1] != 0):
            n, ms, by = rows[k]
            what = CATS[k[1]] + (" form %2d" % k[2] if k[1] == 3 else "        ")
            gbs = "%8.1f GB/s" % (by / (ms * 1e-3) / 1e9) if by > 0 and ms > 0 else ""
            out.append("      %-14s %-4s %5d launches %10.1f us  avg %8.1f us  %10.1f MB %s" % (what, "side" if k[3] else "main", n, ms * 1e3, ms * 1e3 / n, by / 1e6, gbs))
            if k[1] == 3:
                x = tot[(k[2], k[3])]
                x[0] += n; x[1] += ms; x[2] += by
    out.append("all levels: wall %.3f ms, main-stream updates %.3f ms, wall - updates %.3f ms" % (wall_all, gemm_main_all, wall_all - gemm_main_all))
    for (f, s), (n, ms, by) in sorted(tot.items()):
        out.append("      trsm form %2d %-4s %5d launches %10.1f us  avg %8.1f us  %10.1f MB %8.1f GB/s" % (f, "side" if s else "main", n, ms * 1e3, ms * 1e3 / max(n, 1), by / 1e6, by / max(ms * 1e-3, 1e-30) / 1e9))
    txt = "\n".join(out) + "\n"
    sys.stdout.write(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt)
    return 0


if __name__ == "__main__":
    sys.exit(main())
