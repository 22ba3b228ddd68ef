"""Schur-update micro-benchmark (not a test): one launch SB -= LF[ni.., :] * UR over the fronts of a tree level through hsk_gemm_schur_d, with
the direct-to-LDS kernels off (register-staged gemm_op_kernel) and on (gemm_op_lds_kernel / gemm_op_lds_edge_kernel), side by side.
usage: tools/bench_gemm_schur.py [WORKLOAD [repeat]] -- default poisson3d_128: the (ni, nb) of every level with 2 ... 256 fronts are taken
from the elimination tree itself; the operands hold one finite value (no host data: a level is tens of GB).  HS_BENCH_LIB=path loads
another build of the library."""
import collections, ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hsamd
hs = hsamd.load()
if os.environ.get("HS_BENCH_LIB"): hs._lib.LIB_PATH = os.environ["HS_BENCH_LIB"]
L = hs._lib.lib()
pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
workload = sys.argv[1] if len(sys.argv) > 1 else "poisson3d_128"
rep = int(sys.argv[2]) if len(sys.argv) > 2 else 3
_, _, nd = hs.problems.make_problem(workload, rhs="randn")
nd, _ = hs.symfact(nd)
levels, stack = collections.defaultdict(list), [(nd, 0)]
while stack:
    n, d = stack.pop()
    levels[d].append((len(n.int), len(n.bnd)))
    stack += [(c, d + 1) for c in (n.left, n.right) if c is not None]
for d in sorted(levels):
    fronts = [(ni, nb) for ni, nb in levels[d] if ni > 0 and nb > 0]
    if not 2 <= len(fronts) <= 256: continue
    ni, nb = (np.array(x, dtype=np.int64) for x in zip(*fronts))
    out, kern = [], ""
    for on in (0, 1):
        prev = L.hsk_gemm_lds_enable(on)
        ms, r_lds, r_edge = C.c_double(0), C.c_int64(0), C.c_int64(0)
        hs._lib.check(L.hsk_gemm_schur_d(len(fronts), pi(ni), pi(nb), None, None, None, 0, C.byref(r_lds), C.byref(r_edge), rep, C.byref(ms)))
        L.hsk_gemm_lds_enable(prev)
        assert (r_lds.value + r_edge.value) == on, (on, r_lds.value, r_edge.value)
        if on: kern = "lds" if r_lds.value else "edge"
        out.append(ms.value)
    fl = float(np.sum(2.0 * nb * nb * ni))
    c = collections.Counter(int(x) for x in ni).most_common(3)
    print(f"fronts {len(fronts):4d}  ni {'/'.join(str(k) for k, _ in c):>16s}  nb <= {int(nb.max()):6d}  register-staged {out[0]:9.3f} ms {fl/out[0]/1e9:6.2f} TFLOP/s   "
          f"direct-to-LDS ({kern:4s}) {out[1]:9.3f} ms {fl/out[1]/1e9:6.2f} TFLOP/s   ratio {out[0]/out[1]:.3f}", flush=True)
