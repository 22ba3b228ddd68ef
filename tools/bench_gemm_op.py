"""Plain-update micro-benchmark (not a test): TFLOP/s of one Sched::gemm launch through hsk_gemm_op_d, register-staged gemm_op_kernel
(HS_GEMM_LDS off) and gemm_op_lds_kernel (on) side by side.  usage: tools/bench_gemm_op.py [M N K [repeat]] -- default: the table of DESIGN.md
section 4 (K = 32 ... 4096 on 16384^2, then 8192^3).  HS_BENCH_LIB=path loads another build of the library."""
import ctypes as C, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hsamd
hs = hsamd.load()
if os.environ.get("HS_BENCH_LIB"): hs._lib.LIB_PATH = os.environ["HS_BENCH_LIB"]
L = hs._lib.lib()
pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
rng = np.random.default_rng(0)
pool = {}
def rand(n):  # one pool of normals, re-used by every shape (generating 2 GiB per shape would dominate the run)
    if pool.get("n", 0) < n: pool["n"], pool["x"] = n, rng.standard_normal(n)
    return pool["x"][:n]
def run(M, N, K, rep=5):
    A, B, Cm = rand(M * K), rand(K * N), rand(M * N).copy()
    out = []
    for on in (0, 1):
        prev = L.hsk_gemm_lds_enable(on)
        ms, routed = C.c_double(0), C.c_int64(0)
        Mv, Nv = np.array([M], dtype=np.int64), np.array([N], dtype=np.int64)
        hs._lib.check(L.hsk_gemm_op_d(1, pi(Mv), pi(Nv), K, 0, 0, pd(A), pd(B), pd(Cm), C.byref(routed), rep, C.byref(ms)))
        L.hsk_gemm_lds_enable(prev)
        assert routed.value == on, (on, routed.value)
        out.append(ms.value)
    fl = 2.0 * M * N * K
    print(f"M={M:6d} N={N:6d} K={K:6d}  register-staged {out[0]:9.3f} ms {fl/out[0]/1e9:7.2f} TFLOP/s   direct-to-LDS {out[1]:9.3f} ms {fl/out[1]/1e9:7.2f} TFLOP/s   ratio {out[0]/out[1]:.3f}", flush=True)
if len(sys.argv) >= 4:
    run(*[int(a) for a in sys.argv[1:4]], rep=int(sys.argv[4]) if len(sys.argv) > 4 else 5)
else:
    for K in (32, 64, 128, 256, 512, 1024, 4096): run(16384, 16384, K)
    run(8192, 8192, 8192)
