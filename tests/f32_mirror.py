"""The demotion rule of hs_f32_create (csrc/kernels_f32.hip) in NumPy: every real scalar (real and imaginary parts separately) is rounded to
Float32, to nearest with ties to even; an element that is finite in Float64 and +-Inf in Float32 counts as an overflow, a nonzero element
that becomes zero or a Float32 subnormal as flushed."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)  # the smallest normal


def _reals(x):
    x = np.asarray(x)
    return x.view(np.float64) if x.dtype.kind == "c" else x.astype(np.float64, copy=False)


def demote(x):
    """``(x rounded through Float32, as Float64 / ComplexF64; overflow count; flush count)``"""
    x = np.ascontiguousarray(x)
    r = _reals(x)
    with np.errstate(over="ignore", under="ignore"):
        f = r.astype(np.float32)
    over = int(np.count_nonzero(np.isfinite(r) & np.isinf(f)))
    flush = int(np.count_nonzero((r != 0.0) & (np.abs(f) < np.float32(FLT_MIN))))
    w = f.astype(np.float64)
    return (w.view(np.complex128) if x.dtype.kind == "c" else w).reshape(x.shape), over, flush


def rounded(x):
    return demote(x)[0]
