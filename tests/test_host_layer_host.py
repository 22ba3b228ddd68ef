"""The shared host layer (csrc/hs_host.h): every module throws an int through HS_FAIL and its entry points return it through HS_GUARD.
One argument refusal per module whose entry layer had no host-side case that pins the code AND the message; no GPU is needed (the
refusals come before any device work, and the HSS module's first refusal without a device is the missing device itself)."""
import ctypes as C

from conftest import have_gpu


def _last(L):
    return L.hs_last_error().decode(), L.hs_last_error_info()


def test_symbolic_refusal_travels_as_code_and_message(hs):
    L, lib = hs._lib.lib(), hs._lib
    one = (C.c_int64 * 1)(7)  # a father that is not -1: a tree without a root
    out = C.c_void_p()
    st = L.hs_symbolic_from_elimtree(1, one, one, one, one, one, 1, one, one, 1, C.byref(out))
    assert st == lib.HS_ERR_ARGUMENT and not out.value
    assert _last(L) == ("ArgumentError: found either less than or more than one root.", 0)


def test_comm_refusal_travels_as_code_and_message(hs):
    L, lib = hs._lib.lib(), hs._lib
    fn = lib.HS_TRANSFER_FN(lambda *a: 0)
    out = C.c_void_p(1)
    st = L.hs_comm_create_host(fn, None, 2, 2, C.byref(out))
    assert st == lib.HS_ERR_ARGUMENT and not out.value
    assert _last(L) == ("ArgumentError: rank 2 of 2", 0)
    assert L.hs_comm_create_host(fn, None, 0, 2, None) == lib.HS_ERR_ARGUMENT
    assert _last(L) == ("ArgumentError: null argument", 0)


def test_testhook_refusal_travels_as_code_and_message(hs):
    L, lib = hs._lib.lib(), hs._lib
    a = (C.c_double * 4)()
    st = L.hsk_mod_inner_d(2, 0, 1, a, 2, a, 2, 0, a, 1)  # k = 0
    assert st == lib.HS_ERR_ARGUMENT
    assert _last(L) == ("hsk_mod_inner: n >= 1, k in 1..256, m in 1..64, leading dimensions and non-null arrays required", 0)


def test_gmres_block_refusal_travels_as_code_and_message(hs):
    L, lib = hs._lib.lib(), hs._lib
    colptr, rowval = (C.c_int64 * 2)(1, 2), (C.c_int64 * 1)(1)
    nz, b, x = (C.c_double * 1)(1.0), (C.c_double * 1)(1.0), (C.c_double * 1)()
    iters, conv = (C.c_int64 * 1)(), (C.c_int * 1)()
    st = L.hs_gmres_block_d(None, 1, colptr, rowval, nz, b, 1, x, 1, 1, 2, 0, 1e-9, 0.0, 0, -1, None, iters, conv, None)  # where = 2
    assert st == lib.HS_ERR_ARGUMENT
    assert _last(L) == ("ArgumentError: hs_gmres_block: where = 2 (0: host pointers, 1: device pointers)", 2)


def test_hss_refusal_travels_as_code_and_message(hs):
    L, lib = hs._lib.lib(), hs._lib
    out = C.c_void_p(1)
    st = L.hs_hss_compress_d(0, None, 0, 0, None, C.byref(out))
    got = (st, _last(L))  # (before have_gpu() asks the library for a device, which sets its own message without one)
    assert not out.value
    if have_gpu():
        assert got == (lib.HS_ERR_ARGUMENT, ("ArgumentError: hs_hss_compress needs n > 0, lda >= n and a matrix", 0))
    else:
        assert got == (lib.HS_ERR_DEVICE, ("no HIP device available (the HSS module has no CPU fallback)", 0))
