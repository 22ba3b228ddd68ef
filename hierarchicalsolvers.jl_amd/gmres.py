"""Right-preconditioned restarted GMRES with every vector resident on the GPU.

The call the reference's scenario makes (``test/rungmres.jl:47-48``)::

    x, ch = gmres(A, b; Pr=F, reltol=1e-9, restart=30, log=true, maxiter=30)

``IterativeSolvers.gmres`` (0.9.0, not part of the reference tree) uses the preconditioner only through ``ldiv!``.  ``gmres`` here is
``hs_gmres_{d,z}`` of the C ABI (include/hs_solver.h, csrc/hs_gmres_block.hip: the lockstep driver on one column): hand-written CSR product,
Gram-Schmidt and Givens kernels, the preconditioner applied through ``hs_ldiv_dev_*`` on device pointers -- what a Julia host calls instead
of ``IterativeSolvers.gmres``.
``trans="T"`` / ``"C"`` (or ``Pr=transpose(F)`` / ``adjoint(F)``) solve ``transpose(A) x = b`` / ``A' x = b`` with the same factorization
(``hs_gmres_t_*``, ``hs_gmres_block_t_*``); ``A=None`` takes the matrix the handle already holds on the device.
(An independent torch restatement of the same iteration lives under tests/gmres_mirror.py: test infrastructure, not product.)
Parity unpinned: IterativeSolvers is absent.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import _lib

__all__ = ["gmres", "gmres_native", "gmres_device", "gmres_block", "gmres_block_info"]


def _csc_fields(A, dtype):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return (np.ascontiguousarray(A.indptr, dtype=np.int64) + 1, np.ascontiguousarray(A.indices, dtype=np.int64) + 1,
            np.ascontiguousarray(A.data, dtype=dtype))


_TRANS = {"N": 0, "T": 1, "C": 2}


def _op_of(Pr, trans):
    """``(FactorNode or None, trans code)`` of the ``Pr`` / ``trans`` pair: ``Pr=transpose(F)`` / ``adjoint(F)`` is shorthand for the matching
    ``trans``; a pair that names two different operators raises ``ValueError``."""
    from .solver import TransposedFactor

    if trans is not None and trans not in _TRANS:
        raise ValueError(f"trans must be 'N', 'T' or 'C', not {trans!r}")
    code = None if trans is None else _TRANS[trans]
    if isinstance(Pr, TransposedFactor):
        w = Pr.trans
        if code is not None and code != w and not (Pr.dtype.kind != "c" and code in (1, 2)):  # Float64: adjoint = transpose
            raise ValueError(f"trans={trans!r} conflicts with Pr={Pr!r}")
        return Pr.parent, w
    return Pr, code or 0


def _own_size(A, Pr):
    if A is not None:
        return A.shape[0]
    if Pr is None:
        raise ValueError("ArgumentError: A=None selects the matrix of the factorization Pr, which is None")
    return Pr.n


def gmres(A, b, Pr=None, reltol=None, abstol=0.0, restart=None, maxiter=None, log=False, x0=None, device=None, trans=None):
    """Restarted GMRES(restart) on ``A x = b`` with right preconditioner ``Pr`` (a :class:`FactorNode`), behind the C ABI (``hs_gmres_{d,z}``).

    ``trans="T"`` / ``"C"`` (the letters of :meth:`FactorNode.solve`) solve ``transpose(A) x = b`` / ``adjoint(A) x = b`` preconditioned by
    ``transpose(Pr)`` / ``adjoint(Pr)`` (``hs_gmres_t_{d,z}``); ``A`` is always the matrix itself.  ``Pr=transpose(F)`` / ``adjoint(F)`` is
    shorthand for the matching ``trans``.  ``A=None`` takes the matrix ``Pr`` was factored from, as the handle holds it on the device: nothing
    is converted or uploaded.  With ``trans`` ``"N"`` (the default) and an explicit ``A`` the call is ``hs_gmres_{d,z}`` as before.

    Defaults follow IterativeSolvers 0.9: ``restart = min(20, n)``, ``maxiter = n``, ``reltol = sqrt(eps)``; convergence when
    ``||b - A x|| <= max(reltol * ||r0||, abstol)``.  Returns ``x`` (NumPy, host) or ``(x, history)`` with
    ``history = dict(resnorm=[...], isconverged, iters)``.  (``device`` is accepted for compatibility; the library uses the current device.)"""
    Pr, tcode = _op_of(Pr, trans)
    n = _own_size(A, Pr)
    cplx = (A is not None and np.iscomplexobj(A.data)) or np.iscomplexobj(b) or (Pr is not None and Pr.dtype.kind == "c")
    dt = np.complex128 if cplx else np.float64
    colptr, rowval, nz = _csc_fields(A, dt) if A is not None else (None, None, None)
    bb = np.ascontiguousarray(b, dtype=dt)
    x = np.zeros(n, dtype=dt) if x0 is None else np.ascontiguousarray(x0, dtype=dt).copy()
    maxit = n if maxiter is None else int(maxiter)
    hist = np.zeros(maxit + 2)
    iters, conv = _lib.i64(0), C.c_int(0)
    L = _lib.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tail = (vp(bb), vp(x), 0, int(x0 is not None), -1.0 if reltol is None else float(reltol), float(abstol), -1 if restart is None else int(restart), maxit,
            hist.ctypes.data_as(_lib.p_f64), C.byref(iters), C.byref(conv), None)
    h = Pr._h if Pr is not None else None
    if tcode == 0 and A is not None:
        fn = L.hs_gmres_z if cplx else L.hs_gmres_d
        _lib.check(fn(h, n, colptr.ctypes.data_as(_lib.p_i64), rowval.ctypes.data_as(_lib.p_i64), vp(nz), *tail))
    else:
        fn = L.hs_gmres_t_z if cplx else L.hs_gmres_t_d
        a3 = (None, None, None) if A is None else (colptr.ctypes.data_as(_lib.p_i64), rowval.ctypes.data_as(_lib.p_i64), vp(nz))
        _lib.check(fn(h, tcode, n, *a3, *tail))
    if log:
        return x, dict(resnorm=[float(v) for v in hist[: iters.value + 1]], isconverged=bool(conv.value), iters=int(iters.value))
    return x


gmres_native = gmres  # the name round 2 gave the C-ABI solver while `gmres` was still a torch restatement


def gmres_device(A, b_dev, solver, reltol=1e-9, abstol=0.0, restart=30, maxiter=30):
    """``hs_gmres_*`` on a torch device vector with the factorization held by a :class:`dist.StagedSolver` (single rank) as the right
    preconditioner; returns ``(x_dev, resnorm history)``."""
    import torch

    n = A.shape[0]
    cplx = b_dev.is_complex()
    dt = np.complex128 if cplx else np.float64
    colptr, rowval, nz = _csc_fields(A, dt)
    x = torch.zeros_like(b_dev)
    hist = np.zeros(int(maxiter) + 2)
    iters, conv = _lib.i64(0), C.c_int(0)
    L = _lib.lib()
    fn = L.hs_gmres_z if cplx else L.hs_gmres_d
    stream = C.c_void_p(torch.cuda.current_stream(b_dev.device).cuda_stream)
    _lib.check(fn(solver.backend._h, n, colptr.ctypes.data_as(_lib.p_i64), rowval.ctypes.data_as(_lib.p_i64), nz.ctypes.data_as(C.c_void_p),
                  C.c_void_p(b_dev.data_ptr()), C.c_void_p(x.data_ptr()), 1, 0, float(reltol), float(abstol), int(restart), int(maxiter),
                  hist.ctypes.data_as(_lib.p_f64), C.byref(iters), C.byref(conv), stream))
    return x, [float(v) for v in hist[: iters.value + 1]]


def gmres_block(A, B, Pr=None, reltol=None, abstol=0.0, restart=None, maxiter=None, log=False, X0=None, trans=None):
    """:func:`gmres` on every column of the ``n x nrhs`` block ``B`` in lockstep (``hs_gmres_block_{d,z}``): the columns share the restart
    cycle and the Arnoldi index, so a step applies ``Pr`` to all active columns with one block solve (``hs_ldiv_block_dev_*``) and multiplies
    by ``A`` with one SpMM.  Every column keeps its own Krylov space and stopping test and returns what :func:`gmres` returns for it alone
    (to the rounding by which :func:`ldiv_block` and :func:`ldiv` differ).  ``Pr`` must be a handle the block solve serves
    (:class:`UnsupportedError` otherwise: :func:`gmres` serves those).  Returns ``X`` or ``(X, [history dict per column])``; a 1-D ``B`` is
    one column and returns a vector (and one history dict).  With ``log=True`` the history buffer is ``(maxiter + 1) x nrhs`` doubles: give a
    ``maxiter`` when ``n`` and ``nrhs`` are both large (the default is ``n``).  ``trans``, ``Pr=transpose(F)`` / ``adjoint(F)`` and ``A=None``
    as in :func:`gmres` (``hs_gmres_block_t_{d,z}``, the block solve ``hs_ldiv_block_dev_t_*``).  ``Pr`` may be a :class:`ModifiedFactor`
    (:func:`modify`): ``A`` is then the modified matrix ``A1`` itself (``A=None`` raises ``ValueError``: the handle holds the old ``A``) and
    every step applies ``op(A1)^-1`` through ``hs_mod_ldiv_dev_*`` (``hs_gmres_block_mod_{d,z}``).  ``Pr`` may be a :class:`DemotedFactor`
    (:func:`demote`): every step applies ``op(F)^-1`` from the Float32 copy of the factors (``hs_gmres_block_f32_{d,z}``) while the Krylov
    solver stays Float64; ``A`` must be given (``A=None`` raises ``ValueError``: the copy holds no matrix)."""
    from .solver import DemotedFactor, ModifiedFactor

    mod = Pr if isinstance(Pr, ModifiedFactor) else None
    dem = Pr if isinstance(Pr, DemotedFactor) else None
    if dem is not None:  # Pr = hs.demote(F): the preconditioner hs_f32_ldiv_dev_* (hs_gmres_block_f32_*)
        if trans is not None and trans not in _TRANS:
            raise ValueError(f"trans must be 'N', 'T' or 'C', not {trans!r}")
        if A is None:
            raise ValueError("ArgumentError: A=None with Pr a DemotedFactor: a demoted factorization holds no matrix; pass A")
        tcode = 0 if trans is None else _TRANS[trans]
    elif mod is not None:  # Pr = hs.modify(F, ...): A is the MODIFIED matrix, the preconditioner hs_mod_ldiv_dev_* (hs_gmres_block_mod_*)
        if trans is not None and trans not in _TRANS:
            raise ValueError(f"trans must be 'N', 'T' or 'C', not {trans!r}")
        if A is None:
            raise ValueError("ArgumentError: A=None with Pr a ModifiedFactor: the handle holds the unmodified matrix; pass the modified A")
        tcode = 0 if trans is None else _TRANS[trans]
    else:
        Pr, tcode = _op_of(Pr, trans)
    n = _own_size(A, Pr)
    B = np.asarray(B)
    vec = B.ndim == 1
    if B.shape[0] != n:
        raise _lib.DimensionMismatch(f"DimensionMismatch: B has {B.shape[0]} rows, A is {n} x {n}")
    cplx = (A is not None and np.iscomplexobj(A.data)) or np.iscomplexobj(B) or (Pr is not None and Pr.dtype.kind == "c") or (X0 is not None and np.iscomplexobj(X0))
    dt = np.complex128 if cplx else np.float64
    colptr, rowval, nz = _csc_fields(A, dt) if A is not None else (None, None, None)
    Bm = np.asfortranarray(B.reshape(n, -1), dtype=dt)
    k = Bm.shape[1]
    if X0 is None:
        X = np.zeros((n, k), dtype=dt, order="F")
    else:
        X = np.array(np.asarray(X0).reshape(n, -1), dtype=dt, order="F")
        if X.shape != Bm.shape:
            raise _lib.DimensionMismatch(f"DimensionMismatch: X0 is {X.shape[0]} x {X.shape[1]}, B is {n} x {k}")
    maxit = n if maxiter is None else int(maxiter)
    # (maxiter + 1) x nrhs doubles, of which the library writes iters[c] + 1 per column: with the default maxiter = n that is 8 n nrhs bytes of
    # address space, so it is allocated only when the history is asked for
    hist = np.zeros((maxit + 1, max(k, 1)), order="F") if log else None
    iters = np.zeros(max(k, 1), dtype=np.int64)
    conv = np.zeros(max(k, 1), dtype=np.int32)
    L = _lib.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tail = (vp(Bm), n, vp(X), n, k, 0, int(X0 is not None), -1.0 if reltol is None else float(reltol), float(abstol), -1 if restart is None else int(restart), maxit,
            hist.ctypes.data_as(_lib.p_f64) if log else None, iters.ctypes.data_as(_lib.p_i64), conv.ctypes.data_as(C.POINTER(C.c_int)), None)
    h = Pr._h if Pr is not None else None
    if dem is not None:
        fn = L.hs_gmres_block_f32_z if cplx else L.hs_gmres_block_f32_d
        _lib.check(fn(h, tcode, n, colptr.ctypes.data_as(_lib.p_i64), rowval.ctypes.data_as(_lib.p_i64), vp(nz), *tail))
    elif mod is not None:
        fn = L.hs_gmres_block_mod_z if cplx else L.hs_gmres_block_mod_d
        _lib.check(fn(h, tcode, n, colptr.ctypes.data_as(_lib.p_i64), rowval.ctypes.data_as(_lib.p_i64), vp(nz), *tail))
    elif tcode == 0 and A is not None:
        fn = L.hs_gmres_block_z if cplx else L.hs_gmres_block_d
        _lib.check(fn(h, n, colptr.ctypes.data_as(_lib.p_i64), rowval.ctypes.data_as(_lib.p_i64), vp(nz), *tail))
    else:
        fn = L.hs_gmres_block_t_z if cplx else L.hs_gmres_block_t_d
        a3 = (None, None, None) if A is None else (colptr.ctypes.data_as(_lib.p_i64), rowval.ctypes.data_as(_lib.p_i64), vp(nz))
        _lib.check(fn(h, tcode, n, *a3, *tail))
    res = X[:, 0] if vec else X
    if log:
        chs = [dict(resnorm=[float(v) for v in hist[: iters[c] + 1, c]], isconverged=bool(conv[c]), iters=int(iters[c])) for c in range(k)]
        return res, (chs[0] if vec else chs)
    return res


def gmres_block_info():
    """Figures of this thread's last :func:`gmres_block` call (``hs_gmres_block_info``)."""
    out = np.zeros(8)
    _lib.check(_lib.lib().hs_gmres_block_info(out.ctypes.data_as(_lib.p_f64)))
    return {"seconds": float(out[0]), "prec_calls": int(out[1]), "column_applications": int(out[2]), "spmm_launches": int(out[3]), "cycles": int(out[4]),
            "groups": int(out[5]), "workspace_bytes": int(out[6]), "max_active": int(out[7])}
