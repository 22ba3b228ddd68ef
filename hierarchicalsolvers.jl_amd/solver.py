"""Host mirror of the reference's numeric API over the C ABI.

=====================================  ====================================================
reference (Julia)                      here
=====================================  ====================================================
``SolverOptions(; kw...)``             :class:`SolverOptions`  (HierarchicalSolvers.jl:30-79)
``factor(A, nd, nd_loc, opts; kw...)`` :func:`factor`          (factorization.jl:5-11)
``FactorNode{T}``                      :class:`FactorNode`     (factornode.jl:7-39)
``ldiv!(F, B)``, ``ldiv!(C, F, B)``    :func:`ldiv`            (factornode.jl:62-74)
``transpose(F)``, ``adjoint(F)``       :func:`transpose`, :func:`adjoint` (``ldiv`` takes them: ``A^T x = b``, ``A^H x = b``)
``maxrank(F)``                         :func:`maxrank`         (factornode.jl:49-57)
``opnorm(A, p)``, ``opnormestinv(A)``  :func:`opnorm`, :func:`opnormestinv` (on the factorization's A and F; ``hs_condest.hip``)
``cond(A, p)`` (estimated)             :func:`condest`
``xGERFS`` (refine, berr, ferr)        :func:`ldiv_refine`, :func:`ldiv_refine_block`
``logabsdet(F)``, ``logdet``, ``det``  :func:`logabsdet`, :func:`logdet`, :func:`det` (``hs_selinv.hip``)
selected inverse (no Julia name)       :func:`selinv`, :func:`selinv_diag`: ``diag(A^-1)`` and ``A^-1`` on the pattern of ``A``;
                                       :func:`selinv_lr`, :func:`selinv_lr_diag` for compressed factorizations
``eigs(A; nev, sigma)`` (Arpack)       :func:`eigs`: the eigenpairs of ``A`` nearest ``sigma`` from the factors of ``A - sigma*I`` (``hs_eigs.hip``)
``eigs(A, B; nev, sigma)`` (Arpack)    :func:`eigs` with ``M=B``: ``A x = lambda B x`` from the factors of ``A - sigma*B``
partial factorization (no Julia name)  :func:`schur_complement`, :func:`condense`, :func:`interface_solve`, :func:`expand` (``hs_interface.hip``)
``F \\ b``                              ``F.solve(b)``
=====================================  ====================================================

All arithmetic happens in ``libhs_solver.so`` on the GPU; this module only marshals arrays.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from . import _lib
from .nesteddissection import flatten_tree

__all__ = ["SolverOptions", "chkopts", "factor", "factorize", "FactorNode", "ldiv", "maxrank", "transpose", "adjoint", "opnorm", "opnormestinv", "condest",
           "ldiv_refine", "ldiv_refine_block", "ldiv_refine_block_info", "logabsdet", "logdet", "det", "ulv_mode", "selinv", "selinv_diag", "selinv_info", "selinv_lr", "selinv_lr_diag", "selinv_lr_info", "sym_info", "equil_info", "equil_scales",
           "sensitivity", "sensitivity_matrix", "misfit", "sens_info", "tangent", "gn_hessvec", "gn_diag", "gn_info", "eigs", "eigs_info", "eigs_gen_info", "interface_indices", "schur_complement", "condense", "interface_solve", "expand", "interface_info"]


class SolverOptions:
    """Mirror of ``mutable struct SolverOptions`` and its kw-constructor defaults
    ``5, 1, 1e-6, 1e-6, 0.5, 32, -1, 10, false`` (HierarchicalSolvers.jl:43-54)."""

    _fields = ("swlevel", "swsize", "atol", "rtol", "c_tol", "leafsize", "kest", "stepsize", "verbose")
    _ext = ("keep_schur", "seed", "profile", "split_size", "hss_min", "hss_dexp", "mf", "dist_top", "symmetric", "equilibrate")

    def __init__(self, **kw):
        self.swlevel, self.swsize = 5, 1
        self.atol, self.rtol, self.c_tol = 1e-6, 1e-6, 0.5
        self.leafsize, self.kest, self.stepsize = 32, -1, 10
        self.verbose = False
        self.keep_schur = False
        self.profile = False
        self.seed = 123
        self.split_size = 0  # columns per slice of a compressed front's interior block (multiple of 256, 0 = off)
        self.hss_min = 0  # > 0 (multiple of 1024): compressed-level fronts with at least this many interior DOFs keep D as HSS
        self.hss_dexp = None  # orders of magnitude by which the HSS form of D is tighter than atol, rtol (None: 2; 0: the same)
        # matrix-free compressed branch: S leaves flagged fronts as HSS, parents assemble from the children's generators.  True / 'dense': the
        # interior block D of such a parent is expanded and eliminated densely (HSS only where hss_min says so); 2 / 'hss': D is an HSS matrix
        self.mf = False
        # multi-rank factorizations: fronts above the rank cut are eliminated by all ranks of their group (csrc/hs_dist.h) instead of its first rank
        self.dist_top = False
        # A == A.T entry for entry (real symmetric or COMPLEX symmetric; not Hermitian): dense fronts update only their lower triangle.  Checked on
        # the device by hs_numeric_begin (ValueError naming the first offending entry); sym_info(F) reports what the factorization did with it
        self.symmetric = False
        # scale the rows and columns of A by powers of two on the device before it is factored (A_s = 2^er A 2^ec, Ruiz sweeps in the infinity
        # norm): pivoting and the compression tolerances atol / rtol then act on A_s, the solves scale B and the result so that they answer for A
        # itself, bit for bit as a handle of the prescaled matrix would; equil_info(F) / equil_scales(F) report what was found
        self.equilibrate = False
        self._set(kw)

    def _set(self, kw):
        for k, v in kw.items():
            if k not in self._fields and k not in self._ext:
                raise TypeError(f"type SolverOptions has no field {k}")  # setfield! on an unknown field
            setattr(self, k, v)

    def copy(self, **kw):
        """``copy(opts; kw...)`` (HierarchicalSolvers.jl:62-71)."""
        o = SolverOptions()
        for f in self._fields + self._ext:
            setattr(o, f, getattr(self, f))
        o._set(kw)
        return o

    def to_c(self):
        o = _lib.hs_options()
        o.swlevel, o.swsize = int(self.swlevel), int(self.swsize)
        o.atol, o.rtol, o.c_tol = float(self.atol), float(self.rtol), float(self.c_tol)
        o.leafsize, o.kest, o.stepsize = int(self.leafsize), int(self.kest), int(self.stepsize)
        o.verbose = 1 if self.verbose else 0
        o.keep_schur = 1 if self.keep_schur else 0
        o.profile = 1 if self.profile else 0
        o.seed = int(self.seed)
        ss = int(self.split_size)
        if ss < 0 or ss % 256 or ss // 256 > 255:
            raise ValueError("split_size must be a multiple of 256 in 0:65280")
        o.split = ss // 256
        hm = int(self.hss_min)
        if hm < 0 or hm % 1024 or hm // 1024 > 255:
            raise ValueError("hss_min must be a multiple of 1024 in 0:261120")
        o.hss_d = hm // 1024
        if self.mf in (False, None, 0):
            o.mf = 0
        elif self.mf in (True, 1, "dense"):
            o.mf = 1  # interior blocks of the matrix-free fronts dense unless hss_min asks for HSS
        elif self.mf in (2, "hss"):
            o.mf = 2  # every interior block an HSS matrix (the reference's formulation)
        elif self.mf in (3, "block"):
            o.mf = 3  # interior blocks as the reference's 2x2 block factorization over the children's HSS blocks (blockmatrix.jl:121-130)
        else:
            raise ValueError("mf must be False, True / 'dense', 2 / 'hss' or 3 / 'block'")
        o.dist_top = 1 if self.dist_top else 0
        o.symmetric = 1 if self.symmetric else 0
        o.equilibrate = 1 if self.equilibrate else 0
        if self.hss_dexp is not None:
            if not 0 <= int(self.hss_dexp) <= 12:
                raise ValueError("hss_dexp must be in 0:12")
            o.hss_dexp = int(self.hss_dexp) + 1
        return o


def chkopts(opts):
    """``chkopts!`` (HierarchicalSolvers.jl:73-79); ``ArgumentError`` -> ``ValueError``."""
    if not opts.swsize >= 1:
        raise ValueError("ArgumentError: swsize")
    if not opts.atol >= 0.0:
        raise ValueError("ArgumentError: atol")
    if not opts.rtol >= 0.0:
        raise ValueError("ArgumentError: rtol")
    if not (0.0 < opts.c_tol <= 1.0):
        raise ValueError("ArgumentError: c_tol")
    if not opts.leafsize >= 1:
        raise ValueError("ArgumentError: leafsize")


def _p64(a):
    return a.ctypes.data_as(_lib.p_i64)


def _pf64(a):
    return a.ctypes.data_as(_lib.p_f64)


class FactorNode:
    """Handle to a device-resident factorization (the reference's ``FactorNode{T}`` tree,
    factornode.jl:7-39).  The per-node blocks stay in HBM; ``node_blocks`` exports one node for
    inspection.  Freed by ``hs_free`` when garbage-collected (the Julia shim uses a finalizer)."""

    def __init__(self, handle, dtype, n, flat):
        self._h = handle
        self.dtype = np.dtype(dtype)
        self.n = int(n)
        self._flat = flat
        self._pattern = None  # (indptr, indices) of the factored matrix, CSC with sorted indices: the order of hs_selinv's pattern values

    def __del__(self):
        self.free()

    def free(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().hs_free(h)

    @property
    def eltype(self):  # eltype(::FactorNode{T}) (factornode.jl:41)
        return self.dtype.type

    def __repr__(self):  # Base.show (factornode.jl:42)
        return f"FactorNode{{{'ComplexF64' if self.dtype.kind == 'c' else 'Float64'}}}"

    @property
    def shape(self):
        return (self.n, self.n)

    def stats(self):
        st = _lib.hs_stats()
        _lib.check(_lib.lib().hs_get_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def solve(self, b, trans="N"):
        """``F \\ b``; ``trans="T"``: ``transpose(F) \\ b``, ``"C"``: ``adjoint(F) \\ b``."""
        if trans not in ("N", "T", "C"):
            raise ValueError(f"trans must be 'N', 'T' or 'C', not {trans!r}")
        return ldiv({"N": self, "T": transpose(self), "C": adjoint(self)}[trans], b)

    # -- inspection (tests) -------------------------------------------------------------------
    @property
    def nnodes(self):
        return int(self._flat["nnodes"])

    def node_info(self, node):
        ni, nb, lv = _lib.i64(), _lib.i64(), _lib.i64()
        _lib.check(_lib.lib().hs_node_info(self._h, node, C.byref(ni), C.byref(nb), C.byref(lv)))
        return ni.value, nb.value, lv.value

    def node_ranks(self, node):
        """``(compressed, rank(L), rank(R))`` of one front (ranks are 0 for dense Gauss transforms)."""
        rl, rr = _lib.i64(), _lib.i64()
        st = _lib.lib().hs_node_ranks(self._h, node, C.byref(rl), C.byref(rr))
        if st < 0:
            _lib.check(st)
        return bool(st), rl.value, rr.value

    def node_blocks(self, node, with_schur=False):
        """Stored blocks of one node: ``LU`` (ni x ni packed), ``Lbi`` (nb x ni), ``Uib`` (ni x nb),
        ``rperm`` (0-based, ``(P x)[i] = x[rperm[i]]``) and optionally ``S`` (needs ``keep_schur``)."""
        ni, nb, _ = self.node_info(node)
        L = _lib.lib()
        out = {}
        for name, which, shp in (("LU", _lib.HS_BLK_LU, (ni, ni)), ("Lbi", _lib.HS_BLK_LBI, (nb, ni)), ("Uib", _lib.HS_BLK_UIB, (ni, nb))) + (
            (("S", _lib.HS_BLK_S, (nb, nb)),) if with_schur else ()
        ):
            a = np.zeros(shp, dtype=self.dtype, order="F")
            if a.size:
                _lib.check(L.hs_node_export(self._h, node, which, a.ctypes.data_as(_lib.p_f64)))
            out[name] = a
        rp = np.zeros(ni, dtype=np.int64)
        if ni:
            _lib.check(L.hs_node_export_piv(self._h, node, _p64(rp)))
        out["rperm"] = rp
        return out

    def node_lu(self, node):
        """``(LU, rperm)`` of one front's interior block wherever it keeps a dense pivoted LU -- also a matrix-free front with a densely
        eliminated ``D`` (``mf=True``), which exports no other block (``HS_BLK_DLU``)."""
        ni, _, _ = self.node_info(node)
        LU = np.zeros((ni, ni), dtype=self.dtype, order="F")
        rp = np.zeros(ni, dtype=np.int64)
        if ni:
            _lib.check(_lib.lib().hs_node_export(self._h, node, _lib.HS_BLK_DLU, LU.ctypes.data_as(_lib.p_f64)))
            _lib.check(_lib.lib().hs_node_export_piv(self._h, node, _p64(rp)))
        return LU, rp

    def schur_hss(self, node, **kw):
        """``F.S`` of one node as an :class:`hss.HssMatrix` (``compress(S[perm,perm], cl, cl)``, factorization.jl:56-57,109-110;
        needs ``keep_schur``).  Without keywords the factorization's own ``leafsize, atol, rtol, kest, seed`` apply; with any of
        ``leafsize, atol, rtol, kest, seed, pad, level_scale`` given, the others take the ``SolverOptions`` defaults."""
        import ctypes as C

        from . import hss

        o = None
        if kw:
            d = dict(leafsize=32, atol=1e-6, rtol=1e-6, kest=64, pad=8, seed=123, level_scale=0.5)  # SolverOptions defaults
            d.update(kw)
            o = C.byref(_lib.hs_hss_options(d["leafsize"], 0, d["atol"], d["rtol"], d["kest"], d["pad"], d["seed"], d["level_scale"]))
        h = C.c_void_p()
        _lib.check(_lib.lib().hs_node_schur_hss(self._h, node, o, C.byref(h)))
        return hss.HssMatrix(h, self.dtype == np.complex128)

    def reference_blocks(self, node, with_schur=False):
        """The reference's FactorNode fields of one node, rebuilt from the stored factors:
        ``D = P'LU`` (raw interior block), ``L = Abi*D^-1``, ``R = D^-1*Aib`` (factorization.jl:33-37,69-71)."""
        import scipy.linalg as sla

        b = self.node_blocks(node, with_schur)
        LU, rp = b["LU"], b["rperm"]
        ni = LU.shape[0]
        Lm = np.tril(LU, -1) + np.eye(ni, dtype=self.dtype)
        Um = np.triu(LU)
        PD = Lm @ Um
        D = np.empty_like(PD)
        D[rp] = PD  # (P D)[i] = D[rperm[i]]
        # L_ref = Lbi * L^-1 * P ;  R_ref = U^-1 * Uib
        X = sla.solve_triangular(Lm, b["Lbi"].T, lower=True, trans="T", unit_diagonal=True) if ni else b["Lbi"].T  # L^-T Lbi^T
        Lref = np.empty_like(b["Lbi"])
        Lref[:, rp] = X.T  # (M P)[:, rp[i]] = M[:, i]
        Rref = sla.solve_triangular(Um, b["Uib"], lower=False) if ni and b["Uib"].size else b["Uib"].copy()
        out = dict(D=D, L=Lref, R=Rref)
        if with_schur:
            out["S"] = b["S"]
        return out


def factor(A, nd, nd_loc, opts=None, **kw):
    """``factor(A::SparseMatrixCSC{T}, nd, nd_loc, opts=SolverOptions(); kw...) -> FactorNode{T}``
    (factorization.jl:5-11).  ``T`` is ``float64`` or ``complex128``."""
    opts = (opts or SolverOptions()).copy(**kw)
    chkopts(opts)
    A = sp.csc_matrix(A)
    if A.shape[0] != A.shape[1]:
        raise _lib.DimensionMismatch("DimensionMismatch: A is not square")
    A.sort_indices()
    n = A.shape[0]
    is_c = np.iscomplexobj(A.data)
    dtype = np.complex128 if is_c else np.float64
    colptr = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1  # Julia's 1-based SparseMatrixCSC fields
    rowval = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    nzval = np.ascontiguousarray(A.data, dtype=dtype)
    flat = flatten_tree(nd, nd_loc)
    t = _lib.hs_tree()
    t.nnodes = flat["nnodes"]
    for k in ("left", "right", "int_ptr", "int_idx", "bnd_ptr", "bnd_idx", "iloc_ptr", "iloc_idx", "bloc_ptr", "bloc_idx"):
        flat[k] = np.ascontiguousarray(flat[k], dtype=np.int64)
        setattr(t, k, _p64(flat[k]))
    co = opts.to_c()
    h = C.c_void_p()
    L = _lib.lib()
    fn = L.hs_factor_z if is_c else L.hs_factor_d
    st = fn(n, _p64(colptr), _p64(rowval), nzval.ctypes.data_as(_lib.p_f64), C.byref(t), C.byref(co), C.byref(h))
    _lib.check(st)
    F = FactorNode(h, dtype, n, flat)
    F._pattern = (A.indptr.copy(), A.indices.copy())
    return F


factorize = factor  # BASELINE.json's north star uses this name


def trim():
    """Give the device blocks the library parks between factorizations (the factor arena of the last freed handle, the recycled blocks of the
    HSS / low-rank modules) back to the driver; returns the bytes released (``hs_trim``, include/hs_solver.h)."""
    return int(_lib.lib().hs_trim())


class TransposedFactor:
    """``Transpose(F)`` / ``Adjoint(F)`` of a :class:`FactorNode` (Julia's lazy wrappers): holds the factorization, reads the same
    factors.  Made by :func:`transpose` / :func:`adjoint`, consumed by :func:`ldiv` (``hs_ldiv_t_*``, include/hs_solver.h)."""

    def __init__(self, parent, conj):
        self.parent = parent
        self.conj = bool(conj)

    @property
    def trans(self):
        return 2 if self.conj else 1  # the `trans` argument of hs_ldiv_t_*

    @property
    def n(self):
        return self.parent.n

    @property
    def dtype(self):
        return self.parent.dtype

    @property
    def shape(self):
        return self.parent.shape

    def __repr__(self):
        return f"{'Adjoint' if self.conj else 'Transpose'}{{{repr(self.parent)}}}"

    def solve(self, b):
        """``transpose(F) \\ b`` / ``adjoint(F) \\ b``."""
        return ldiv(self, b)


def _wrap(F, conj):
    if isinstance(F, TransposedFactor):
        if F.conj == conj or F.dtype.kind != "c":  # transpose(transpose(F)) = adjoint(adjoint(F)) = F; Float64: adjoint = transpose
            return F.parent
        raise TypeError("conj(F) of a ComplexF64 factorization (transpose of an adjoint) is not supported")
    if not isinstance(F, FactorNode):
        raise TypeError(f"expected a FactorNode, got {type(F).__name__}")
    return TransposedFactor(F, conj)


def transpose(F):
    """``transpose(F)``: ``ldiv(transpose(F), B)`` solves ``A^T X = B`` with the factors of ``A``."""
    return _wrap(F, False)


def adjoint(F):
    """``adjoint(F)`` (``F'``): ``ldiv(adjoint(F), B)`` solves ``A^H X = B`` with the factors of ``A``."""
    return _wrap(F, True)


def _ldiv_dense(name, sym, args):
    """The body of :func:`ldiv`, :func:`ldiv_block`, :func:`ldiv_block_t` and :func:`ldiv_ulv`: ``(F, B)`` or ``(C, F, B)`` with ``F`` possibly
    wrapped by :func:`transpose` / :func:`adjoint`, the shape and dtype rules of ``ldiv!``, column-major staging, one call of
    ``<sym>_d`` / ``<sym>_z`` with ``trans``.  ``sym`` None: ``hs_ldiv_*`` for a plain ``F``, ``hs_ldiv_t_*`` otherwise."""
    if len(args) == 2:
        F, B = args
        Cout = None
    elif len(args) == 3:
        Cout, F, B = args
    else:
        raise TypeError(f"{name}(F, B) or {name}(C, F, B)")
    trans = 0
    if isinstance(F, TransposedFactor):
        F, trans = F.parent, F.trans
    B = np.asarray(B)
    if B.shape[0] != F.n:
        raise _lib.DimensionMismatch(f"DimensionMismatch: B has {B.shape[0]} rows, F is {F.n} x {F.n}")
    if B.dtype != F.dtype:
        if F.dtype.kind == "f" and B.dtype.kind == "c":
            raise TypeError("MethodError: no method matching ldiv!(::Array{ComplexF64}, ::FactorNode{Float64}, ::Array{ComplexF64})")
        B = B.astype(F.dtype)
    vec = B.ndim == 1
    Bm = np.asfortranarray(B.reshape(F.n, -1))
    Cm = np.empty_like(Bm, order="F")
    if sym is None:
        sym = "hs_ldiv_t" if trans else "hs_ldiv"
    fn = getattr(_lib.lib(), sym + ("_z" if F.dtype.kind == "c" else "_d"))
    head = (F._h,) if sym == "hs_ldiv" else (F._h, trans)  # hs_ldiv_* is the one entry without a trans argument
    _lib.check(fn(*head, Cm.ctypes.data_as(_lib.p_f64), F.n, Bm.ctypes.data_as(_lib.p_f64), F.n, F.n, Bm.shape[1]))
    res = Cm[:, 0] if vec else Cm
    if Cout is not None:
        Cout[...] = res
        return Cout
    return res


def ldiv(*args):
    """``ldiv!(F, B)`` / ``ldiv!(C, F, B)`` (factornode.jl:62-74): ``C = F^-1 B`` for a vector or an
    ``n x nrhs`` matrix.  The 2-argument form returns a new array like the reference (which
    allocates ``similar(B)``, factornode.jl:62); the 3-argument form writes into ``C`` (``C`` may be ``B``).
    ``F`` may be ``transpose(F)`` or ``adjoint(F)``: then ``C = F^-T B`` / ``C = F^-H B``."""
    return _ldiv_dense("ldiv", None, args)


def ldiv_block(*args):
    """``ldiv!(F, B)`` / ``ldiv!(C, F, B)`` through the block solve (``hs_ldiv_block_*``): the same arguments and results as :func:`ldiv`
    (to rounding), but the ``nrhs`` columns travel through the elimination tree together, ``HS_LDIV_BLOCK_COLS`` (default 32) at a time, so
    the factors are read once per chunk instead of once per column.  ``F`` must be a plain :class:`FactorNode` whose fronts keep a dense LU
    of their interior block (``transpose(F)`` / ``adjoint(F)`` -- served by :func:`ldiv_block_t` -- and HSS interior blocks raise
    :class:`UnsupportedError`)."""
    return _ldiv_dense("ldiv_block", "hs_ldiv_block", args)


def ldiv_block_t(*args):
    """``ldiv!(F, B)`` / ``ldiv!(C, F, B)`` with ``F`` a :class:`FactorNode`, ``transpose(F)`` or ``adjoint(F)``, through the block solve
    (``hs_ldiv_block_t_*``): the arguments and results of :func:`ldiv_block`, the columns travelling through the tree together in both
    directions.  A plain ``F`` returns the bits of :func:`ldiv_block`.  The same handles are served as there."""
    return _ldiv_dense("ldiv_block_t", "hs_ldiv_block_t", args)


def ldiv_ulv(*args):
    """``ldiv!(F, B)`` / ``ldiv!(C, F, B)`` for a block ``B`` with ``F`` a :class:`FactorNode`, ``transpose(F)`` or ``adjoint(F)``
    (``hs_ldiv_ulv_*``): the block solve that also serves fronts whose interior block ``D`` is held as an HSS matrix (``hss_d``,
    ``mf = 2, 3``) -- one ULV solve with ``D`` (transposed: from the same stored factors) per front and chunk of columns.  A handle
    without such fronts returns the bits of :func:`ldiv_block_t`."""
    return _ldiv_dense("ldiv_ulv", "hs_ldiv_ulv", args)


def ldiv_block_info(F):
    """Figures of the last :func:`ldiv_block` / :func:`ldiv_block_t` call on ``F`` (``hs_ldiv_block_info``): device seconds, factor bytes read by the model
    (chunks x sum over fronts of ``(ni^2 + 2 ni nb) sizeof(T)``), flops executed on the matrix pipe (padding included), useful flops,
    column chunks, workspace bytes."""
    out = np.zeros(6)
    _lib.check(_lib.lib().hs_ldiv_block_info(F._h, _pf64(out)))
    return {"seconds": float(out[0]), "factor_bytes": float(out[1]), "flops_executed": float(out[2]), "flops_useful": float(out[3]),
            "chunks": int(out[4]), "workspace_bytes": int(out[5])}


def _mul_operand(F, what):
    """``(FactorNode, trans)`` of the operand of :func:`mul` / :func:`factor_error`; the other factor objects are refused."""
    if isinstance(F, (ModifiedFactor, DemotedFactor)):
        raise _lib.UnsupportedError(f"{what}: a {type(F).__name__} is not served (products with the stored factors of a FactorNode, transpose(F) or adjoint(F) only)")
    return _unwrap(F)


def _device_block(name, F, X):
    """``(address, ld, nrhs)`` of a column-major device tensor with ``F.n`` rows and ``F``'s element type."""
    import torch

    want = torch.complex128 if F.dtype.kind == "c" else torch.float64
    if not X.is_cuda or X.dtype != want:
        raise TypeError(f"{name}: a device block must be a device tensor of {F.dtype}")
    if X.dim() not in (1, 2) or X.shape[0] != F.n:
        raise _lib.DimensionMismatch(f"DimensionMismatch: B has {tuple(X.shape)[:1]} rows, F is {F.n} x {F.n}")
    nrhs = 1 if X.dim() == 1 else X.shape[1]
    ld = F.n if (X.dim() == 1 or nrhs == 1) else X.stride(1)
    if (F.n > 1 and X.stride(0) != 1) or ld < F.n:
        raise ValueError(f"{name}: a device block must be column-major (stride 1 down a column)")
    return X.data_ptr(), ld, nrhs


def mul(*args):
    """``mul(F, X)`` / ``mul(C, F, X)``: ``C = op(F) X`` with the STORED factorization as an operator (``hs_mul_*``; ``lmul!``-style, the
    counterpart of :func:`ldiv_block_t`).  ``F`` is a :class:`FactorNode`, ``transpose(F)`` or ``adjoint(F)``; ``X`` a vector, an
    ``n x nrhs`` NumPy block (the shape and dtype rules of :func:`ldiv`) or a column-major device tensor (``hs_mul_dev_*`` on the current
    stream; the result is a new device tensor, or ``C``, which may be ``X``).  For an exact factorization ``F X = A X`` to rounding; for a
    compressed one it is the product with the approximation the solves invert.  Two calls return the same bits and a column does not depend
    on its neighbours.  The handles :func:`ldiv_block_t` refuses are refused; so are :class:`ModifiedFactor` and :class:`DemotedFactor`."""
    if len(args) == 2:
        Fo, X = args
        Cout = None
    elif len(args) == 3:
        Cout, Fo, X = args
    else:
        raise TypeError("mul(F, X) or mul(C, F, X)")
    F, trans = _mul_operand(Fo, "mul")
    if hasattr(X, "data_ptr"):  # a device tensor
        import torch

        px, ldx, nrhs = _device_block("mul", F, X)
        if Cout is None:
            Cout = torch.empty((nrhs, F.n), dtype=X.dtype, device=X.device).T if X.dim() == 2 else torch.empty_like(X)
        elif not hasattr(Cout, "data_ptr") or tuple(Cout.shape) != tuple(X.shape):
            raise TypeError("mul: C must be a device tensor of X's shape")
        pc, ldc, _ = _device_block("mul", F, Cout)
        fn = getattr(_lib.lib(), "hs_mul_dev" + ("_z" if F.dtype.kind == "c" else "_d"))
        _lib.check(fn(F._h, trans, pc, ldc, px, ldx, F.n, nrhs, torch.cuda.current_stream().cuda_stream))
        return Cout
    return _ldiv_dense("mul", "hs_mul", args)


def mul_info(F):
    """Figures of the last :func:`mul` (or :func:`factor_error`) on ``F`` (``hs_mul_info``), the keys of :func:`ldiv_block_info`.  A product
    is never filed as the handle's last block solve."""
    F, _ = _mul_operand(F, "mul_info")
    out = np.zeros(6)
    _lib.check(_lib.lib().hs_mul_info(F._h, _pf64(out)))
    return {"seconds": float(out[0]), "factor_bytes": float(out[1]), "flops_executed": float(out[2]), "flops_useful": float(out[3]),
            "chunks": int(out[4]), "workspace_bytes": int(out[5])}


def factor_error(F, k=32, seed=0, probes=None, full=False):
    """``||op(A) W - op(F) W||_F / ||op(A) W||_F`` on the device (``hs_factor_error_*``): how far the stored factorization is from the
    matrix it was made from, a property of the handle alone -- no solve, no right-hand side, no conditioning.  ``probes`` (``n x k`` NumPy
    block or column-major device tensor) gives ``W``; otherwise ``W`` is the library's ``k`` seeded +-1 columns (no generator state: two
    calls return the same bits), for which the figure estimates ``||op(A) - op(F)||_F / ||op(A)||_F`` (Hutchinson: relative deviation of
    the squared norm about ``sqrt(2 / k)``).  ``full=True`` returns ``{"error", "norm_r", "norm_aw", "seconds"}``."""
    F, trans = _mul_operand(F, "factor_error")
    fn = getattr(_lib.lib(), "hs_factor_error" + ("_z" if F.dtype.kind == "c" else "_d"))
    out = np.zeros(4)
    if probes is None:
        _lib.check(fn(F._h, trans, None, 0, int(k), int(seed), 0, _pf64(out)))
    elif hasattr(probes, "data_ptr"):
        pw, ldw, kk = _device_block("factor_error", F, probes)
        _lib.check(fn(F._h, trans, pw, ldw, kk, int(seed), 1, _pf64(out)))
    else:
        W = np.asarray(probes)
        if W.ndim not in (1, 2) or W.shape[0] != F.n:
            raise _lib.DimensionMismatch(f"DimensionMismatch: probes has {W.shape[:1]} rows, F is {F.n} x {F.n}")
        if W.dtype.kind == "c" and F.dtype.kind != "c":
            raise TypeError("MethodError: ComplexF64 probes for a Float64 factorization")
        W = np.asfortranarray(W.reshape(F.n, -1).astype(F.dtype, copy=False))
        _lib.check(fn(F._h, trans, W.ctypes.data, F.n, W.shape[1], int(seed), 0, _pf64(out)))
    if full:
        return {"error": float(out[0]), "norm_r": float(out[1]), "norm_aw": float(out[2]), "seconds": float(out[3])}
    return float(out[0])


class ModifiedFactor:
    """``A + U V^H`` (or ``A + dA``) solved from the factorization of ``A`` (``hs_mod``, include/hs_solver.h): made by :func:`modify`, consumed
    by :func:`ldiv_mod` and by ``gmres_block(A1, B, Pr=M)``.  Holds ``F`` (which therefore outlives it) and, on the device, ``U``, ``V`` (or
    the modified columns), ``Z = F^-1 U`` and the LU of the ``k x k`` capacitance matrix ``C = I + V^H Z``."""

    def __init__(self, handle, parent, k):
        self._h = handle
        self.parent = parent
        self.k = int(k)

    def __del__(self):
        self.free()

    def free(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().hs_mod_free(h)

    @property
    def n(self):
        return self.parent.n

    @property
    def dtype(self):
        return self.parent.dtype

    @property
    def shape(self):
        return self.parent.shape

    @property
    def rcond(self):
        """``1 / (||C||_1 ||C^-1||_1)`` of the capacitance matrix (1 for ``k = 0``): what the correction costs in accuracy."""
        return self.info()["rcond"]

    def info(self):
        """``hs_mod_info``: rank, ``rcond``, seconds to build, device seconds of the last solve, device bytes held, whether ``W = F^-H V`` exists
        (built by the first transposed solve), block-solve calls issued so far."""
        out = np.zeros(8)
        _lib.check(_lib.lib().hs_mod_info(self._h, _pf64(out)))
        return {"k": int(out[0]), "rcond": float(out[1]), "build_seconds": float(out[2]), "solve_seconds": float(out[3]), "bytes": int(out[4]),
                "has_w": bool(out[5]), "block_solves": int(out[6])}

    def __repr__(self):
        return f"ModifiedFactor{{{repr(self.parent)}, k={self.k}}}"


def modify(F, U=None, V=None, dA=None):
    """A :class:`ModifiedFactor` of ``A1 = A + U V^H`` (``U``, ``V``: ``n x k`` arrays, ``k <= 256``; Float64: ``V^T``) or of ``A1 = A + dA``
    (``dA``: an ``n x n`` ``scipy.sparse`` matrix; its nonempty columns ``J`` give ``U = dA[:, J]``, ``V = I[:, J]``) from the factorization
    ``F`` of ``A``, without refactoring (``hs_mod_create_*``).  Indices refer to the factored (already permuted) matrix.  ``F`` must be a
    plain :class:`FactorNode` that :func:`ldiv_block_t` serves (:class:`UnsupportedError` otherwise, and for ``k > 256``: refactor);
    a singular ``A1`` raises :class:`SingularException`."""
    if not isinstance(F, FactorNode):
        raise TypeError(f"expected a FactorNode, got {type(F).__name__}")
    if dA is not None and (U is not None or V is not None):
        raise ValueError("ArgumentError: modify takes either U and V or dA, not both")
    if dA is None and (U is None) != (V is None):
        raise ValueError("ArgumentError: modify needs both U and V")
    n = F.n
    sfx = "_z" if F.dtype.kind == "c" else "_d"
    h = C.c_void_p()
    if dA is not None:
        if not sp.issparse(dA):
            raise TypeError(f"expected a scipy.sparse matrix for dA, got {type(dA).__name__}")
        if dA.shape != (n, n):
            raise _lib.DimensionMismatch(f"DimensionMismatch: dA is {dA.shape[0]} x {dA.shape[1]}, F is {n} x {n}")
        if F.dtype.kind == "f" and dA.dtype.kind == "c":
            raise TypeError("MethodError: a ComplexF64 modification of a FactorNode{Float64}")
        dA = sp.csc_matrix(dA, copy=True).astype(F.dtype)
        dA.sum_duplicates()
        dA.sort_indices()
        colptr = np.ascontiguousarray(dA.indptr, dtype=np.int64) + 1
        rowval = np.ascontiguousarray(dA.indices, dtype=np.int64) + 1
        vals = np.ascontiguousarray(dA.data, dtype=F.dtype)
        k = int(np.count_nonzero(np.diff(colptr)))
        _lib.check(getattr(_lib.lib(), "hs_mod_create_sparse" + sfx)(F._h, n, _p64(colptr), _p64(rowval), vals.ctypes.data_as(C.c_void_p), C.byref(h)))
        return ModifiedFactor(h, F, k)
    if U is None:
        Um = Vm = np.zeros((n, 0), dtype=F.dtype, order="F")
    else:
        U, V = np.asarray(U), np.asarray(V)
        if U.ndim == 1:
            U = U.reshape(-1, 1)
        if V.ndim == 1:
            V = V.reshape(-1, 1)
        if U.ndim != 2 or V.ndim != 2 or U.shape != V.shape or U.shape[0] != n:
            raise _lib.DimensionMismatch(f"DimensionMismatch: U is {U.shape}, V is {V.shape}, F is {n} x {n}")
        if F.dtype.kind == "f" and (U.dtype.kind == "c" or V.dtype.kind == "c"):
            raise TypeError("MethodError: a ComplexF64 modification of a FactorNode{Float64}")
        Um = np.asfortranarray(U, dtype=F.dtype)
        Vm = np.asfortranarray(V, dtype=F.dtype)
    k = Um.shape[1]
    _lib.check(getattr(_lib.lib(), "hs_mod_create" + sfx)(F._h, n, k, Um.ctypes.data_as(C.c_void_p), max(n, 1), Vm.ctypes.data_as(C.c_void_p), max(n, 1), C.byref(h)))
    return ModifiedFactor(h, F, k)


_MOD_TRANS = {None: 0, "N": 0, "T": 1, "C": 2, "H": 2}


def ldiv_mod(*args, trans="N"):
    """``ldiv_mod(M, B, trans="N")`` / ``ldiv_mod(C, M, B, trans=...)``: ``C = op(A1)^-1 B`` for a :class:`ModifiedFactor` ``M`` of ``A1``
    (``hs_mod_ldiv_*``), with the shape and dtype rules of :func:`ldiv`; ``trans`` as :meth:`hss.HssMatrix.ldiv` (``"N"``, ``"T"``:
    ``transpose(A1)``, ``"C"`` or ``"H"``: ``adjoint(A1)``).  Per chunk of ``HS_LDIV_BLOCK_COLS`` columns: one block solve with ``F``, one
    tall-skinny inner product, one ``k x k`` solve, one rank-``k`` correction.  ``k = 0`` returns the bits of :func:`ldiv_block_t`."""
    if len(args) == 2:
        M, B = args
        Cout = None
    elif len(args) == 3:
        Cout, M, B = args
    else:
        raise TypeError("ldiv_mod(M, B) or ldiv_mod(C, M, B)")
    if not isinstance(M, ModifiedFactor):
        raise TypeError(f"expected a ModifiedFactor, got {type(M).__name__}")
    if trans not in _MOD_TRANS:
        raise ValueError(f"trans must be None, 'N', 'T', 'C' or 'H', got {trans!r}")
    B = np.asarray(B)
    if B.shape[0] != M.n:
        raise _lib.DimensionMismatch(f"DimensionMismatch: B has {B.shape[0]} rows, A1 is {M.n} x {M.n}")
    if B.dtype != M.dtype:
        if M.dtype.kind == "f" and B.dtype.kind == "c":
            raise TypeError("MethodError: no method matching ldiv!(::Array{ComplexF64}, ::ModifiedFactor{Float64}, ::Array{ComplexF64})")
        B = B.astype(M.dtype)
    vec = B.ndim == 1
    Bm = np.asfortranarray(B.reshape(M.n, -1))
    Cm = np.empty_like(Bm, order="F")
    fn = getattr(_lib.lib(), "hs_mod_ldiv" + ("_z" if M.dtype.kind == "c" else "_d"))
    _lib.check(fn(M._h, _MOD_TRANS[trans], Cm.ctypes.data_as(_lib.p_f64), M.n, Bm.ctypes.data_as(_lib.p_f64), M.n, M.n, Bm.shape[1]))
    res = Cm[:, 0] if vec else Cm
    if Cout is not None:
        Cout[...] = res
        return Cout
    return res


class DemotedFactor:
    """A stand-alone copy of a factorization with its stored factors in Float32 (ComplexF32 for a ComplexF64 ``F``): made by :func:`demote`,
    consumed by :func:`ldiv_f32` and by ``gmres_block(A, B, Pr=G)`` (``hs_f32``, include/hs_solver.h).  It keeps no reference to ``F``,
    which may be freed; right-hand sides, results and every accumulation stay Float64 / ComplexF64."""

    def __init__(self, handle, dtype, n):
        self._h = handle
        self.dtype = np.dtype(dtype)
        self.n = int(n)

    def __del__(self):
        self.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def free(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().hs_f32_free(h)

    @property
    def shape(self):
        return (self.n, self.n)

    @property
    def nbytes(self):
        """Device bytes the copy holds: Float32 values plus indices, descriptors and padding (the work blocks of the solve apart)."""
        i = self.info()
        return i["value_bytes"] + i["index_bytes"]

    def info(self):
        """``hs_f32_info``: device seconds of the last solve, Float32 value bytes, the Float64 bytes of the same elements in ``F`` (twice
        that), index / descriptor / padding bytes, work-block bytes, elements flushed to zero or a subnormal, chunks of the last solve,
        seconds of the demotion."""
        out = np.zeros(8)
        _lib.check(_lib.lib().hs_f32_info(self._h, _pf64(out)))
        return {"solve_seconds": float(out[0]), "value_bytes": int(out[1]), "f64_bytes": int(out[2]), "index_bytes": int(out[3]), "workspace_bytes": int(out[4]),
                "flushed": int(out[5]), "chunks": int(out[6]), "demote_seconds": float(out[7])}

    def __repr__(self):
        return f"DemotedFactor{{{'ComplexF32' if self.dtype.kind == 'c' else 'Float32'}}}({self.n} x {self.n})"


def demote(F):
    """A :class:`DemotedFactor` of the plain :class:`FactorNode` ``F`` (``hs_f32_create``): every stored factor element rounded once to
    Float32.  ``F`` must be a handle :func:`ldiv_block_t` serves (:class:`UnsupportedError` otherwise, and when a stored element overflows
    Float32: scale the matrix).  ``F`` is left as it is and may be freed afterwards."""
    if not isinstance(F, FactorNode):
        raise TypeError(f"expected a FactorNode, got {type(F).__name__}")
    h = C.c_void_p()
    _lib.check(_lib.lib().hs_f32_create(F._h, None, C.byref(h)))
    return DemotedFactor(h, F.dtype, F.n)


def ldiv_f32(*args, trans="N"):
    """``ldiv_f32(G, B, trans="N")`` / ``ldiv_f32(C, G, B, trans=...)``: ``C = op(F)^-1 B`` from the Float32 factors of a
    :class:`DemotedFactor` ``G`` (``hs_f32_ldiv_*``), with the shape and dtype rules of :func:`ldiv_block_t`; ``trans`` as in
    :func:`ldiv_mod`.  The result is Float64 / ComplexF64 and carries the rounding of the factors (about ``cond(A) 2^-24`` relative):
    ``gmres_block(A, B, Pr=G)`` recovers full accuracy."""
    if len(args) == 2:
        G, B = args
        Cout = None
    elif len(args) == 3:
        Cout, G, B = args
    else:
        raise TypeError("ldiv_f32(G, B) or ldiv_f32(C, G, B)")
    if not isinstance(G, DemotedFactor):
        raise TypeError(f"expected a DemotedFactor, got {type(G).__name__}")
    if trans not in _MOD_TRANS:
        raise ValueError(f"trans must be None, 'N', 'T', 'C' or 'H', got {trans!r}")
    B = np.asarray(B)
    if B.shape[0] != G.n:
        raise _lib.DimensionMismatch(f"DimensionMismatch: B has {B.shape[0]} rows, F is {G.n} x {G.n}")
    if B.dtype != G.dtype:
        if G.dtype.kind == "f" and B.dtype.kind == "c":
            raise TypeError("MethodError: no method matching ldiv!(::Array{ComplexF64}, ::DemotedFactor{Float32}, ::Array{ComplexF64})")
        B = B.astype(G.dtype)
    vec = B.ndim == 1
    Bm = np.asfortranarray(B.reshape(G.n, -1))
    Cm = np.empty_like(Bm, order="F")
    fn = getattr(_lib.lib(), "hs_f32_ldiv" + ("_z" if G.dtype.kind == "c" else "_d"))
    _lib.check(fn(G._h, _MOD_TRANS[trans], Cm.ctypes.data_as(_lib.p_f64), G.n, Bm.ctypes.data_as(_lib.p_f64), G.n, G.n, Bm.shape[1]))
    res = Cm[:, 0] if vec else Cm
    if Cout is not None:
        Cout[...] = res
        return Cout
    return res


def eigs_info():
    """Figures of this thread's last :func:`eigs` call (``hs_eigs_info``)."""
    out = np.zeros(8)
    _lib.check(_lib.lib().hs_eigs_info(_pf64(out)))
    return {"seconds": float(out[0]), "block_solves": int(out[1]), "column_applications": int(out[2]), "restarts": int(out[3]), "orth_passes": int(out[4]),
            "replaced": int(out[5]), "workspace_bytes": int(out[6]), "ncv": int(out[7])}


def eigs_gen_info():
    """Figures of the generalized part of this thread's last :func:`eigs` call (``hs_eigs_gen_info``): products with ``op(M)``, the columns
    they multiplied, the device bytes held for ``M``, and whether the ``op(M)`` inner product was used."""
    out = np.zeros(4)
    _lib.check(_lib.lib().hs_eigs_gen_info(_pf64(out)))
    return {"m_products": int(out[0]), "m_columns": int(out[1]), "m_bytes": int(out[2]), "inner": "M" if out[3] else "euclid"}


def eigs(F, nev=6, sigma=0.0, ncv=None, block=None, tol=1e-10, maxrestart=100, v0=None, seed=0, vectors=True, log=False, M=None, inner="euclid"):
    """The ``nev`` eigenvalues of ``A`` nearest ``sigma`` and their unit eigenvectors, from the factorization ``F`` of ``A - sigma*I``
    (``hs_eigs_*``): shift-invert block Arnoldi with thick restart, one block solve of ``block`` columns per step.  ``sigma`` is bookkeeping:
    the caller factors the shifted matrix.  ``F`` may be ``transpose(F)`` / ``adjoint(F)``: left eigenvectors (``y^T A = lambda y^T`` /
    ``y^H A = lambda y^H``; the adjoint returns ``conj(lambda)``, the eigenvalues of ``A^H``).

    Returns ``(lam, X)``, nearest first (``X`` is None with ``vectors=False``).  A Float64 factorization returns real arrays unless a
    conjugate pair is among the results; then both are complex, and ``nev + 1`` pairs come back when the ``nev``-th would split a pair.
    ``log=True`` adds a dict: ``resid`` (``||op(A_s) x - (lambda - sigma) x||_2`` with the factored matrix), ``est`` (the Ritz estimates the
    iteration stopped on), ``restarts``, ``nsolves``, ``nconv``, ``seconds``, ``replaced`` (columns replaced after a rank deficiency).
    ``ncv`` (basis columns, ``ncv + block <= 256``), ``block`` (<= 64): None selects the defaults (16, and the multiple of ``block`` at or above
    ``max(2 nev + block, 4 block)``).  ``v0``: an ``n x block`` start block.  Fewer than the wanted pairs within ``tol`` after ``maxrestart``
    restarts raises :class:`NoConvergence`, whose ``partial`` is the tuple that would have been returned (with the log).

    ``M`` (any square ``scipy.sparse`` matrix of order ``n``, in the factored ordering) poses the generalized problem ``A x = lambda M x``
    (``hs_eigs_gen_*``); ``F`` then factors ``A - sigma*M``.  ``M`` is only multiplied with: it may be singular (infinite eigenvalues are
    never returned), non-symmetric, or wider than ``A``'s pattern.  ``transpose(F)`` / ``adjoint(F)`` solve the pencils ``(A^T, M^T)`` /
    ``(A^H, M^H)``.  ``inner="euclid"``: vectors of unit 2-norm, ``est`` as without ``M``.  ``inner="M"`` (Hermitian positive definite
    ``M``): the basis is ``M``-orthonormal, the vectors come back with ``x^H op(M) x = 1`` and ``est`` is measured in the ``M``-norm; an
    ``M`` that is not positive on the start block is a ``ValueError``.  ``resid`` is ``||op(A_s) x - (lambda - sigma) op(M) x||_2`` in both
    modes, and the log gains ``nmprod``, the products with ``op(M)``."""
    F, trans = _unwrap(F)
    n = F.n
    cx = F.dtype.kind == "c"
    if inner not in ("euclid", "M"):
        raise ValueError(f"ArgumentError: eigs: inner = {inner!r} (\"euclid\" or \"M\")")
    Mc = mcolptr = mrowval = None
    if M is not None:
        if not sp.issparse(M):
            raise TypeError(f"eigs: M must be a scipy.sparse matrix, got {type(M).__name__}")
        if M.shape != (n, n):
            raise _lib.DimensionMismatch(f"DimensionMismatch: eigs: M is {M.shape[0]} x {M.shape[1]}, F is {n} x {n}")
        if not cx and M.dtype.kind == "c":
            raise TypeError("MethodError: eigs: a ComplexF64 M for a FactorNode{Float64}")
        Mc = sp.csc_matrix(M, dtype=F.dtype, copy=True)
        Mc.sum_duplicates()
        Mc.sort_indices()
        mcolptr = np.ascontiguousarray(Mc.indptr, dtype=np.int64) + 1
        mrowval = np.ascontiguousarray(Mc.indices, dtype=np.int64) + 1
    sigma = complex(sigma)
    if not cx and sigma.imag != 0.0:
        raise ValueError("ArgumentError: eigs: a complex shift on a Float64 factorization (factor A - sigma*I as ComplexF64)")
    nev = int(nev)
    if nev < 1:
        raise ValueError(f"ArgumentError: eigs: nev = {nev} < 1")
    V0 = None
    if v0 is not None:
        V0 = np.asarray(v0)
        if V0.ndim == 1:
            V0 = V0.reshape(-1, 1)
        if block is None:
            block = V0.shape[1]
        if V0.ndim != 2 or V0.shape != (n, int(block)):
            raise _lib.DimensionMismatch(f"DimensionMismatch: eigs: v0 is {V0.shape}, expected ({n}, {int(block)})")
        if not cx and V0.dtype.kind == "c":
            raise TypeError("MethodError: eigs: a ComplexF64 start block for a FactorNode{Float64}")
        V0 = np.asfortranarray(V0, dtype=F.dtype)
    if block is not None and not 1 <= int(block) <= 64:
        raise ValueError(f"ArgumentError: eigs: block = {block} outside 1:64")
    if ncv is not None and block is not None:  # the library checks the same after filling in its defaults
        if int(ncv) + int(block) > 256:
            raise ValueError(f"ArgumentError: eigs: ncv + block = {int(ncv)} + {int(block)} exceeds the limit of 256 basis columns")
        if int(ncv) < nev + int(block):
            raise ValueError(f"ArgumentError: eigs: ncv = {int(ncv)} < nev + block = {nev} + {int(block)}")
        if n < int(ncv) + int(block):
            raise ValueError(f"ArgumentError: eigs: n = {n} < ncv + block = {int(ncv)} + {int(block)}")
    nx = nev + 1
    lam = np.zeros(2 * nx)
    X = np.zeros((n, nx), dtype=F.dtype, order="F") if vectors else None
    resid, est = np.zeros(nx), np.zeros(nx)
    nout, nconv = _lib.i64(), _lib.i64()
    tail = (nev, int(ncv or 0), int(block or 0), sigma.real, sigma.imag, float(tol), int(maxrestart), V0.ctypes.data_as(C.c_void_p) if V0 is not None else None, max(n, 1),
            int(seed), 0, _pf64(lam), X.ctypes.data_as(C.c_void_p) if vectors else None, max(n, 1), _pf64(resid), _pf64(est), C.byref(nout), C.byref(nconv), None)
    if Mc is None:
        _lib.check(getattr(_lib.lib(), "hs_eigs_z" if cx else "hs_eigs_d")(F._h, trans, n, *tail))
    else:
        mnz = np.ascontiguousarray(Mc.data, dtype=F.dtype)
        _lib.check(getattr(_lib.lib(), "hs_eigs_gen_z" if cx else "hs_eigs_gen_d")(F._h, trans, n, mcolptr.ctypes.data_as(_lib.p_i64), mrowval.ctypes.data_as(_lib.p_i64),
                                                                                  mnz.ctypes.data_as(C.c_void_p), 1 if inner == "M" else 0, *tail))
    k = int(nout.value)
    lamc = lam[0:2 * k:2] + 1j * lam[1:2 * k:2]
    Xo = X[:, :k] if vectors else None
    if not cx:
        if np.any(lamc.imag != 0.0):
            if vectors:  # the pair columns (real part, imaginary part) become the two complex vectors
                Xo = Xo.astype(np.complex128)
                c = 0
                while c < k:
                    if lamc[c].imag != 0.0 and c + 1 < k:
                        xr, xi = X[:, c], X[:, c + 1]
                        Xo[:, c], Xo[:, c + 1] = xr + 1j * xi, xr - 1j * xi
                        c += 2
                    else:
                        c += 1
        else:
            lamc = lamc.real.copy()
    res = (lamc, Xo)
    if log or nconv.value < k:
        info = eigs_info()
        res = res + ({"resid": resid[:k].copy(), "est": est[:k].copy(), "restarts": info["restarts"], "nsolves": info["block_solves"], "nconv": int(nconv.value),
                      "seconds": info["seconds"], "replaced": info["replaced"], "ncv": info["ncv"], "nmprod": eigs_gen_info()["m_products"]},)
    if nconv.value < k:
        raise _lib.NoConvergence(f"eigs: {int(nconv.value)} of {k} eigenpairs within tol = {tol:g} after {res[2]['restarts']} restarts", partial=res)
    return res


def _sparse_rhs(F, B):
    """``(F, trans, raw handle, B as canonical CSC, 1-based colptr, 1-based rowval)`` for the ``hs_ldiv_sparse_*`` calls."""
    trans = 0
    if isinstance(F, TransposedFactor):
        F, trans = F.parent, F.trans
    h = F._h if isinstance(F, FactorNode) else F  # a raw handle: dist.plan_only
    n = F.n if isinstance(F, FactorNode) else int(_lib.lib().hs_size(h))
    if not sp.issparse(B):
        raise TypeError(f"expected a scipy.sparse matrix, got {type(B).__name__}")
    if B.shape[0] != n:
        raise _lib.DimensionMismatch(f"DimensionMismatch: B has {B.shape[0]} rows, F is {n} x {n}")
    B = sp.csc_matrix(B, copy=True)
    B.sum_duplicates()
    B.sort_indices()
    colptr = np.ascontiguousarray(B.indptr, dtype=np.int64) + 1
    rowval = np.ascontiguousarray(B.indices, dtype=np.int64) + 1
    return F, trans, h, n, B, colptr, rowval


def _wanted_rows(rows, n):
    if rows is None:
        return None
    rows = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int64)
    if rows.size and (rows.min() < 0 or rows.max() >= n):
        raise _lib.DimensionMismatch(f"BoundsError: rows outside 0:{n - 1}")
    return rows + 1


def ldiv_sparse(F, B, rows=None):
    """``(F \\ B)[rows, :]`` for a sparse ``B`` (``hs_ldiv_sparse_*``): ``B`` is any ``scipy.sparse`` matrix with ``n`` rows (converted to canonical
    CSC: duplicates summed, indices sorted), ``F`` a :class:`FactorNode`, ``transpose(F)`` or ``adjoint(F)``, ``rows`` a 0-based integer
    array (any order, repeats allowed) or ``None`` for all rows.  Returns a dense ``len(rows) x nrhs`` array (``n x nrhs`` for ``None``).
    The forward sweep of a chunk of columns visits only the fronts that own a stored row of ``B`` and their ancestors, the backward sweep
    only the fronts that own a wanted row and their ancestors; the result equals ``ldiv_block_t(F, B.toarray())[rows]`` bit for bit.
    Indices refer to the factored (already permuted) matrix.  Dtype rules and refusals are those of :func:`ldiv_block`."""
    F, trans, h, n, B, colptr, rowval = _sparse_rhs(F, B)
    if not isinstance(F, FactorNode):
        raise TypeError(f"expected a FactorNode, got {type(F).__name__}")
    if B.dtype != F.dtype:
        if F.dtype.kind == "f" and B.dtype.kind == "c":
            raise TypeError("MethodError: no method matching ldiv!(::Array{ComplexF64}, ::FactorNode{Float64}, ::SparseMatrixCSC{ComplexF64})")
        B = B.astype(F.dtype)
    vals = np.ascontiguousarray(B.data, dtype=F.dtype)
    rows1 = _wanted_rows(rows, n)
    nout = n if rows1 is None else len(rows1)
    X = np.zeros((nout, B.shape[1]), dtype=F.dtype, order="F")
    L = _lib.lib()
    fn = L.hs_ldiv_sparse_z if F.dtype.kind == "c" else L.hs_ldiv_sparse_d
    _lib.check(fn(h, trans, n, B.shape[1], _p64(colptr), _p64(rowval), vals.ctypes.data_as(_lib.p_f64), None if rows1 is None else _p64(rows1), nout,
                  X.ctypes.data_as(_lib.p_f64), max(nout, 1)))
    return X


def _num_nodes(h):
    """Node ids of the C ABI on this handle: the user's tree, and the pseudo-root when the root keeps a boundary."""
    st = _lib.hs_stats()
    _lib.check(_lib.lib().hs_get_stats(h, C.byref(st)))
    nn = int(st.nnodes)
    return nn + 1 if _lib.lib().hs_node_info(h, nn, None, None, None) == _lib.HS_OK else nn


def ldiv_sparse_plan(F, B, rows=None):
    """What ``ldiv_sparse(F, B, rows)`` would visit (``hs_ldiv_sparse_plan``; host work only, ``F`` may also be the handle of
    ``dist.plan_only``): ``order`` (the processing order, 0-based column ids), ``nchunks``, and ``active[chunk, node]`` with bit 0 = the
    forward sweep of the chunk visits the node, bit 1 = the backward sweep does (node ids of the tree in post-order)."""
    F, trans, h, n, B, colptr, rowval = _sparse_rhs(F, B)
    rows1 = _wanted_rows(rows, n)
    nr = 0 if rows1 is None else len(rows1)
    pr = None if rows1 is None else _p64(rows1)
    L = _lib.lib()
    order = np.zeros(B.shape[1], dtype=np.int64)
    nch = _lib.i64(0)
    _lib.check(L.hs_ldiv_sparse_plan(h, trans, n, B.shape[1], _p64(colptr), _p64(rowval), pr, nr, _p64(order), C.byref(nch), None))
    nn = _num_nodes(h)
    active = np.zeros((nch.value, nn), dtype=np.uint8)
    if active.size:
        _lib.check(L.hs_ldiv_sparse_plan(h, trans, n, B.shape[1], _p64(colptr), _p64(rowval), pr, nr, None, None, active.ctypes.data_as(C.POINTER(C.c_uint8))))
    return {"order": order, "nchunks": int(nch.value), "active": active}


def ldiv_sparse_info(F):
    """Figures of the last :func:`ldiv_sparse` call on ``F`` (``hs_ldiv_sparse_info``): device seconds, factor bytes read by the model (per chunk
    and sweep ``(ni^2 / 2 + ni nb) sizeof(T)`` over the visited fronts), front visits of the forward and of the backward sweeps, fronts x
    chunks (what a dense block solve visits per sweep), chunks, values moved between host and device, workspace bytes."""
    F, _ = _unwrap(F)
    out = np.zeros(8)
    _lib.check(_lib.lib().hs_ldiv_sparse_info(F._h, _pf64(out)))
    return {"seconds": float(out[0]), "factor_bytes": float(out[1]), "visits_forward": int(out[2]), "visits_backward": int(out[3]),
            "visits_dense": int(out[4]), "chunks": int(out[5]), "values_moved": int(out[6]), "workspace_bytes": int(out[7])}


def _sens_handle(F):
    """``(FactorNode or None, trans, raw handle, n, dtype)``: ``F`` may also be the raw handle of ``dist.plan_only`` (refusal tests)."""
    trans = 0
    if isinstance(F, TransposedFactor):
        F, trans = F.parent, F.trans
    if isinstance(F, FactorNode):
        return F, trans, F._h, F.n, F.dtype
    L = _lib.lib()
    return None, trans, F, int(L.hs_size(F)), np.dtype(np.complex128 if L.hs_is_complex(F) else np.float64)


def _sens_block(name, M, n, dtype, ncols=None):
    """A dense array or ``scipy.sparse`` matrix as an ``hs_block_arg``; returns ``(arg, nrhs, keep-alive objects)``."""
    if sp.issparse(M):
        if M.shape[0] != n:
            raise _lib.DimensionMismatch(f"DimensionMismatch: {name} has {M.shape[0]} rows, F is {n} x {n}")
        if M.dtype != dtype:
            if dtype.kind == "f" and M.dtype.kind == "c":
                raise TypeError(f"MethodError: no method matching sensitivity(::FactorNode{{Float64}}, {name}::SparseMatrixCSC{{ComplexF64}})")
            M = M.astype(dtype)
        M = sp.csc_matrix(M, copy=True)
        M.sum_duplicates()
        M.sort_indices()
        colptr = np.ascontiguousarray(M.indptr, dtype=np.int64) + 1
        rowval = np.ascontiguousarray(M.indices, dtype=np.int64) + 1
        vals = np.ascontiguousarray(M.data, dtype=dtype)
        arg = _lib.hs_block_arg(None, 0, _p64(colptr), _p64(rowval), vals.ctypes.data)
        nrhs, keep = M.shape[1], (colptr, rowval, vals)
    else:
        M = np.asarray(M)
        if M.ndim == 1:
            M = M.reshape(-1, 1)
        if M.ndim != 2 or M.shape[0] != n:
            raise _lib.DimensionMismatch(f"DimensionMismatch: {name} has {M.shape[0] if M.ndim else 0} rows, F is {n} x {n}")
        if M.dtype != dtype:
            if dtype.kind == "f" and M.dtype.kind == "c":
                raise TypeError(f"MethodError: no method matching sensitivity(::FactorNode{{Float64}}, {name}::Array{{ComplexF64}})")
            M = M.astype(dtype)
        M = np.asfortranarray(M)
        arg = _lib.hs_block_arg(M.ctypes.data, max(n, 1), None, None, None)
        nrhs, keep = M.shape[1], (M,)
    if ncols is not None and nrhs != ncols:
        raise _lib.DimensionMismatch(f"DimensionMismatch: {name} has {nrhs} columns, B has {ncols}")
    return arg, nrhs, keep


def _sens_pattern(pattern):
    if pattern in ("A", 0):
        return 0
    if pattern in ("diag", 1):
        return 1
    raise ValueError(f"ArgumentError: pattern must be 'A' or 'diag', not {pattern!r}")


def _sens_len(F, h, n, pcode):
    if pcode == 1:
        return n
    if F is not None and F._pattern is not None:
        return len(F._pattern[1])
    return 0  # a raw handle: only the refusals are reachable


def sensitivity(F, B, W, itmax=0, pattern="A", want=()):
    """Adjoint-state sensitivity of a real objective on the pattern of the factored matrix ``A`` (``hs_sens_*``).  ``F`` is a
    :class:`FactorNode`, ``transpose(F)`` or ``adjoint(F)``: with ``op(A)`` accordingly, ``X = op(A)^-1 B`` and ``W`` the cotangent
    (``dJ = Re<W, dX>``), ``Lam = op(A)^-H W`` and the result ``G`` satisfies, for any ``E`` on the pattern of ``A``,
    ``d/ds Re<W, op(A + sE)^-1 B> = Re sum(E.data * conj(G))`` at ``s = 0`` -- e.g. ``G_ij = -sum_c Lam_ic conj(X_jc)`` for a plain ``F``.
    ``B`` and ``W`` are dense ``n x k`` arrays or ``scipy.sparse`` matrices (sparse blocks take the pruned sweeps of :func:`ldiv_sparse` and
    give the bits of their dense expansion).  ``G`` is a 1-D array aligned with the ``data`` of the factored matrix (CSC, sorted indices;
    :func:`sensitivity_matrix` wraps it), or of length ``n`` for ``pattern="diag"``.  ``itmax > 0`` solves both systems through
    :func:`ldiv_refine_block` (compressed factorizations).  ``want`` may name ``"X"`` and ``"Lam"``: the result is then
    ``(G, X, Lam)`` restricted to what was asked for, in that order.  Nothing but ``G`` and the requested blocks leaves the device.
    Dtype rules and error classes are those of :func:`ldiv_block`."""
    Fn, trans, h, n, dtype = _sens_handle(F)
    pcode = _sens_pattern(pattern)
    want = (want,) if isinstance(want, str) else tuple(want)
    for w in want:
        if w not in ("X", "Lam"):
            raise ValueError(f"ArgumentError: want may name 'X' and 'Lam', not {w!r}")
    if int(itmax) != itmax:
        raise TypeError("itmax must be an integer")
    argB, k, keepB = _sens_block("B", B, n, dtype)
    argW, _, keepW = _sens_block("W", W, n, dtype, k)
    G = np.zeros(_sens_len(Fn, h, n, pcode), dtype=dtype)
    X = np.zeros((n, k), dtype=dtype, order="F") if "X" in want else None
    Lam = np.zeros((n, k), dtype=dtype, order="F") if "Lam" in want else None
    L = _lib.lib()
    fn = L.hs_sens_z if dtype.kind == "c" else L.hs_sens_d
    _lib.check(fn(h, trans, n, k, C.byref(argB), C.byref(argW), int(itmax), pcode, G.ctypes.data, None if X is None else X.ctypes.data, max(n, 1),
                  None if Lam is None else Lam.ctypes.data, max(n, 1)))
    del keepB, keepW
    out = (G,) + ((X,) if X is not None else ()) + ((Lam,) if Lam is not None else ())
    return out[0] if len(out) == 1 else out


def sensitivity_matrix(F, G):
    """``G`` of :func:`sensitivity` / :func:`misfit` (``pattern="A"``) as a ``scipy.sparse.csc_matrix`` on the pattern of the factored matrix."""
    F, _ = _unwrap(F)
    if F._pattern is None:
        raise ValueError("ArgumentError: this FactorNode does not know the pattern of its matrix")
    G = np.asarray(G)
    if G.shape != (len(F._pattern[1]),):
        raise _lib.DimensionMismatch(f"DimensionMismatch: G has shape {G.shape}, the factored matrix stores {len(F._pattern[1])} entries")
    return sp.csc_matrix((G.copy(), F._pattern[1].copy(), F._pattern[0].copy()), shape=(F.n, F.n))


def misfit(F, B, rows, D, itmax=0, pattern="A", want_residual=False):
    """Least-squares misfit at receiver rows and its sensitivity (``hs_misfit_*``): with ``X = op(A)^-1 B``, ``R = X[rows, :] - D``
    (``rows``: distinct 0-based indices, any order; ``D``: ``len(rows) x k``), ``J[c] = 0.5 ||R[:, c]||^2`` and ``G`` the sensitivity of
    ``sum(J)`` as :func:`sensitivity` defines it for ``W = R`` scattered to ``rows``.  The cotangent is built on the device and is sparse, so
    the adjoint solve takes the pruned path.  Returns ``(J, G)`` or, with ``want_residual``, ``(J, G, R)``.  Repeated rows raise
    ``ValueError`` (ArgumentError)."""
    Fn, trans, h, n, dtype = _sens_handle(F)
    pcode = _sens_pattern(pattern)
    if int(itmax) != itmax:
        raise TypeError("itmax must be an integer")
    argB, k, keepB = _sens_block("B", B, n, dtype)
    rows = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int64)
    if rows.size and (rows.min() < 0 or rows.max() >= n):
        raise _lib.DimensionMismatch(f"BoundsError: rows outside 0:{n - 1}")
    rows1 = rows + 1
    nr = len(rows1)
    D = np.asarray(D)
    if D.ndim == 1:
        D = D.reshape(-1, 1)
    if D.shape != (nr, k):
        raise _lib.DimensionMismatch(f"DimensionMismatch: D has shape {D.shape}, expected {(nr, k)}")
    if D.dtype != dtype:
        if dtype.kind == "f" and D.dtype.kind == "c":
            raise TypeError("MethodError: no method matching misfit(::FactorNode{Float64}, D::Array{ComplexF64})")
        D = D.astype(dtype)
    D = np.asfortranarray(D)
    G = np.zeros(_sens_len(Fn, h, n, pcode), dtype=dtype)
    J = np.zeros(k)
    R = np.zeros((nr, k), dtype=dtype, order="F") if want_residual else None
    L = _lib.lib()
    fn = L.hs_misfit_z if dtype.kind == "c" else L.hs_misfit_d
    _lib.check(fn(h, trans, n, k, C.byref(argB), _p64(rows1), nr, D.ctypes.data, max(nr, 1), int(itmax), pcode, J.ctypes.data,
                  None if R is None else R.ctypes.data, max(nr, 1), G.ctypes.data))
    del keepB
    return (J, G, R) if want_residual else (J, G)


def sens_info(F):
    """Figures of the last :func:`sensitivity` / :func:`misfit` call on ``F`` (``hs_sens_info``): device seconds in total, of the forward
    solves, of the adjoint solves and of the reduction (staging included), column groups, stored entries x columns reduced, values moved
    between host and device, workspace bytes."""
    F, _ = _unwrap(F)
    out = np.zeros(8)
    _lib.check(_lib.lib().hs_sens_info(F._h, _pf64(out)))
    return {"seconds": float(out[0]), "seconds_forward": float(out[1]), "seconds_adjoint": float(out[2]), "seconds_reduce": float(out[3]),
            "groups": int(out[4]), "products": int(out[5]), "values_moved": int(out[6]), "workspace_bytes": int(out[7])}


def _gn_inputs(fname, F, B, X, itmax, pattern):
    """The arguments :func:`tangent`, :func:`gn_hessvec` and :func:`gn_diag` share: ``(Fn, trans, h, n, dtype, pcode, argB or None, k, Xin or
    None, keep-alive objects)``.  ``X`` (the fields of an earlier call) replaces ``B``, which may then be ``None``."""
    Fn, trans, h, n, dtype = _sens_handle(F)
    pcode = _sens_pattern(pattern)
    if int(itmax) != itmax:
        raise TypeError("itmax must be an integer")
    if B is None and X is None:
        raise ValueError(f"ArgumentError: {fname}: B and X are both None")
    argB, k, keep, Xin = None, None, (), None
    if B is not None:
        argB, k, keep = _sens_block("B", B, n, dtype)
    if X is not None:
        Xin = np.asarray(X)
        if Xin.ndim == 1:
            Xin = Xin.reshape(-1, 1)
        if Xin.ndim != 2 or Xin.shape[0] != n or (k is not None and Xin.shape[1] != k):
            raise _lib.DimensionMismatch(f"DimensionMismatch: X has shape {Xin.shape}, expected {(n, k if k is not None else Xin.shape[-1])}")
        if Xin.dtype != dtype:
            if dtype.kind == "f" and Xin.dtype.kind == "c":
                raise TypeError(f"MethodError: no method matching {fname}(::FactorNode{{Float64}}, X::Array{{ComplexF64}})")
            Xin = Xin.astype(dtype)
        Xin = np.asfortranarray(Xin)
        k = Xin.shape[1]
    return Fn, trans, h, n, dtype, pcode, argB, k, Xin, keep


def _gn_direction(fname, E, length, dtype):
    E = np.asarray(E).reshape(-1)
    if E.shape != (length,):
        raise _lib.DimensionMismatch(f"DimensionMismatch: E has {E.size} values, expected {length}")
    if E.dtype != dtype:
        if dtype.kind == "f" and E.dtype.kind == "c":
            raise TypeError(f"MethodError: no method matching {fname}(::FactorNode{{Float64}}, E::Vector{{ComplexF64}})")
        E = E.astype(dtype)
    return np.ascontiguousarray(E)


def _gn_rows(rows, n):
    rows = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int64)
    if rows.size and (rows.min() < 0 or rows.max() >= n):
        raise _lib.DimensionMismatch(f"BoundsError: rows outside 0:{n - 1}")
    return rows + 1


def _gn_want(want, allowed):
    want = (want,) if isinstance(want, str) else tuple(want)
    for w in want:
        if w not in allowed:
            raise ValueError("ArgumentError: want may name " + " and ".join(repr(a) for a in allowed) + f", not {w!r}")
    return want


def tangent(F, B, E, rows=None, itmax=0, pattern="A", X=None, want=()):
    """Tangent-linear (Born) solve (``hs_tangent_*``): with ``op(A)`` as in :func:`sensitivity`, ``X = op(A)^-1 B`` and ``E`` a perturbation of
    the stored entries of ``A`` (aligned with the ``data`` of the factored matrix; ``n`` diagonal values for ``pattern="diag"``), returns
    ``dX = d/ds op(A + sE)^-1 B`` at ``s = 0``, i.e. ``-op(A)^-1 op(E) X``: ``n x k``, or the rows ``rows`` (distinct 0-based indices, any
    order) of it.  It is the forward mode of :func:`sensitivity`: ``Re<W, dX> = Re sum(E * conj(G))`` for that function's ``G``.  ``X=`` takes
    the fields of an earlier call (``want="X"``) and skips the forward solve; ``B`` may then be ``None``.  ``want`` may name ``"X"``: the result
    is then ``(dX, X)``.  Blocks, dtype rules and error classes are those of :func:`sensitivity`."""
    Fn, trans, h, n, dtype, pcode, argB, k, Xin, keep = _gn_inputs("tangent", F, B, X, itmax, pattern)
    want = _gn_want(want, ("X",))
    E = _gn_direction("tangent", E, _sens_len(Fn, h, n, pcode), dtype)
    rows1 = None if rows is None else _gn_rows(rows, n)
    m = n if rows1 is None else len(rows1)
    rbuf = None if rows1 is None else (rows1 if m else np.zeros(1, dtype=np.int64))  # an empty list is still a list: never a null pointer
    dX = np.zeros((m, k), dtype=dtype, order="F")
    Xo = np.zeros((n, k), dtype=dtype, order="F") if "X" in want else None
    L = _lib.lib()
    fn = L.hs_tangent_z if dtype.kind == "c" else L.hs_tangent_d
    _lib.check(fn(h, trans, n, k, None if argB is None else C.byref(argB), None if Xin is None else Xin.ctypes.data, max(n, 1), E.ctypes.data, pcode, int(itmax),
                  None if rbuf is None else _p64(rbuf), 0 if rows1 is None else m, dX.ctypes.data, max(m, 1), None if Xo is None else Xo.ctypes.data, max(n, 1)))
    del keep
    return (dX, Xo) if Xo is not None else dX


def gn_hessvec(F, B, rows, E, itmax=0, pattern="A", X=None, want=()):
    """Gauss-Newton Hessian-vector product of the least-squares misfit at the receiver rows ``rows`` (``hs_gn_hessvec_*``): with
    ``J E = tangent(F, B, E, rows)``, returns ``H E = J* J E`` (the adjoint in the real inner product), which is the ``G`` of
    :func:`sensitivity` for ``W = J E`` scattered to ``rows`` -- aligned with the ``data`` of the factored matrix like ``E``
    (:func:`sensitivity_matrix` wraps it), or of length ``n`` for ``pattern="diag"``.  ``Re<E1, H E2> = Re<J E1, J E2>``.  ``X=`` takes the
    fields of an earlier call and skips the forward solve: a product then costs two block solves instead of three (a CG loop on a fixed ``A``
    and ``B`` asks for ``want="X"`` once).  ``want`` may name ``"JE"`` and ``"X"``: the result is then ``(HE, JE, X)`` restricted to what
    was asked for, in that order.  Nothing else of size ``n x k`` leaves the device."""
    Fn, trans, h, n, dtype, pcode, argB, k, Xin, keep = _gn_inputs("gn_hessvec", F, B, X, itmax, pattern)
    want = _gn_want(want, ("JE", "X"))
    E = _gn_direction("gn_hessvec", E, _sens_len(Fn, h, n, pcode), dtype)
    rows1 = _gn_rows(rows, n)
    nr = len(rows1)
    HE = np.zeros(len(E), dtype=dtype)
    JE = np.zeros((nr, k), dtype=dtype, order="F") if "JE" in want else None
    Xo = np.zeros((n, k), dtype=dtype, order="F") if "X" in want else None
    L = _lib.lib()
    fn = L.hs_gn_hessvec_z if dtype.kind == "c" else L.hs_gn_hessvec_d
    _lib.check(fn(h, trans, n, k, None if argB is None else C.byref(argB), None if Xin is None else Xin.ctypes.data, max(n, 1), E.ctypes.data, pcode, int(itmax),
                  _p64(rows1), nr, HE.ctypes.data, None if JE is None else JE.ctypes.data, max(nr, 1), None if Xo is None else Xo.ctypes.data, max(n, 1)))
    del keep
    out = (HE,) + ((JE,) if JE is not None else ()) + ((Xo,) if Xo is not None else ())
    return out[0] if len(out) == 1 else out


def gn_diag(F, B, rows, itmax=0, pattern="A", X=None, factors=False):
    """Diagonal of the Gauss-Newton Hessian of :func:`gn_hessvec` (``hs_gn_diag_*``), the usual preconditioner of a Gauss-Newton loop: a real
    array aligned with the ``data`` of the factored matrix (length ``n`` for ``pattern="diag"``), ``Hd[p] = z2[a] * x2[b]`` for the stored
    entry ``p = (i, j)`` with ``(a, b) = (i, j)`` for a plain ``F`` and ``(j, i)`` for ``transpose(F)`` / ``adjoint(F)``, where
    ``x2 = sum(|X|^2, axis=1)`` and ``z2 = sum(|Z|^2, axis=1)`` for the adjoint states ``Z = op(A)^-H S`` of the unit columns of ``rows``.
    Costs one forward block solve (none with ``X=``) and ``len(rows)`` adjoint columns on the pruned path.  ``factors=True`` returns
    ``(Hd, z2, x2)``."""
    Fn, trans, h, n, dtype, pcode, argB, k, Xin, keep = _gn_inputs("gn_diag", F, B, X, itmax, pattern)
    rows1 = _gn_rows(rows, n)
    nr = len(rows1)
    Hd = np.zeros(_sens_len(Fn, h, n, pcode))
    z2, x2 = (np.zeros(n), np.zeros(n)) if factors else (None, None)
    L = _lib.lib()
    fn = L.hs_gn_diag_z if dtype.kind == "c" else L.hs_gn_diag_d
    _lib.check(fn(h, trans, n, k, None if argB is None else C.byref(argB), None if Xin is None else Xin.ctypes.data, max(n, 1), _p64(rows1), nr, pcode, int(itmax),
                  Hd.ctypes.data, None if z2 is None else z2.ctypes.data, None if x2 is None else x2.ctypes.data))
    del keep
    return (Hd, z2, x2) if factors else Hd


def gn_info(F):
    """Figures of the last :func:`tangent` / :func:`gn_hessvec` / :func:`gn_diag` call on ``F`` (``hs_gn_info``): device seconds in total, of
    the forward, tangent and adjoint solves and of the products and reductions, column groups, block solves issued, workspace bytes."""
    F, _ = _unwrap(F)
    out = np.zeros(8)
    _lib.check(_lib.lib().hs_gn_info(F._h, _pf64(out)))
    return {"seconds": float(out[0]), "seconds_forward": float(out[1]), "seconds_tangent": float(out[2]), "seconds_adjoint": float(out[3]),
            "seconds_products": float(out[4]), "groups": int(out[5]), "block_solves": int(out[6]), "workspace_bytes": int(out[7])}


def _block_cols():
    """Columns per chunk of the block solves: the library's reading of ``HS_LDIV_BLOCK_COLS``."""
    try:
        v = int(os.environ.get("HS_LDIV_BLOCK_COLS", "32"))
    except ValueError:
        v = 32
    return v if v in (16, 32, 48, 64) else 32


def inv_entries(F, I, J):
    """``(A^-1)[I[k], J[k]]`` for arbitrary 0-based index pairs -- entries of the inverse outside the pattern of ``A`` too, which
    :func:`selinv` does not give -- by :func:`ldiv_sparse` on unit columns: the distinct ``J`` become unit right-hand sides, the library
    orders them so that the columns of a chunk are neighbours in the tree, and each group of ``HS_LDIV_BLOCK_COLS`` columns asks for the
    union of its ``I`` only.  ``transpose(F)`` / ``adjoint(F)`` give the entries of ``(A^T)^-1`` / ``(A^H)^-1``.  On a compressed
    factorization the result is the entry of the approximate inverse the factors define.  The cost follows the number of distinct
    columns: with few distinct rows and many columns ask the transposed form, ``inv_entries(transpose(F), J, I)`` (conjugate it for a
    ComplexF64 ``adjoint``), which solves for the few rows instead.  Indices refer to the factored (already permuted) matrix."""
    Fn, _ = _unwrap(F)
    n = Fn.n
    I = np.asarray(I, dtype=np.int64).reshape(-1)
    J = np.asarray(J, dtype=np.int64).reshape(-1)
    if I.shape != J.shape:
        raise _lib.DimensionMismatch(f"DimensionMismatch: {len(I)} row and {len(J)} column indices")
    for a in (I, J):
        if a.size and (a.min() < 0 or a.max() >= n):
            raise _lib.DimensionMismatch(f"BoundsError: index outside 0:{n - 1}")
    out = np.zeros(len(I), dtype=Fn.dtype)
    if not len(I):
        return out
    cols, cid = np.unique(J, return_inverse=True)
    E = sp.csc_matrix((np.ones(len(cols), dtype=Fn.dtype), cols, np.arange(len(cols) + 1)), shape=(n, len(cols)))
    order = ldiv_sparse_plan(F, E, rows=I[:1])["order"]
    by_col = np.argsort(cid, kind="stable")  # the pairs of column c: by_col[start[c]:start[c + 1]]
    start = np.searchsorted(cid[by_col], np.arange(len(cols) + 1))
    kc = _block_cols()
    for g0 in range(0, len(cols), kc):
        grp = order[g0:g0 + kc]
        pairs = np.concatenate([by_col[start[c]:start[c + 1]] for c in grp])
        rows, rid = np.unique(I[pairs], return_inverse=True)
        X = ldiv_sparse(F, E[:, grp], rows)
        pos = np.empty(len(cols), dtype=np.int64)
        pos[grp] = np.arange(len(grp))
        out[pairs] = X[rid, pos[cid[pairs]]]
    return out


def maxrank(F):
    """``maxrank(F)`` (factornode.jl:49-57)."""
    return int(_lib.lib().hs_maxrank(F._h))


def _unwrap(F):
    """``(FactorNode, trans)`` of ``F``, ``transpose(F)`` or ``adjoint(F)``."""
    if isinstance(F, TransposedFactor):
        return F.parent, F.trans
    if not isinstance(F, FactorNode):
        raise TypeError(f"expected a FactorNode, got {type(F).__name__}")
    return F, 0


def ulv_mode(F, on=None):
    """The per-handle switch ``hs_ulv_mode``: with ``on=True`` :func:`gmres_block`, :func:`gmres`, :func:`ldiv_refine`,
    :func:`ldiv_refine_block`, :func:`opnormestinv`, :func:`condest`, :func:`sensitivity` / :func:`misfit` (dense blocks) and
    :func:`logabsdet` serve a handle whose fronts keep their interior block ``D`` as an HSS matrix (``hss_d``, ``mf = 2, 3``) through
    the ULV block solve of :func:`ldiv_ulv`; with ``on=False`` (the default state of a handle) they refuse it as before.  A handle without
    such fronts is not affected.  ``on=None`` only queries.  Returns the previous setting.  ``F``, ``transpose(F)`` and ``adjoint(F)``
    are views of one handle and share the setting; do not change it while another thread is inside a call on that handle."""
    F, _ = _unwrap(F)
    mode = -1 if on is None else (1 if on else 0)
    prev = int(_lib.lib().hs_ulv_mode(F._h, mode))
    if prev < 0:
        _lib.check(prev)
    return bool(prev)


def _pcode(p):
    if p == 1:
        return 1
    if p in (np.inf, "inf", "Inf"):
        return 0
    raise ValueError(f"ArgumentError: p must be 1 or Inf, not {p!r}")


def opnorm(F, p=1):
    """``opnorm(A, p)``, p = 1 or ``np.inf``, of the matrix ``F`` factors (the values of its last numeric factorization), computed on the
    device (``hs_opnorm``).  For ``transpose(F)`` / ``adjoint(F)``: the norm of ``A^T`` / ``A^H``."""
    F, trans = _unwrap(F)
    pc = _pcode(p)
    if trans:
        pc = 1 - pc  # ||A^T||_1 = ||A||_Inf
    out = C.c_double()
    _lib.check(_lib.lib().hs_opnorm(F._h, pc, C.byref(out)))
    return out.value


def opnormestinv(F, t=2, itmax=5, nsolves=False):
    """Julia's ``opnormestinv``: a lower bound of ``||op(F)^-1||_1`` (usually within a factor of 3) by the Higham-Tisseur block 1-norm
    estimator with ``t`` columns (``t`` is clipped to ``n`` like Julia's ``min(2, n)``).  ``F`` may be ``transpose(F)`` or ``adjoint(F)``.
    ``nsolves=True`` returns ``(est, columns solved)``."""
    F, trans = _unwrap(F)
    t = min(int(t), F.n)
    est, ns = C.c_double(), _lib.i64()
    _lib.check(_lib.lib().hs_normestinv(F._h, trans, t, int(itmax), C.byref(est), C.byref(ns), None))
    return (est.value, ns.value) if nsolves else est.value


def condest(F, p=1, t=2):
    """``cond(A, p) ~ opnorm(A, p) * opnormestinv``, p = 1 or ``np.inf`` (``hs_condest``).  For a compressed factorization this estimates
    cond(A) only as well as F approximates A.  ``condest(transpose(F), p)`` is the estimate for ``A^T``."""
    F, trans = _unwrap(F)
    pc = _pcode(p)
    if trans:
        pc = 1 - pc  # cond_1(A^T) = cond_Inf(A)
    t = min(int(t), F.n)
    out = C.c_double()
    _lib.check(_lib.lib().hs_condest(F._h, pc, t, C.byref(out), None, None, None))
    return out.value


def ldiv_refine(F, B, itmax=5, ferr=True):
    """LAPACK xGERFS on ``op(A) X = B`` (``op`` by ``F``, ``transpose(F)`` or ``adjoint(F)``): ``X = op(F) \\ B``, then iterative refinement
    with the residual of A itself, at most ``itmax`` corrections (``hs_ldiv_refine_*``).  Returns ``(X, berr, ferr, steps)``: the componentwise
    backward error, the forward error bound (None with ``ferr=False``) and the corrections made, per column (scalars for a vector B)."""
    F, trans = _unwrap(F)
    B = np.asarray(B)
    if B.shape[0] != F.n:
        raise _lib.DimensionMismatch(f"DimensionMismatch: B has {B.shape[0]} rows, F is {F.n} x {F.n}")
    if B.dtype != F.dtype:
        if F.dtype.kind == "f" and B.dtype.kind == "c":
            raise TypeError("MethodError: no method matching ldiv_refine(::FactorNode{Float64}, ::Array{ComplexF64})")
        B = B.astype(F.dtype)
    vec = B.ndim == 1
    Bm = np.asfortranarray(B.reshape(F.n, -1))
    k = Bm.shape[1]
    X = np.empty_like(Bm, order="F")
    be = np.zeros(k)
    fe = np.zeros(k) if ferr else None
    st = np.zeros(k, dtype=np.int64)
    L = _lib.lib()
    fn = L.hs_ldiv_refine_z if F.dtype.kind == "c" else L.hs_ldiv_refine_d
    _lib.check(fn(F._h, trans, X.ctypes.data_as(_lib.p_f64), F.n, Bm.ctypes.data_as(_lib.p_f64), F.n, F.n, k, int(itmax), _pf64(be),
                  _pf64(fe) if ferr else None, _p64(st)))
    if vec:
        return X[:, 0], float(be[0]), (float(fe[0]) if ferr else None), int(st[0])
    return X, be, fe, st


def ldiv_refine_block(F, B, itmax=5, ferr=True):
    """:func:`ldiv_refine` for a block of right-hand sides in lockstep (``hs_ldiv_refine_block_*``): the same arguments and return shapes,
    every column the same xGERFS iteration and error bounds, but all active columns take a correction together through one block solve
    (:func:`ldiv_block_t`), so the factors are read once per chunk of columns and not once per column.  Results agree with
    :func:`ldiv_refine` to the rounding by which block and single solves differ.  Handles the block solve refuses (HSS interior blocks,
    more than one rank) raise :class:`UnsupportedError`."""
    F, trans = _unwrap(F)
    B = np.asarray(B)
    if B.shape[0] != F.n:
        raise _lib.DimensionMismatch(f"DimensionMismatch: B has {B.shape[0]} rows, F is {F.n} x {F.n}")
    if B.dtype != F.dtype:
        if F.dtype.kind == "f" and B.dtype.kind == "c":
            raise TypeError("MethodError: no method matching ldiv_refine_block(::FactorNode{Float64}, ::Array{ComplexF64})")
        B = B.astype(F.dtype)
    vec = B.ndim == 1
    Bm = np.asfortranarray(B.reshape(F.n, -1))
    k = Bm.shape[1]
    X = np.empty_like(Bm, order="F")
    be = np.zeros(k)
    fe = np.zeros(k) if ferr else None
    st = np.zeros(k, dtype=np.int64)
    L = _lib.lib()
    fn = L.hs_ldiv_refine_block_z if F.dtype.kind == "c" else L.hs_ldiv_refine_block_d
    _lib.check(fn(F._h, trans, X.ctypes.data_as(_lib.p_f64), F.n, Bm.ctypes.data_as(_lib.p_f64), F.n, F.n, k, int(itmax), _pf64(be),
                  _pf64(fe) if ferr else None, _p64(st)))
    if vec:
        return X[:, 0], float(be[0]), (float(fe[0]) if ferr else None), int(st[0])
    return X, be, fe, st


def ldiv_refine_block_info():
    """Figures of this thread's last :func:`ldiv_refine_block` call (``hs_ldiv_refine_block_info``)."""
    out = np.zeros(8)
    _lib.check(_lib.lib().hs_ldiv_refine_block_info(_pf64(out)))
    return {"seconds": float(out[0]), "block_solves": int(out[1]), "column_applications": int(out[2]), "residual_launches": int(out[3]),
            "max_active": int(out[4]), "groups": int(out[5]), "workspace_bytes": int(out[6]), "estimator_column_applications": int(out[7])}


def logabsdet(F):
    """``LinearAlgebra.logabsdet(F) -> (log|det F|, sign)`` from the diagonals and row permutations of the stored LU factors
    (``hs_logabsdet``); ``sign`` is ``+-1.0`` for Float64 and a unit complex number for ComplexF64 (``0`` with ``-inf`` for an exactly
    singular pivot).  ``transpose(F)`` has the same determinant, ``adjoint(F)`` the conjugate.  For a compressed factorization this is the
    determinant of ``F``, which approximates that of ``A`` only as well as ``F`` approximates ``A``."""
    F, trans = _unwrap(F)
    la = C.c_double()
    sg = np.zeros(2)
    _lib.check(_lib.lib().hs_logabsdet(F._h, C.byref(la), _pf64(sg)))
    if F.dtype.kind == "c":
        sign = complex(sg[0], -sg[1] if trans == 2 else sg[1])
    else:
        sign = float(sg[0])
    return la.value, sign


def logdet(F):
    """``LinearAlgebra.logdet(F)``: ``log(det(F))``; for Float64 a negative determinant raises ``ValueError`` (Julia's ``DomainError``),
    for ComplexF64 the complex logarithm with the imaginary part in ``(-pi, pi]``."""
    la, sign = logabsdet(F)
    if isinstance(sign, complex):
        return complex(la, np.angle(sign)) if sign != 0 else complex(la, 0.0)
    if sign < 0:
        raise ValueError("DomainError: the determinant is negative; logdet of a real factorization needs det > 0 (use logabsdet)")
    return la


def det(F):
    """``LinearAlgebra.det(F) = sign * exp(log|det F|)`` (over- and underflows like Julia's)."""
    la, sign = logabsdet(F)
    return sign * np.exp(la)


def selinv(F, diag=True, pattern=True, budget=0):
    """Selected inverse of an exact factorization (``hs_selinv``): ``(diag(A^-1), Z)`` with ``Z`` a ``scipy.sparse.csc_matrix`` that has
    ``A``'s ``indptr / indices`` and ``Z[i, j] = (A^-1)[i, j]`` on them -- computed from the stored factors front by front, root to
    leaves, without the dense inverse.  ``diag=False`` / ``pattern=False`` return ``None`` in that place.  ``budget``: bytes of device
    scratch alive at a time (0: what the device has free).  ``transpose(F)`` / ``adjoint(F)`` give the selected inverse of ``A^T`` /
    ``A^H`` on the pattern of ``A`` (``Z[i, j] = (A^-1)[j, i]``, conjugated for the adjoint).  Compressed factorizations are refused
    (``UnsupportedError``; :func:`selinv_lr` serves them)."""
    return _selinv_call(_lib.lib().hs_selinv, "selinv", F, diag, pattern, budget)


def _selinv_call(entry, name, F, diag, pattern, budget):
    """What :func:`selinv` and :func:`selinv_lr` share: the output arrays, the call of ``entry`` and the return value."""
    F, trans = _unwrap(F)
    if not diag and not pattern:
        raise ValueError(f"ArgumentError: {name} with diag=False and pattern=False computes nothing")
    d = np.zeros(F.n, dtype=F.dtype) if diag else None
    z = None
    if pattern:
        if F._pattern is None:
            raise ValueError("ArgumentError: this FactorNode does not know the pattern of its matrix")
        z = np.zeros(len(F._pattern[1]), dtype=F.dtype)
    _lib.check(entry(F._h, 1 if trans else 0, d.ctypes.data if diag else None, z.ctypes.data if pattern else None, 0, int(budget), None))
    if trans == 2 and F.dtype.kind == "c":
        d = d.conj() if diag else None
        z = z.conj() if pattern else None
    Z = sp.csc_matrix((z, F._pattern[1].copy(), F._pattern[0].copy()), shape=(F.n, F.n)) if pattern else None
    return d, Z


def selinv_diag(F, budget=0):
    """``diag(A^-1)`` (marginal variances of a GMRF with precision ``A``, the diagonal of a Green's function) by :func:`selinv`."""
    return selinv(F, diag=True, pattern=False, budget=budget)[0]


def sym_info(F):
    """What ``SolverOptions.symmetric`` did in the last factorization of ``F`` (``hs_sym_info``): ``option`` (in effect), ``fronts_lower`` (dense
    fronts eliminated on their lower triangle) and ``fronts_general`` (fronts eliminated as without the option: dense fronts of a tournament-pivoted
    or redone level or with compressed children, and the compressed, HSS and matrix-free fronts)."""
    out = np.zeros(4, dtype=np.int64)
    _lib.check(_lib.lib().hs_sym_info(F._h, _p64(out)))
    return dict(option=bool(out[0]), fronts_lower=int(out[1]), fronts_general=int(out[2]))


def equil_info(F):
    """What ``SolverOptions.equilibrate`` did in the last factorization of ``F`` (``hs_equil_info``): ``option`` (in effect), ``sweeps`` (Ruiz sweeps
    run, the one that moved no exponent included) and the extreme exponents ``er_min``, ``er_max``, ``ec_min``, ``ec_max`` of
    ``A_s = 2^er A 2^ec``.  With the option off everything is 0."""
    F, _ = _unwrap(F)
    out = np.zeros(6, dtype=np.int64)
    _lib.check(_lib.lib().hs_equil_info(F._h, _p64(out)))
    return dict(option=bool(out[0]), sweeps=int(out[1]), er_min=int(out[2]), er_max=int(out[3]), ec_min=int(out[4]), ec_max=int(out[5]))


def equil_scales(F):
    """``(er, ec)``: the int32 exponents of the row and column scales an equilibrated factorization found, ``A_s = 2^er A 2^ec``
    (``hs_equil_scales``); ``ValueError`` on a handle factored without ``equilibrate``."""
    F, _ = _unwrap(F)
    er = np.zeros(F.n, dtype=np.int32)
    ec = np.zeros(F.n, dtype=np.int32)
    p32 = C.POINTER(C.c_int32)
    _lib.check(_lib.lib().hs_equil_scales(F._h, er.ctypes.data_as(p32), ec.ctypes.data_as(p32)))
    return er, ec


def selinv_info(F):
    """Figures of the last :func:`selinv` call on ``F`` (``hs_selinv_info``): device seconds, real flops executed, peak scratch bytes,
    batches of fronts."""
    F, _ = _unwrap(F)
    out = np.zeros(4)
    _lib.check(_lib.lib().hs_selinv_info(F._h, _pf64(out)))
    return dict(seconds=float(out[0]), flops=float(out[1]), peak_bytes=float(out[2]), batches=int(out[3]))


def selinv_lr(F, diag=True, pattern=True, budget=0):
    """Selected inverse of a compressed factorization (``hs_selinv_lr``), with the arguments and the return value of :func:`selinv`:
    ``diag(F^-1)`` and ``F^-1`` on the pattern of ``A``, ``F`` being the operator the solves apply.  The recurrence runs through the
    low-rank Gauss transforms of the compressed fronts (substitutions on ``rank`` columns instead of ``|bnd|``), dense fronts run
    :func:`selinv`'s; on an exact factorization it returns :func:`selinv`'s bits.  ``transpose(F)`` gives ``F^-T`` on the pattern: the
    gradient of :func:`logabsdet` with respect to the entries of ``A``.  Refused (``UnsupportedError``): HSS interior blocks
    (``mf = 2, 3``, ``hss_d``), sliced fronts, several ranks."""
    return _selinv_call(_lib.lib().hs_selinv_lr, "selinv_lr", F, diag, pattern, budget)


def selinv_lr_diag(F, budget=0):
    """``diag(F^-1)`` of a compressed factorization by :func:`selinv_lr`."""
    return selinv_lr(F, diag=True, pattern=False, budget=budget)[0]


def selinv_lr_info(F):
    """Figures of the last :func:`selinv_lr` call on ``F`` (``hs_selinv_lr_info``): device seconds, real flops executed, peak scratch
    bytes, batches of fronts, fronts served through low-rank transforms, the largest rank used, and the flops :func:`selinv`'s dense-form
    recurrence would execute on the same front shapes (a host count).  :func:`selinv_info` keeps its own figures."""
    F, _ = _unwrap(F)
    out = np.zeros(8)
    _lib.check(_lib.lib().hs_selinv_lr_info(F._h, _pf64(out)))
    return dict(seconds=float(out[0]), flops=float(out[1]), peak_bytes=float(out[2]), batches=int(out[3]), lowrank_fronts=int(out[4]),
                max_rank=int(out[5]), flops_dense_form=float(out[6]))


# ---- Schur-complement mode (hs_interface.hip): the interface matrix, condense and expand solves --------------------------------------
def interface_indices(F):
    """The interface of ``F``: the 0-based ids of the boundary the root of its tree keeps (``root.bnd``, e.g. from
    ``problems.graph_nested_dissection(A, nmax, interface=...)``), in the order of the rows and columns of :func:`schur_complement`.
    Empty for an ordinary tree."""
    F, _ = _unwrap(F)
    nb = _lib.i64()
    _lib.check(_lib.lib().hs_interface_size(F._h, C.byref(nb)))
    idx = np.zeros(nb.value, dtype=np.int64)
    if nb.value:
        _lib.check(_lib.lib().hs_interface_indices(F._h, _p64(idx)))
    return idx - 1


def schur_complement(F, device=False):
    """The dense Schur complement ``S = A_bb - A_bi A_ii^-1 A_ib`` of ``F`` on its interface ``b`` (:func:`interface_indices`), rebuilt on
    the device from the pivoted LU the factorization keeps of it (``hs_interface_matrix_*``): no second factorization, the factors are only
    read, two calls return the same bits.  ``transpose(F)`` / ``adjoint(F)`` give ``S^T`` / ``S^H``.  ``device=True`` returns a device
    tensor (column-major) instead of a NumPy array.  For a compressed factorization this is the Schur complement of the compressed
    factorization."""
    F, trans = _unwrap(F)
    nb = len(interface_indices(F))
    fn = getattr(_lib.lib(), "hs_interface_matrix" + ("_z" if F.dtype.kind == "c" else "_d"))
    if device:
        import torch

        St = torch.zeros((nb, nb), dtype=torch.complex128 if F.dtype.kind == "c" else torch.float64, device="cuda")  # its transpose is column-major
        _lib.check(fn(F._h, St.data_ptr() if nb else None, max(nb, 1), 1, None))
        S = St.t()
        return S if trans == 0 else (S.t() if trans == 1 else S.t().conj())
    S = np.zeros((nb, nb), dtype=F.dtype, order="F")
    _lib.check(fn(F._h, S.ctypes.data if nb else None, max(nb, 1), 0, None))
    return S if trans == 0 else (S.T if trans == 1 else S.conj().T)


def _interface_phase(name, F, Cb):
    """One of the three phases in place on the ``n x nrhs`` block ``Cb``: a column-major NumPy array or device tensor of ``F``'s dtype."""
    F, trans = _unwrap(F)
    sfx = "_z" if F.dtype.kind == "c" else "_d"
    if hasattr(Cb, "data_ptr"):  # a device tensor
        import torch

        want = torch.complex128 if F.dtype.kind == "c" else torch.float64
        if not Cb.is_cuda or Cb.dtype != want:
            raise TypeError(f"{name}: the block must be a {F.dtype} array or a device tensor of that type (it is updated in place)")
        if Cb.dim() not in (1, 2) or Cb.shape[0] != F.n:
            raise _lib.DimensionMismatch(f"DimensionMismatch: the block has {tuple(Cb.shape)[:1]} rows, F is {F.n} x {F.n}")
        nrhs = 1 if Cb.dim() == 1 else Cb.shape[1]
        ld = F.n if (Cb.dim() == 1 or nrhs == 1) else Cb.stride(1)
        if Cb.stride(0) != 1 or ld < F.n:
            raise ValueError(f"{name}: the device block must be column-major (stride 1 down a column): it is updated in place")
        fn = getattr(_lib.lib(), "hs_interface_" + name + "_dev" + sfx)
        _lib.check(fn(F._h, trans, Cb.data_ptr(), ld, F.n, nrhs, torch.cuda.current_stream().cuda_stream))
        return Cb
    if not isinstance(Cb, np.ndarray) or Cb.dtype != F.dtype:
        raise TypeError(f"{name}: the block must be a {F.dtype} array or a device tensor of that type (it is updated in place)")
    if Cb.ndim not in (1, 2) or Cb.shape[0] != F.n:
        raise _lib.DimensionMismatch(f"DimensionMismatch: the block has {Cb.shape[:1]} rows, F is {F.n} x {F.n}")
    if not (Cb.flags.f_contiguous and Cb.flags.writeable):
        raise ValueError(f"{name}: the block must be a writeable column-major array (np.asfortranarray): it is updated in place")
    nrhs = 1 if Cb.ndim == 1 else Cb.shape[1]
    fn = getattr(_lib.lib(), "hs_interface_" + name + sfx)
    _lib.check(fn(F._h, trans, Cb.ctypes.data_as(_lib.p_f64), F.n, F.n, nrhs))
    return Cb


def condense(F, B):
    """First phase of a solve split at the interface (``hs_interface_condense_*``), in place on the column-major block ``B`` (NumPy or
    device tensor), which is returned: afterwards ``B[idx] = g = B_b - op(A)_bi op(A)_ii^-1 B_i`` with ``idx = interface_indices(F)``;
    the other rows hold the forward intermediates :func:`expand` needs (opaque).  ``F`` may be ``transpose(F)`` / ``adjoint(F)``."""
    return _interface_phase("condense", F, B)


def interface_solve(F, Cb):
    """Second phase (``hs_interface_solve_*``), in place: ``C[idx] = op(S)^-1 C[idx]`` with the factors the handle keeps of ``S``; the other
    rows are left alone.  A caller with its own interface system (``(S + K) y = g + h``) overwrites ``C[idx]`` itself instead."""
    return _interface_phase("solve", F, Cb)


def expand(F, Cb):
    """Third phase (``hs_interface_expand_*``), in place on a block :func:`condense` has filled: reads ``C[idx]`` as the interface values
    ``y`` and leaves ``op(A)_ii^-1 (B_i - op(A)_ib y)`` in the other rows; ``C[idx]`` is not changed.
    ``expand(F, interface_solve(F, condense(F, B)))`` returns the bits of ``ldiv_block_t(F, B)``."""
    return _interface_phase("expand", F, Cb)


def interface_info(F):
    """Figures of the last interface calls on ``F`` (``hs_interface_info``): device seconds and executed real flops of the last
    :func:`schur_complement`, the interface size, the device seconds of the last condense / solve / expand, the column chunks of the last
    phase call."""
    F, _ = _unwrap(F)
    out = np.zeros(8)
    _lib.check(_lib.lib().hs_interface_info(F._h, _pf64(out)))
    return dict(matrix_seconds=float(out[0]), matrix_flops=float(out[1]), nb=int(out[2]), condense_seconds=float(out[3]), solve_seconds=float(out[4]),
                expand_seconds=float(out[5]), chunks=int(out[6]))
