"""ctypes binding of ``libhs_solver.so`` (C ABI: ``include/hs_solver.h``, ``include/hs_kernels.h``).

There is no CPU fallback: if the shared library is missing, or it finds no HIP
device, the calls raise.  ``build()`` compiles the library in-tree with hipcc
(cross-compiles for gfx950 without a GPU).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhs_solver.so")
CSRC = os.path.join(_HERE, "csrc")

i64 = C.c_int64
p_i64 = C.POINTER(C.c_int64)
p_f64 = C.POINTER(C.c_double)


class hs_options(C.Structure):
    _fields_ = [
        ("swlevel", i64), ("swsize", i64), ("atol", C.c_double), ("rtol", C.c_double), ("c_tol", C.c_double),
        ("leafsize", i64), ("kest", i64), ("stepsize", i64), ("verbose", C.c_uint8),
        ("keep_schur", C.c_uint8), ("profile", C.c_uint8), ("split", C.c_uint8), ("hss_d", C.c_uint8), ("hss_dexp", C.c_uint8), ("mf", C.c_uint8), ("dist_top", C.c_uint8), ("seed", i64), ("symmetric", C.c_uint8), ("equilibrate", C.c_uint8),
    ]


class hs_tree(C.Structure):
    _fields_ = [
        ("nnodes", i64), ("left", p_i64), ("right", p_i64),
        ("int_ptr", p_i64), ("int_idx", p_i64), ("bnd_ptr", p_i64), ("bnd_idx", p_i64),
        ("iloc_ptr", p_i64), ("iloc_idx", p_i64), ("bloc_ptr", p_i64), ("bloc_idx", p_i64),
    ]


class hs_stats(C.Structure):
    _fields_ = [
        ("n", i64), ("nnodes", i64), ("nlevels", i64), ("max_ni", i64), ("max_nb", i64),
        ("flops_factor", C.c_double), ("bytes_factors", C.c_double), ("bytes_solve", C.c_double),
        ("t_symbolic", C.c_double), ("t_upload", C.c_double), ("t_assemble", C.c_double), ("t_panel", C.c_double),
        ("t_trsm", C.c_double), ("t_gemm", C.c_double), ("t_total", C.c_double), ("t_solve", C.c_double),
        ("gemm_flops", C.c_double), ("gemm_launches", i64),
        ("t_mfma_kernel", C.c_double), ("mfma_kernel_launches", i64), ("gemm_bytes", C.c_double),
    ]


class hs_sparse_dev(C.Structure):
    _fields_ = [("n", i64), ("colptr", C.c_void_p), ("rowval", C.c_void_p), ("nzval", C.c_void_p),
                ("rowptr", C.c_void_p), ("colind", C.c_void_p), ("nzval_r", C.c_void_p)]


class hs_block_arg(C.Structure):
    """An n x nrhs block of ``hs_sens_*`` / ``hs_misfit_*`` / ``hs_tangent_*`` / ``hs_gn_*``: dense (``dense``, ``ld``) or, with ``dense`` NULL, 1-based CSC."""
    _fields_ = [("dense", C.c_void_p), ("ld", i64), ("colptr", p_i64), ("rowval", p_i64), ("nzval", C.c_void_p)]


class hs_hss_blockop(C.Structure):
    _fields_ = [("n1", i64), ("n2", i64), ("H1", C.c_void_p), ("H2", C.c_void_p), ("gid", p_i64), ("A", C.POINTER(hs_sparse_dev)), ("lpos", C.c_void_p)]


class hs_hss_options(C.Structure):
    _fields_ = [("leafsize", i64), ("first_split", i64), ("atol", C.c_double), ("rtol", C.c_double), ("kest", i64), ("pad", i64), ("seed", i64),
                ("level_scale", C.c_double)]


# hs_transfer_fn (include/hs_solver.h): one host message per peer and direction
HS_TRANSFER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, i64, p_i64, C.POINTER(C.c_void_p), p_i64, i64, p_i64, C.POINTER(C.c_void_p), p_i64)

HS_OK = 0
HS_ERR_ARGUMENT, HS_ERR_DIMENSION, HS_ERR_TREE, HS_ERR_SINGULAR = -1, -2, -3, -4
HS_ERR_HSS_LEAF, HS_ERR_DEVICE, HS_ERR_NOMEM, HS_ERR_UNSUPPORTED = -5, -6, -7, -8
HS_BLK_LU, HS_BLK_LBI, HS_BLK_UIB, HS_BLK_S, HS_BLK_DLU = 0, 1, 2, 3, 4

# every symbol include/*.h declares (tests check the library exports all of them)
EXPORTS = [
    "hs_options_default", "hs_factor_d", "hs_factor_z", "hs_ldiv_d", "hs_ldiv_z", "hs_ldiv_dev_d", "hs_ldiv_dev_z",
    "hs_ldiv_t_d", "hs_ldiv_t_z", "hs_ldiv_dev_t_d", "hs_ldiv_dev_t_z",
    "hs_ldiv_block_d", "hs_ldiv_block_z", "hs_ldiv_block_dev_d", "hs_ldiv_block_dev_z", "hs_ldiv_block_info", "hsk_multi_prob_d", "hsk_multi_prob_z",
    "hs_ldiv_block_t_d", "hs_ldiv_block_t_z", "hs_ldiv_block_dev_t_d", "hs_ldiv_block_dev_t_z", "hsk_multi_prob_t_d", "hsk_multi_prob_t_z",
    "hs_ldiv_ulv_d", "hs_ldiv_ulv_z", "hs_ldiv_ulv_dev_d", "hs_ldiv_ulv_dev_z", "hs_ulv_mode", "hs_hss_logabsdet", "hsk_ulv_det_d", "hsk_ulv_det_z",
    "hs_mul_d", "hs_mul_z", "hs_mul_dev_d", "hs_mul_dev_z", "hs_mul_info", "hs_factor_error_d", "hs_factor_error_z",
    "hsk_multi_tri_d", "hsk_multi_tri_z", "hsk_multi_tri_t_d", "hsk_multi_tri_t_z",
    "hs_ldiv_sparse_d", "hs_ldiv_sparse_z", "hs_ldiv_sparse_dev_d", "hs_ldiv_sparse_dev_z", "hs_ldiv_sparse_plan", "hs_ldiv_sparse_info",
    "hs_opnorm", "hs_normestinv", "hs_condest", "hs_ldiv_refine_d", "hs_ldiv_refine_z", "hs_ldiv_refine_dev_d", "hs_ldiv_refine_dev_z",
    "hs_ldiv_refine_block_d", "hs_ldiv_refine_block_z", "hs_ldiv_refine_block_dev_d", "hs_ldiv_refine_block_dev_z", "hs_ldiv_refine_block_info",
    "hs_logabsdet", "hs_selinv", "hs_selinv_info", "hs_selinv_lr", "hs_selinv_lr_info", "hs_sym_info", "hs_equil_info", "hs_equil_scales",
    "hs_interface_size", "hs_interface_indices", "hs_interface_matrix_d", "hs_interface_matrix_z", "hs_interface_info", "hsk_lu_product_d", "hsk_lu_product_z",
    "hs_interface_condense_d", "hs_interface_condense_z", "hs_interface_condense_dev_d", "hs_interface_condense_dev_z",
    "hs_interface_solve_d", "hs_interface_solve_z", "hs_interface_solve_dev_d", "hs_interface_solve_dev_z",
    "hs_interface_expand_d", "hs_interface_expand_z", "hs_interface_expand_dev_d", "hs_interface_expand_dev_z",
    "hs_sens_d", "hs_sens_z", "hs_sens_dev_d", "hs_sens_dev_z", "hs_misfit_d", "hs_misfit_z", "hs_misfit_dev_d", "hs_misfit_dev_z", "hs_sens_info", "hsk_sddmm_d", "hsk_sddmm_z",
    "hs_tangent_d", "hs_tangent_z", "hs_tangent_dev_d", "hs_tangent_dev_z", "hs_gn_hessvec_d", "hs_gn_hessvec_z", "hs_gn_hessvec_dev_d", "hs_gn_hessvec_dev_z",
    "hs_gn_diag_d", "hs_gn_diag_z", "hs_gn_diag_dev_d", "hs_gn_diag_dev_z", "hs_gn_info", "hsk_gn_rhs_d", "hsk_gn_rhs_z", "hsk_gn_rowsq_d", "hsk_gn_rowsq_z",
    "hs_mod_create_d", "hs_mod_create_z", "hs_mod_create_dev_d", "hs_mod_create_dev_z", "hs_mod_create_sparse_d", "hs_mod_create_sparse_z", "hs_mod_ldiv_d", "hs_mod_ldiv_z",
    "hs_mod_ldiv_dev_d", "hs_mod_ldiv_dev_z", "hs_mod_info", "hs_mod_free", "hs_gmres_block_mod_d", "hs_gmres_block_mod_z",
    "hs_eigs_d", "hs_eigs_z", "hs_eigs_info", "hs_eigs_gen_d", "hs_eigs_gen_z", "hs_eigs_gen_info", "hsk_eigs_coldot_d", "hsk_eigs_coldot_z", "hsk_eigs_rotate_d", "hsk_eigs_rotate_z", "hsk_eigs_chol_inv_d", "hsk_eigs_chol_inv_z", "hsk_small_eig_z", "hsk_eigs_phase_timing", "hsk_eigs_phases", "hsk_eigs_gen_mprod_seconds",
    "hs_f32_create", "hs_f32_ldiv_d", "hs_f32_ldiv_z", "hs_f32_ldiv_dev_d", "hs_f32_ldiv_dev_z", "hs_f32_info", "hs_f32_free", "hs_gmres_block_f32_d", "hs_gmres_block_f32_z",
    "hsk_multi_prob_f32_d", "hsk_multi_prob_f32_z", "hsk_multi_prob_t_f32_d", "hsk_multi_prob_t_f32_z", "hsk_round_factors_f32",
    "hsk_mod_inner_d", "hsk_mod_inner_z", "hsk_mod_apply_d", "hsk_mod_apply_z", "hsk_mod_gather_d", "hsk_mod_gather_z", "hsk_mod_cap_d", "hsk_mod_cap_z",
    "hs_maxrank", "hs_is_complex", "hs_size", "hs_free", "hs_last_error", "hs_last_error_info", "hs_get_stats",
    "hs_node_info", "hs_node_ranks", "hs_node_export", "hs_node_export_piv", "hs_device_info",
    "hs_analyze", "hs_plan", "hs_numeric_begin", "hs_numeric_levels", "hs_numeric_end", "hs_solve_fwd_levels", "hs_solve_bwd_levels",
    "hs_nlevels", "hs_cut_level", "hs_node_owner", "hs_num_exchanges", "hs_exchange_info", "hs_set_schur_buffer",
    "hs_pack_bnd", "hs_unpack_bnd", "hs_extract_owned", "hs_gmres_d", "hs_gmres_z", "hs_gmres_block_d", "hs_gmres_block_z", "hs_gmres_block_info", "hsk_spmm_d", "hsk_spmm_z",
    "hs_gmres_t_d", "hs_gmres_t_z", "hs_gmres_block_t_d", "hs_gmres_block_t_z", "hsk_spmm_op_d", "hsk_spmm_op_z",
    "hs_exchange_kind", "hs_schur_pack_size", "hs_schur_pack", "hs_schur_unpack", "hs_flow_info", "hs_hss_pack_size", "hs_hss_pack", "hs_hss_unpack", "hs_hss_qr_order",
    "hs_comm_unique_id", "hs_comm_create_rccl", "hs_comm_create_host", "hs_comm_free", "hs_comm_kind", "hs_comm_selftest", "hs_comm_bandwidth", "hs_set_comm",
    "hs_symbolic_from_elimtree", "hs_symbolic_from_graph", "hs_symbolic_size", "hs_symbolic_perm", "hs_symbolic_tree", "hs_symbolic_free",
    "hs_hss_options_default", "hs_hss_compress_d", "hs_hss_compress_z", "hs_hss_compress_ex_d", "hs_hss_compress_ex_z", "hs_hss_compress_lru_d", "hs_hss_compress_lru_z", "hs_hss_compress_lru_multi_d", "hs_hss_compress_lru_multi_z", "hs_hss_set_stream", "hs_hss_rank", "hs_hss_size", "hs_hss_samples", "hs_hss_num_nodes",
    "hs_hss_node_info", "hs_hss_node_data", "hs_hss_getindex", "hs_hss_basis", "hs_hss_expand", "hs_hss_mul", "hs_hss_mul_t", "hs_hss_child", "hs_hss_factor", "hs_hss_ldiv", "hs_hss_ldiv_t", "hsk_ulv_t_group_d", "hsk_ulv_t_group_z", "hs_hss_time", "hs_hss_trim", "hs_hss_free", "hs_node_schur_hss",
    "hs_hss_offdiag", "hs_hss_bytes", "hs_hss_prune_leaves", "hs_hss_compatible", "hs_hss_depth", "hs_hss_compress_blockop_d", "hs_hss_compress_blockop_z", "hs_hss_blockop_apply",
    "hsk_gemm_d", "hsk_gemm_z", "hsk_lowrank_d", "hsk_lowrank_z", "hsk_front_factor_d", "hsk_front_factor_z", "hsk_front_batch_d", "hsk_front_batch_z", "hsk_sweep_level_d", "hsk_sweep_level_z", "hsk_flow_tall_rule", "hsk_sweep_path", "hsk_mfma_f64_peak", "hsk_mfma_f64_peak_random", "hsk_flow_pingpong_us", "hsk_bisect_perm",
    "hs_probs_stats_mode", "hs_probs_stats", "hs_trim", "hs_stream_order",
    "hsk_leaf_envelope", "hsk_envelope_enable", "hsk_branch_envelope", "hsk_branch_envelope_enable", "hsk_front_batch_env_d", "hsk_op_flops_mode", "hsk_op_flops",
    "hsk_env_order_enable", "hsk_env_tile_order", "hsk_env_phase_order", "hsk_env_perm", "hsk_env_perm_slot_limit", "hsk_env_perm_min_tiles", "hsk_env_perm_launches",
    "hsk_gemm_op_d", "hsk_gemm_lds_enable", "hsk_gemm_lds_launches",
    "hsk_gemm_lds_edge_launches", "hsk_gemm_reg_launches", "hsk_gemm_lds_route", "hsk_gemm_schur_d",
    "hsk_trsm_inv_d", "hsk_trsm_strip_enable", "hsk_trsm_strip_launches", "hsk_trsm_half_launches", "hsk_lookahead_runs", "hsk_front_batch_sym_d", "hsk_front_batch_sym_z",
    "hsk_qr_params", "hsk_qr_chol_d", "hsk_qr_chol_z", "hsk_qr_select", "hsk_qr_refine_d", "hsk_qr_refine_z",
]

_lib = None


def build(force=False, verbose=False):
    """Compile ``libhs_solver.so`` for gfx950 in-tree (``make`` in ``csrc/``)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, capture_output=not verbose)
    r = subprocess.run(["make", "-C", CSRC, "-j4"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libhs_solver.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


def lib():
    """Load the shared library (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built (run __graft_entry__.build() or `make -C {CSRC}`); "
            "there is no CPU fallback"
        )
    # PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64 (same SONAMEs as /opt/rocm's).  Two HSA
    # runtimes cannot share a process, so when torch is installed let it load its runtime FIRST; this
    # library then binds to the already-loaded one.  (A Julia host has no torch and uses /opt/rocm's.)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.hs_options_default.argtypes = [C.POINTER(hs_options)]
    L.hs_options_default.restype = None
    for f in (L.hs_factor_d, L.hs_factor_z):
        f.argtypes = [i64, p_i64, p_i64, p_f64, C.POINTER(hs_tree), C.POINTER(hs_options), C.POINTER(vp)]
        f.restype = C.c_int
    for f in (L.hs_ldiv_d, L.hs_ldiv_z):
        f.argtypes = [vp, p_f64, i64, p_f64, i64, i64, i64]
        f.restype = C.c_int
    for f in (L.hs_ldiv_dev_d, L.hs_ldiv_dev_z):
        f.argtypes = [vp, vp, i64, vp, i64, i64, i64, vp]
        f.restype = C.c_int
    # (F, trans, C, ldc, B, ldb, n, nrhs) on the host, the same on the device with a stream
    for host, dev in (("hs_ldiv_t", "hs_ldiv_dev_t"), ("hs_ldiv_block", "hs_ldiv_block_dev"), ("hs_ldiv_block_t", "hs_ldiv_block_dev_t"), ("hs_ldiv_ulv", "hs_ldiv_ulv_dev"),
                      ("hs_mul", "hs_mul_dev")):
        for sfx in ("_d", "_z"):
            f = getattr(L, host + sfx)
            f.argtypes = [vp, C.c_int, p_f64, i64, p_f64, i64, i64, i64]
            f.restype = C.c_int
            f = getattr(L, dev + sfx)
            f.argtypes = [vp, C.c_int, vp, i64, vp, i64, i64, i64, vp]
            f.restype = C.c_int
    L.hs_ldiv_block_info.argtypes = [vp, p_f64]
    L.hs_ldiv_block_info.restype = C.c_int
    L.hs_mul_info.argtypes = [vp, p_f64]
    L.hs_mul_info.restype = C.c_int
    for f in (L.hs_factor_error_d, L.hs_factor_error_z):  # Omega: a host or a device address (where)
        f.argtypes = [vp, C.c_int, vp, i64, i64, i64, C.c_int, p_f64]
        f.restype = C.c_int
    for f in (L.hsk_multi_tri_d, L.hsk_multi_tri_z):
        f.argtypes = [i64, i64, i64, p_f64, i64, p_f64, i64, p_f64, i64, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        f.restype = C.c_int
    for f in (L.hsk_multi_tri_t_d, L.hsk_multi_tri_t_z):
        f.argtypes = [i64, i64, i64, p_f64, i64, p_f64, i64, p_f64, i64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        f.restype = C.c_int
    for f in (L.hs_ldiv_sparse_d, L.hs_ldiv_sparse_z):
        f.argtypes = [vp, C.c_int, i64, i64, p_i64, p_i64, p_f64, p_i64, i64, p_f64, i64]
        f.restype = C.c_int
    for f in (L.hs_ldiv_sparse_dev_d, L.hs_ldiv_sparse_dev_z):
        f.argtypes = [vp, C.c_int, i64, i64, p_i64, p_i64, vp, p_i64, i64, vp, i64, vp]
        f.restype = C.c_int
    L.hs_ldiv_sparse_plan.argtypes = [vp, C.c_int, i64, i64, p_i64, p_i64, p_i64, i64, p_i64, p_i64, C.POINTER(C.c_uint8)]
    L.hs_ldiv_sparse_plan.restype = C.c_int
    L.hs_ldiv_sparse_info.argtypes = [vp, p_f64]
    L.hs_ldiv_sparse_info.restype = C.c_int
    for f in (L.hsk_multi_prob_d, L.hsk_multi_prob_z):
        f.argtypes = [i64, i64, i64, p_f64, i64, p_f64, i64, p_f64, i64, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        f.restype = C.c_int
    for f in (L.hsk_multi_prob_t_d, L.hsk_multi_prob_t_z):
        f.argtypes = [i64, i64, i64, p_f64, i64, p_f64, i64, p_f64, i64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        f.restype = C.c_int
    L.hs_opnorm.argtypes = [vp, C.c_int, p_f64]
    L.hs_opnorm.restype = C.c_int
    L.hs_normestinv.argtypes = [vp, C.c_int, i64, i64, p_f64, p_i64, vp]
    L.hs_normestinv.restype = C.c_int
    L.hs_condest.argtypes = [vp, C.c_int, i64, p_f64, p_f64, p_f64, vp]
    L.hs_condest.restype = C.c_int
    for f in (L.hs_ldiv_refine_d, L.hs_ldiv_refine_z):
        f.argtypes = [vp, C.c_int, p_f64, i64, p_f64, i64, i64, i64, i64, p_f64, p_f64, p_i64]
        f.restype = C.c_int
    for f in (L.hs_ldiv_refine_dev_d, L.hs_ldiv_refine_dev_z):
        f.argtypes = [vp, C.c_int, vp, i64, vp, i64, i64, i64, i64, p_f64, p_f64, p_i64, vp]
        f.restype = C.c_int
    for f in (L.hs_ldiv_refine_block_d, L.hs_ldiv_refine_block_z):
        f.argtypes = [vp, C.c_int, p_f64, i64, p_f64, i64, i64, i64, i64, p_f64, p_f64, p_i64]
        f.restype = C.c_int
    for f in (L.hs_ldiv_refine_block_dev_d, L.hs_ldiv_refine_block_dev_z):
        f.argtypes = [vp, C.c_int, vp, i64, vp, i64, i64, i64, i64, p_f64, p_f64, p_i64, vp]
        f.restype = C.c_int
    L.hs_ldiv_refine_block_info.argtypes = [p_f64]
    L.hs_ldiv_refine_block_info.restype = C.c_int
    pb = C.POINTER(hs_block_arg)
    for f in (L.hs_sens_d, L.hs_sens_z):
        f.argtypes = [vp, C.c_int, i64, i64, pb, pb, i64, C.c_int, vp, vp, i64, vp, i64]
        f.restype = C.c_int
    for f in (L.hs_sens_dev_d, L.hs_sens_dev_z):
        f.argtypes = [vp, C.c_int, i64, i64, pb, pb, i64, C.c_int, vp, vp, i64, vp, i64, vp]
        f.restype = C.c_int
    for f in (L.hs_misfit_d, L.hs_misfit_z):
        f.argtypes = [vp, C.c_int, i64, i64, pb, p_i64, i64, vp, i64, i64, C.c_int, vp, vp, i64, vp]
        f.restype = C.c_int
    for f in (L.hs_misfit_dev_d, L.hs_misfit_dev_z):
        f.argtypes = [vp, C.c_int, i64, i64, pb, p_i64, i64, vp, i64, i64, C.c_int, vp, vp, i64, vp, vp]
        f.restype = C.c_int
    L.hs_sens_info.argtypes = [vp, p_f64]
    L.hs_sens_info.restype = C.c_int
    for f in (L.hsk_sddmm_d, L.hsk_sddmm_z):
        f.argtypes = [i64, p_i64, p_i64, i64, vp, i64, vp, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, p_f64]
        f.restype = C.c_int
    # (F, trans, n, nrhs, B, Xin, ldxin, E, pattern, itmax, rows, nrows, dX, lddx, X, ldx)
    for f in (L.hs_tangent_d, L.hs_tangent_z):
        f.argtypes = [vp, C.c_int, i64, i64, pb, vp, i64, vp, C.c_int, i64, p_i64, i64, vp, i64, vp, i64]
        f.restype = C.c_int
    for f in (L.hs_tangent_dev_d, L.hs_tangent_dev_z):
        f.argtypes = [vp, C.c_int, i64, i64, pb, vp, i64, vp, C.c_int, i64, p_i64, i64, vp, i64, vp, i64, vp]
        f.restype = C.c_int
    # (..., rows, nrows, HE, JE, ldje, X, ldx)
    for f in (L.hs_gn_hessvec_d, L.hs_gn_hessvec_z):
        f.argtypes = [vp, C.c_int, i64, i64, pb, vp, i64, vp, C.c_int, i64, p_i64, i64, vp, vp, i64, vp, i64]
        f.restype = C.c_int
    for f in (L.hs_gn_hessvec_dev_d, L.hs_gn_hessvec_dev_z):
        f.argtypes = [vp, C.c_int, i64, i64, pb, vp, i64, vp, C.c_int, i64, p_i64, i64, vp, vp, i64, vp, i64, vp]
        f.restype = C.c_int
    # (F, trans, n, nrhs, B, Xin, ldxin, rows, nrows, pattern, itmax, Hd, z2, x2)
    for f in (L.hs_gn_diag_d, L.hs_gn_diag_z):
        f.argtypes = [vp, C.c_int, i64, i64, pb, vp, i64, p_i64, i64, C.c_int, i64, vp, vp, vp]
        f.restype = C.c_int
    for f in (L.hs_gn_diag_dev_d, L.hs_gn_diag_dev_z):
        f.argtypes = [vp, C.c_int, i64, i64, pb, vp, i64, p_i64, i64, C.c_int, i64, vp, vp, vp, vp]
        f.restype = C.c_int
    L.hs_gn_info.argtypes = [vp, p_f64]
    L.hs_gn_info.restype = C.c_int
    for f in (L.hsk_gn_rhs_d, L.hsk_gn_rhs_z):
        f.argtypes = [C.c_int, i64, p_i64, p_i64, vp, C.c_int, vp, i64, i64, vp, i64]
        f.restype = C.c_int
    for f in (L.hsk_gn_rowsq_d, L.hsk_gn_rowsq_z):
        f.argtypes = [i64, i64, vp, i64, vp]
        f.restype = C.c_int
    for f in (L.hs_mod_create_d, L.hs_mod_create_z):
        f.argtypes = [vp, i64, i64, vp, i64, vp, i64, C.POINTER(vp)]
        f.restype = C.c_int
    for f in (L.hs_mod_create_dev_d, L.hs_mod_create_dev_z):
        f.argtypes = [vp, i64, i64, vp, i64, vp, i64, vp, C.POINTER(vp)]
        f.restype = C.c_int
    for f in (L.hs_mod_create_sparse_d, L.hs_mod_create_sparse_z):
        f.argtypes = [vp, i64, p_i64, p_i64, vp, C.POINTER(vp)]
        f.restype = C.c_int
    for f in (L.hs_mod_ldiv_d, L.hs_mod_ldiv_z):
        f.argtypes = [vp, C.c_int, p_f64, i64, p_f64, i64, i64, i64]
        f.restype = C.c_int
    for f in (L.hs_mod_ldiv_dev_d, L.hs_mod_ldiv_dev_z):
        f.argtypes = [vp, C.c_int, vp, i64, vp, i64, i64, i64, vp]
        f.restype = C.c_int
    L.hs_mod_info.argtypes = [vp, p_f64]
    L.hs_mod_info.restype = C.c_int
    L.hs_mod_free.argtypes = [vp]
    L.hs_mod_free.restype = None
    for f in (L.hs_gmres_block_mod_d, L.hs_gmres_block_mod_z):
        f.argtypes = [vp, C.c_int, i64, p_i64, p_i64, vp, vp, i64, vp, i64, i64, C.c_int, C.c_int, C.c_double, C.c_double, i64, i64, p_f64, p_i64, C.POINTER(C.c_int), vp]
        f.restype = C.c_int
    L.hs_f32_create.argtypes = [vp, vp, C.POINTER(vp)]
    L.hs_f32_create.restype = C.c_int
    for f in (L.hs_f32_ldiv_d, L.hs_f32_ldiv_z):
        f.argtypes = [vp, C.c_int, p_f64, i64, p_f64, i64, i64, i64]
        f.restype = C.c_int
    for f in (L.hs_f32_ldiv_dev_d, L.hs_f32_ldiv_dev_z):
        f.argtypes = [vp, C.c_int, vp, i64, vp, i64, i64, i64, vp]
        f.restype = C.c_int
    L.hs_f32_info.argtypes = [vp, p_f64]
    L.hs_f32_info.restype = C.c_int
    L.hs_f32_free.argtypes = [vp]
    L.hs_f32_free.restype = None
    for f in (L.hs_gmres_block_f32_d, L.hs_gmres_block_f32_z):
        f.argtypes = [vp, C.c_int, i64, p_i64, p_i64, vp, vp, i64, vp, i64, i64, C.c_int, C.c_int, C.c_double, C.c_double, i64, i64, p_f64, p_i64, C.POINTER(C.c_int), vp]
        f.restype = C.c_int
    for f in (L.hsk_multi_prob_f32_d, L.hsk_multi_prob_f32_z):
        f.argtypes = [i64, i64, i64, p_f64, i64, p_f64, i64, p_f64, i64, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        f.restype = C.c_int
    for f in (L.hsk_multi_prob_t_f32_d, L.hsk_multi_prob_t_f32_z):
        f.argtypes = [i64, i64, i64, p_f64, i64, p_f64, i64, p_f64, i64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        f.restype = C.c_int
    L.hsk_round_factors_f32.argtypes = [vp, p_i64]
    L.hsk_round_factors_f32.restype = C.c_int
    for f in (L.hsk_mod_inner_d, L.hsk_mod_inner_z):
        f.argtypes = [i64, i64, i64, vp, i64, vp, i64, C.c_int, vp, i64]
        f.restype = C.c_int
    for f in (L.hsk_mod_apply_d, L.hsk_mod_apply_z):
        f.argtypes = [i64, i64, i64, vp, i64, vp, i64, vp, i64, C.c_int]
        f.restype = C.c_int
    for f in (L.hsk_mod_gather_d, L.hsk_mod_gather_z):
        f.argtypes = [i64, i64, i64, vp, i64, p_i64, vp, i64]
        f.restype = C.c_int
    for f in (L.hsk_mod_cap_d, L.hsk_mod_cap_z):
        f.argtypes = [i64, i64, vp, i64, C.c_int, vp, i64]
        f.restype = C.c_int
    for f in (L.hs_eigs_d, L.hs_eigs_z):
        f.argtypes = [vp, C.c_int, i64, i64, i64, i64, C.c_double, C.c_double, C.c_double, i64, vp, i64, i64, C.c_int, p_f64, vp, i64, p_f64, p_f64, p_i64, p_i64, vp]
        f.restype = C.c_int
    L.hs_eigs_info.argtypes = [p_f64]
    L.hs_eigs_info.restype = C.c_int
    for f in (L.hs_eigs_gen_d, L.hs_eigs_gen_z):
        f.argtypes = [vp, C.c_int, i64, p_i64, p_i64, vp, C.c_int, i64, i64, i64, C.c_double, C.c_double, C.c_double, i64, vp, i64, i64, C.c_int, p_f64, vp, i64, p_f64, p_f64,
                      p_i64, p_i64, vp]
        f.restype = C.c_int
    L.hs_eigs_gen_info.argtypes = [p_f64]
    L.hs_eigs_gen_info.restype = C.c_int
    for f in (L.hsk_eigs_coldot_d, L.hsk_eigs_coldot_z):
        f.argtypes = [i64, i64, vp, i64, vp, i64, C.POINTER(C.c_int), p_f64]
        f.restype = C.c_int
    for f in (L.hsk_eigs_rotate_d, L.hsk_eigs_rotate_z):
        f.argtypes = [i64, i64, i64, vp, i64, vp, i64, C.c_int, vp, i64]
        f.restype = C.c_int
    for f in (L.hsk_eigs_chol_inv_d, L.hsk_eigs_chol_inv_z):
        f.argtypes = [i64, vp, i64, vp, vp, C.POINTER(C.c_int)]
        f.restype = C.c_int
    L.hsk_small_eig_z.argtypes = [i64, vp, i64, vp, vp, i64]
    L.hsk_small_eig_z.restype = C.c_int
    L.hsk_eigs_phase_timing.argtypes = [C.c_int]
    L.hsk_eigs_phase_timing.restype = C.c_int
    L.hsk_eigs_phases.argtypes = [p_f64]
    L.hsk_eigs_phases.restype = C.c_int
    L.hsk_eigs_gen_mprod_seconds.argtypes = []
    L.hsk_eigs_gen_mprod_seconds.restype = C.c_double
    L.hs_logabsdet.argtypes = [vp, p_f64, p_f64]
    L.hs_logabsdet.restype = C.c_int
    L.hs_ulv_mode.argtypes = [vp, C.c_int]
    L.hs_ulv_mode.restype = C.c_int
    L.hs_hss_logabsdet.argtypes = [vp, p_f64, p_f64, p_f64]
    L.hs_hss_logabsdet.restype = C.c_int
    for f in (L.hsk_ulv_det_d, L.hsk_ulv_det_z):
        f.argtypes = [i64, p_i64, p_i64, p_f64, C.POINTER(C.c_int32), p_f64, C.POINTER(C.c_int32), p_f64]
        f.restype = C.c_int
    L.hs_selinv.argtypes = [vp, C.c_int, vp, vp, C.c_int, i64, vp]
    L.hs_selinv.restype = C.c_int
    L.hs_selinv_info.argtypes = [vp, p_f64]
    L.hs_selinv_info.restype = C.c_int
    L.hs_selinv_lr.argtypes = [vp, C.c_int, vp, vp, C.c_int, i64, vp]
    L.hs_selinv_lr.restype = C.c_int
    L.hs_selinv_lr_info.argtypes = [vp, p_f64]
    L.hs_selinv_lr_info.restype = C.c_int
    L.hs_interface_size.argtypes = [vp, p_i64]
    L.hs_interface_size.restype = C.c_int
    L.hs_interface_indices.argtypes = [vp, p_i64]
    L.hs_interface_indices.restype = C.c_int
    for f in (L.hs_interface_matrix_d, L.hs_interface_matrix_z):  # (F, S, lds, where, stream): S a host or a device address
        f.argtypes = [vp, vp, i64, C.c_int, vp]
        f.restype = C.c_int
    for ph in ("condense", "solve", "expand"):  # (F, trans, C, ldc, n, nrhs) on the host, the same on the device with a stream
        for sfx in ("_d", "_z"):
            f = getattr(L, "hs_interface_" + ph + sfx)
            f.argtypes = [vp, C.c_int, p_f64, i64, i64, i64]
            f.restype = C.c_int
            f = getattr(L, "hs_interface_" + ph + "_dev" + sfx)
            f.argtypes = [vp, C.c_int, vp, i64, i64, i64, vp]
            f.restype = C.c_int
    L.hs_interface_info.argtypes = [vp, p_f64]
    L.hs_interface_info.restype = C.c_int
    for f in (L.hsk_lu_product_d, L.hsk_lu_product_z):
        f.argtypes = [i64, p_f64, i64, C.POINTER(C.c_int32), p_f64, i64, p_f64]
        f.restype = C.c_int
    L.hs_analyze.argtypes = [C.c_int, i64, p_i64, p_i64, C.POINTER(hs_tree), C.POINTER(hs_options), i64, i64, C.POINTER(vp)]
    L.hs_analyze.restype = C.c_int
    L.hs_plan.argtypes = [C.c_int, i64, C.POINTER(hs_tree), C.POINTER(hs_options), i64, i64, C.POINTER(vp)]
    L.hs_plan.restype = C.c_int
    L.hs_numeric_begin.argtypes = [vp, vp, C.c_int]
    L.hs_numeric_begin.restype = C.c_int
    L.hs_numeric_levels.argtypes = [vp, i64, i64]
    L.hs_numeric_levels.restype = C.c_int
    L.hs_numeric_end.argtypes = [vp]
    L.hs_numeric_end.restype = C.c_int
    for f in (L.hs_solve_fwd_levels, L.hs_solve_bwd_levels):
        f.argtypes = [vp, vp, i64, i64, vp]
        f.restype = C.c_int
    for f in (L.hs_nlevels, L.hs_cut_level, L.hs_num_exchanges):
        f.argtypes = [vp]
        f.restype = i64
    L.hs_node_owner.argtypes = [vp, i64]
    L.hs_node_owner.restype = i64
    L.hs_exchange_info.argtypes = [vp, i64, p_i64]
    L.hs_exchange_info.restype = C.c_int
    L.hs_set_schur_buffer.argtypes = [vp, i64, vp]
    L.hs_set_schur_buffer.restype = C.c_int
    L.hs_exchange_kind.argtypes = [vp, i64]
    L.hs_exchange_kind.restype = i64
    L.hs_schur_pack_size.argtypes = [vp, i64, p_i64]
    L.hs_schur_pack_size.restype = C.c_int
    L.hs_schur_pack.argtypes = [vp, i64, vp, i64, vp]
    L.hs_schur_pack.restype = C.c_int
    L.hs_schur_unpack.argtypes = [vp, i64, vp, i64, vp]
    L.hs_schur_unpack.restype = C.c_int
    L.hs_flow_info.argtypes = [vp, p_i64]
    L.hs_flow_info.restype = C.c_int
    L.hs_sym_info.argtypes = [vp, p_i64]
    L.hs_sym_info.restype = C.c_int
    L.hs_equil_info.argtypes = [vp, p_i64]
    L.hs_equil_info.restype = C.c_int
    L.hs_equil_scales.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.hs_equil_scales.restype = C.c_int
    L.hs_hss_qr_order.argtypes = [C.c_int]
    L.hs_hss_qr_order.restype = C.c_int
    L.hs_hss_pack_size.argtypes = [vp, p_i64]
    L.hs_hss_pack_size.restype = C.c_int
    L.hs_hss_pack.argtypes = [vp, vp, i64, vp]
    L.hs_hss_pack.restype = C.c_int
    L.hs_hss_unpack.argtypes = [vp, i64, C.c_int, vp, C.POINTER(vp)]
    L.hs_hss_unpack.restype = C.c_int
    L.hs_pack_bnd.argtypes = [vp, i64, vp, vp, vp]
    L.hs_pack_bnd.restype = C.c_int
    L.hs_unpack_bnd.argtypes = [vp, i64, vp, vp, vp]
    L.hs_unpack_bnd.restype = C.c_int
    L.hs_extract_owned.argtypes = [vp, vp, vp, vp]
    L.hs_extract_owned.restype = C.c_int
    L.hs_comm_unique_id.argtypes = [vp]
    L.hs_comm_unique_id.restype = C.c_int
    L.hs_comm_create_rccl.argtypes = [vp, i64, i64, C.POINTER(vp)]
    L.hs_comm_create_rccl.restype = C.c_int
    L.hs_comm_create_host.argtypes = [HS_TRANSFER_FN, vp, i64, i64, C.POINTER(vp)]
    L.hs_comm_create_host.restype = C.c_int
    L.hs_comm_free.argtypes = [vp]
    L.hs_comm_free.restype = None
    L.hs_comm_kind.argtypes = [vp]
    L.hs_comm_kind.restype = C.c_char_p
    L.hs_comm_selftest.argtypes = [vp, i64]
    L.hs_comm_selftest.restype = C.c_int
    L.hs_comm_bandwidth.argtypes = [vp, i64, i64, C.POINTER(C.c_double)]
    L.hs_comm_bandwidth.restype = C.c_int
    L.hs_set_comm.argtypes = [vp, vp]
    L.hs_set_comm.restype = C.c_int
    for f in (L.hs_gmres_d, L.hs_gmres_z):
        f.argtypes = [vp, i64, p_i64, p_i64, vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, i64, i64, p_f64, p_i64, C.POINTER(C.c_int), vp]
        f.restype = C.c_int
    for f in (L.hs_gmres_block_d, L.hs_gmres_block_z):
        f.argtypes = [vp, i64, p_i64, p_i64, vp, vp, i64, vp, i64, i64, C.c_int, C.c_int, C.c_double, C.c_double, i64, i64, p_f64, p_i64, C.POINTER(C.c_int), vp]
        f.restype = C.c_int
    for f in (L.hs_gmres_t_d, L.hs_gmres_t_z):
        f.argtypes = [vp, C.c_int, i64, p_i64, p_i64, vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, i64, i64, p_f64, p_i64, C.POINTER(C.c_int), vp]
        f.restype = C.c_int
    for f in (L.hs_gmres_block_t_d, L.hs_gmres_block_t_z):
        f.argtypes = [vp, C.c_int, i64, p_i64, p_i64, vp, vp, i64, vp, i64, i64, C.c_int, C.c_int, C.c_double, C.c_double, i64, i64, p_f64, p_i64, C.POINTER(C.c_int), vp]
        f.restype = C.c_int
    for f in (L.hsk_spmm_op_d, L.hsk_spmm_op_z):
        f.argtypes = [C.c_int, i64, p_i64, p_i64, vp, vp, i64, vp, i64, vp, i64, i64]
        f.restype = C.c_int
    L.hs_gmres_block_info.argtypes = [p_f64]
    L.hs_gmres_block_info.restype = C.c_int
    for f in (L.hsk_spmm_d, L.hsk_spmm_z):
        f.argtypes = [i64, p_i64, p_i64, vp, vp, i64, vp, i64, vp, i64, i64]
        f.restype = C.c_int
    L.hs_maxrank.argtypes = [vp]
    L.hs_maxrank.restype = i64
    L.hs_is_complex.argtypes = [vp]
    L.hs_is_complex.restype = C.c_int
    L.hs_size.argtypes = [vp]
    L.hs_size.restype = i64
    L.hs_free.argtypes = [vp]
    L.hs_free.restype = None
    L.hs_last_error.argtypes = []
    L.hs_last_error.restype = C.c_char_p
    L.hs_last_error_info.argtypes = []
    L.hs_last_error_info.restype = i64
    L.hs_get_stats.argtypes = [vp, C.POINTER(hs_stats)]
    L.hs_get_stats.restype = C.c_int
    L.hs_node_info.argtypes = [vp, i64, p_i64, p_i64, p_i64]
    L.hs_node_info.restype = C.c_int
    L.hs_symbolic_from_elimtree.argtypes = [i64, p_i64, p_i64, p_i64, p_i64, p_i64, i64, p_i64, p_i64, i64, C.POINTER(vp)]
    L.hs_symbolic_from_elimtree.restype = C.c_int
    L.hs_symbolic_from_graph.argtypes = [i64, p_i64, p_i64, i64, C.POINTER(vp)]
    L.hs_symbolic_from_graph.restype = C.c_int
    L.hs_symbolic_size.argtypes = [vp]
    L.hs_symbolic_size.restype = i64
    L.hs_symbolic_perm.argtypes = [vp]
    L.hs_symbolic_perm.restype = p_i64
    L.hs_symbolic_tree.argtypes = [vp, C.POINTER(hs_tree)]
    L.hs_symbolic_tree.restype = C.c_int
    L.hs_symbolic_free.argtypes = [vp]
    L.hs_symbolic_free.restype = None
    L.hs_node_ranks.argtypes = [vp, i64, p_i64, p_i64]
    L.hs_node_ranks.restype = C.c_int
    L.hs_node_export.argtypes = [vp, i64, C.c_int, p_f64]
    L.hs_node_export.restype = C.c_int
    L.hs_node_export_piv.argtypes = [vp, i64, p_i64]
    L.hs_node_export_piv.restype = C.c_int
    L.hs_device_info.argtypes = [C.c_char_p, i64, p_i64, p_i64]
    L.hs_device_info.restype = C.c_int
    for f in (L.hsk_gemm_d, L.hsk_gemm_z):
        f.argtypes = [i64, i64, i64, p_f64, i64, p_f64, i64, p_f64, i64, C.c_int, C.c_int, p_f64]
        f.restype = C.c_int
    L.hsk_gemm_op_d.argtypes = [i64, p_i64, p_i64, i64, i64, i64, p_f64, p_f64, p_f64, p_i64, C.c_int, p_f64]
    L.hsk_gemm_op_d.restype = C.c_int
    L.hsk_gemm_lds_enable.argtypes = [C.c_int]
    L.hsk_gemm_lds_enable.restype = C.c_int
    for f in (L.hsk_gemm_lds_launches, L.hsk_gemm_lds_edge_launches, L.hsk_gemm_reg_launches):
        f.argtypes = [C.c_int]
        f.restype = C.c_longlong
    L.hsk_gemm_lds_route.argtypes = [C.c_int] * 5
    L.hsk_gemm_lds_route.restype = C.c_int
    L.hsk_gemm_schur_d.argtypes = [i64, p_i64, p_i64, p_f64, p_f64, p_f64, C.c_int, p_i64, p_i64, C.c_int, p_f64]
    L.hsk_gemm_schur_d.restype = C.c_int
    L.hsk_trsm_inv_d.argtypes = [i64, p_i64, p_i64, i64, i64, i64, i64, i64, p_f64, p_f64, C.c_int, p_i64]
    L.hsk_trsm_inv_d.restype = C.c_int
    L.hsk_trsm_strip_enable.argtypes = [C.c_int]
    L.hsk_trsm_strip_enable.restype = C.c_int
    for f in (L.hsk_trsm_strip_launches, L.hsk_trsm_half_launches, L.hsk_lookahead_runs):
        f.argtypes = [C.c_int]
        f.restype = C.c_longlong
    for f in (L.hsk_front_factor_d, L.hsk_front_factor_z):
        f.argtypes = [i64, i64, i64, p_f64, p_f64, p_f64, p_f64, p_i64, p_i64, p_f64]
        f.restype = C.c_int
    for f in (L.hsk_front_batch_d, L.hsk_front_batch_z, L.hsk_front_batch_sym_d, L.hsk_front_batch_sym_z):
        f.argtypes = [i64, p_i64, p_i64, C.c_int, p_f64, p_f64, p_f64, p_f64, p_i64, p_i64, p_i64, p_f64, p_f64, p_f64, p_f64, p_f64]
        f.restype = C.c_int
    for f in (L.hsk_sweep_level_d, L.hsk_sweep_level_z):
        f.argtypes = [i64, p_i64, p_i64, C.c_int, p_f64, p_i64, i64, p_i64, p_f64, C.c_int, C.c_int, C.c_int, p_f64, p_f64, p_i64, p_i64, p_i64,
                      p_f64, p_f64, p_f64, p_f64, p_f64, p_f64, p_f64, p_f64, C.POINTER(C.c_int)]
        f.restype = C.c_int
    L.hsk_flow_tall_rule.argtypes = [C.c_int, i64, i64]
    L.hsk_flow_tall_rule.restype = C.c_int
    for f in (L.hsk_lowrank_d, L.hsk_lowrank_z):
        f.argtypes = [i64, i64, p_f64, C.c_double, C.c_double, i64, i64, p_i64, p_f64, p_f64, i64]
        f.restype = C.c_int
    p_i32 = C.POINTER(C.c_int32)
    L.hsk_qr_params.argtypes = [p_f64]
    L.hsk_qr_params.restype = C.c_int
    for f in (L.hsk_qr_chol_d, L.hsk_qr_chol_z):
        f.argtypes = [i64, p_i32, p_i32, p_f64, p_f64, p_f64, p_i32, p_f64, p_f64, p_f64, p_f64, p_i32, p_i32]
        f.restype = C.c_int
    L.hsk_qr_select.argtypes = [i64, p_i32, p_i32, p_i32, p_i32, p_f64, p_f64]
    L.hsk_qr_select.restype = C.c_int
    for f in (L.hsk_qr_refine_d, L.hsk_qr_refine_z):
        f.argtypes = [i64, p_i32, p_i32, p_f64, p_i32, p_i32, p_f64, p_f64, C.c_int, C.c_double, C.c_double, C.c_double, p_i32, p_f64, p_f64, p_f64, p_i32, p_i32, p_i64]
        f.restype = C.c_int
    L.hs_hss_options_default.argtypes = [C.POINTER(hs_hss_options)]
    L.hs_hss_options_default.restype = None
    for f in (L.hs_hss_compress_d, L.hs_hss_compress_z):
        f.argtypes = [i64, vp, i64, C.c_int, C.POINTER(hs_hss_options), C.POINTER(vp)]
        f.restype = C.c_int
    for f in (L.hs_hss_compress_ex_d, L.hs_hss_compress_ex_z):
        f.argtypes = [i64, vp, i64, C.c_int, p_i64, C.POINTER(hs_hss_options), vp, C.POINTER(vp)]
        f.restype = C.c_int
    for f in (L.hs_hss_compress_lru_d, L.hs_hss_compress_lru_z):
        f.argtypes = [i64, vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, C.c_int, p_i64, C.POINTER(hs_hss_options), vp, C.POINTER(vp)]
        f.restype = C.c_int
    for f in (L.hs_hss_compress_lru_multi_d, L.hs_hss_compress_lru_multi_z):
        f.argtypes = [i64, p_i64, C.POINTER(vp), p_i64, C.POINTER(vp), p_i64, C.POINTER(vp), p_i64, C.POINTER(vp), p_i64, p_i64, p_i64, C.POINTER(p_i64),
                      C.POINTER(C.POINTER(hs_hss_options)), vp, C.POINTER(vp)]
        f.restype = C.c_int
    for f in (L.hs_hss_rank, L.hs_hss_size, L.hs_hss_samples, L.hs_hss_num_nodes, L.hs_hss_bytes):
        f.argtypes = [vp]
        f.restype = i64
    L.hs_node_schur_hss.argtypes = [vp, i64, C.POINTER(hs_hss_options), C.POINTER(vp)]
    L.hs_node_schur_hss.restype = C.c_int
    L.hs_hss_set_stream.argtypes = [vp, vp]
    L.hs_hss_set_stream.restype = C.c_int
    L.hs_hss_node_info.argtypes = [vp, i64, p_i64]
    L.hs_hss_node_info.restype = C.c_int
    L.hs_hss_node_data.argtypes = [vp, i64, p_i64, vp, vp, vp, vp]
    L.hs_hss_node_data.restype = C.c_int
    L.hs_hss_getindex.argtypes = [vp, p_i64, i64, p_i64, i64, vp, i64, C.c_int]
    L.hs_hss_getindex.restype = C.c_int
    L.hs_hss_trim.argtypes = []
    L.hs_hss_trim.restype = i64
    L.hs_hss_basis.argtypes = [vp, i64, vp, i64, C.c_int]
    L.hs_hss_basis.restype = C.c_int
    L.hs_hss_expand.argtypes = [vp, vp, i64, C.c_int]
    L.hs_hss_expand.restype = C.c_int
    L.hs_hss_mul.argtypes = [vp, vp, i64, vp, i64, i64, C.c_int]
    L.hs_hss_mul.restype = C.c_int
    L.hs_hss_mul_t.argtypes = [vp, vp, i64, vp, i64, i64, C.c_int]
    L.hs_hss_mul_t.restype = C.c_int
    L.hs_hss_child.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.hs_hss_child.restype = C.c_int
    L.hs_hss_prune_leaves.argtypes = [vp, C.POINTER(vp)]
    L.hs_hss_prune_leaves.restype = C.c_int
    L.hs_hss_compatible.argtypes = [vp, vp]
    L.hs_hss_compatible.restype = C.c_int
    L.hs_hss_depth.argtypes = [vp]
    L.hs_hss_depth.restype = i64
    L.hs_hss_offdiag.argtypes = [vp, C.c_int, vp, i64, vp, i64, C.c_int]
    L.hs_hss_offdiag.restype = C.c_int
    for f in (L.hs_hss_compress_blockop_d, L.hs_hss_compress_blockop_z):
        f.argtypes = [C.POINTER(hs_hss_blockop), vp, i64, vp, i64, vp, i64, i64, i64, p_i64, C.POINTER(hs_hss_options), vp, C.POINTER(vp)]
        f.restype = C.c_int
    L.hs_hss_blockop_apply.argtypes = [C.POINTER(hs_hss_blockop), C.c_int, vp, i64, vp, i64, i64, C.c_int, vp]
    L.hs_hss_blockop_apply.restype = C.c_int
    L.hs_hss_factor.argtypes = [vp]
    L.hs_hss_factor.restype = C.c_int
    L.hs_hss_ldiv.argtypes = [vp, vp, i64, i64, C.c_int]
    L.hs_hss_ldiv.restype = C.c_int
    L.hs_hss_ldiv_t.argtypes = [vp, C.c_int, vp, i64, i64, C.c_int]
    L.hs_hss_ldiv_t.restype = C.c_int
    for f in (L.hsk_ulv_t_group_d, L.hsk_ulv_t_group_z):
        f.argtypes = [i64, p_i64, p_f64, i64, p_f64, i64, p_f64, i64, C.c_int]
        f.restype = C.c_int
    L.hs_hss_time.argtypes = [vp, C.c_int]
    L.hs_hss_time.restype = C.c_double
    L.hs_hss_free.argtypes = [vp]
    L.hs_hss_free.restype = None
    L.hsk_bisect_perm.argtypes = [i64, p_i64, p_i64, i64, p_i64, p_i64]
    L.hsk_bisect_perm.restype = C.c_int
    L.hs_stream_order.argtypes = [vp, vp, C.c_int]
    L.hs_stream_order.restype = C.c_int
    L.hs_trim.argtypes = []
    L.hs_trim.restype = i64
    L.hs_probs_stats_mode.argtypes = [C.c_int]
    L.hs_probs_stats_mode.restype = C.c_int
    L.hs_probs_stats.argtypes = [p_f64]
    L.hs_probs_stats.restype = C.c_int
    L.hsk_leaf_envelope.argtypes = [i64, p_i64, p_i64, C.POINTER(C.c_int32), i64, i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.hsk_leaf_envelope.restype = C.c_int
    L.hsk_envelope_enable.argtypes = [C.c_int]
    L.hsk_envelope_enable.restype = C.c_int
    L.hsk_branch_envelope.argtypes = [i64, p_i64, p_i64, C.POINTER(C.c_int32), i64, i64, i64, i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.hsk_branch_envelope.restype = C.c_int
    L.hsk_front_batch_env_d.argtypes = [i64, p_i64, p_i64, C.c_int, p_f64, C.POINTER(C.c_int32), p_f64, p_f64, p_f64, p_i64, p_i64, p_i64]
    L.hsk_front_batch_env_d.restype = C.c_int
    L.hsk_branch_envelope_enable.argtypes = [C.c_int]
    L.hsk_branch_envelope_enable.restype = C.c_int
    L.hsk_env_order_enable.argtypes = [C.c_int]
    L.hsk_env_order_enable.restype = C.c_int
    L.hsk_env_tile_order.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.hsk_env_tile_order.restype = C.c_int
    L.hsk_env_phase_order.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int] + [C.POINTER(C.c_int32)] * 3
    L.hsk_env_phase_order.restype = C.c_int
    L.hsk_env_perm.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_int32)] + [C.c_int] * 10 + [C.POINTER(C.c_uint16)]
    L.hsk_env_perm.restype = C.c_int
    L.hsk_env_perm_slot_limit.argtypes = [C.c_int]
    L.hsk_env_perm_slot_limit.restype = C.c_int
    L.hsk_env_perm_min_tiles.argtypes = [C.c_int]
    L.hsk_env_perm_min_tiles.restype = C.c_int
    L.hsk_env_perm_launches.argtypes = [C.c_int]
    L.hsk_env_perm_launches.restype = C.c_longlong
    L.hsk_op_flops_mode.argtypes = [C.c_int]
    L.hsk_op_flops_mode.restype = C.c_int
    L.hsk_op_flops.argtypes = [p_f64]
    L.hsk_op_flops.restype = C.c_int
    L.hsk_flow_pingpong_us.argtypes = [C.c_int, C.c_int]
    L.hsk_flow_pingpong_us.restype = C.c_double
    L.hsk_mfma_f64_peak.argtypes = [C.c_int, C.c_int]
    L.hsk_mfma_f64_peak.restype = C.c_double
    L.hsk_mfma_f64_peak_random.argtypes = [C.c_int, C.c_int]
    L.hsk_mfma_f64_peak_random.restype = C.c_double
    _lib = L
    return L


class DimensionMismatch(ValueError):
    """Julia ``DimensionMismatch`` (blockmatrix.jl:13-16,116-117; nesteddissection.jl:107)."""


class SingularException(ArithmeticError):
    """``LinearAlgebra.SingularException`` -- what ``\\`` raises in the reference on an exactly singular block."""


class DeviceError(RuntimeError):
    """No usable gfx950 device / HIP runtime failure.  There is no CPU fallback."""


class UnsupportedError(NotImplementedError):
    pass


class NoConvergence(ArithmeticError):
    """An iteration stopped at its limit before every wanted result met the tolerance; ``partial`` carries what it had."""

    def __init__(self, msg, partial=None):
        super().__init__(msg)
        self.partial = partial


def check(status):
    if status == HS_OK:
        return
    msg = lib().hs_last_error().decode("utf-8", "replace")
    info = lib().hs_last_error_info()
    exc = {
        HS_ERR_ARGUMENT: ValueError,  # ArgumentError
        HS_ERR_DIMENSION: DimensionMismatch,
        HS_ERR_TREE: RuntimeError,  # ErrorException (factorization.jl:25)
        HS_ERR_SINGULAR: SingularException,
        HS_ERR_HSS_LEAF: RuntimeError,
        HS_ERR_DEVICE: DeviceError,
        HS_ERR_NOMEM: MemoryError,
        HS_ERR_UNSUPPORTED: UnsupportedError,
    }.get(status, RuntimeError)
    e = exc(msg)
    e.info = info
    e.status = status
    raise e
