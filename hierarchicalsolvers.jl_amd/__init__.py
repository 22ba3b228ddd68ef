"""MI355X-native nested-dissection elimination (HierarchicalSolvers.jl hot path).

Host-side mirror of the reference's public API (``src/HierarchicalSolvers.jl:20-28``)
above the C ABI in ``include/hs_solver.h``.  The directory name contains a dot,
so import it through ``hsamd`` (repo root) which registers it as
``hierarchicalsolvers_jl_amd``.
"""
from .nesteddissection import (  # noqa: F401
    NDNode, isleaf, isbranch, depth, symfact, postorder, postorder_nodes, permuted, invperm,
    contigious, parse_elimtree, serialize_elimtree, getinterior, getboundary, flatten_tree, native_symbolic, native_graph_symbolic,
)
from . import problems  # noqa: F401
from .solver import SolverOptions, chkopts, factor, factorize, FactorNode, TransposedFactor, ldiv, maxrank, trim, transpose, adjoint, opnorm, opnormestinv, condest, ldiv_refine, ldiv_refine_block, ldiv_refine_block_info, logabsdet, logdet, det, ulv_mode, selinv, selinv_diag, selinv_info, selinv_lr, selinv_lr_diag, selinv_lr_info, sym_info, equil_info, equil_scales, ldiv_block, ldiv_block_t, ldiv_ulv, ldiv_block_info, mul, mul_info, factor_error, ldiv_sparse, ldiv_sparse_plan, ldiv_sparse_info, inv_entries, sensitivity, sensitivity_matrix, misfit, sens_info, tangent, gn_hessvec, gn_diag, gn_info, ModifiedFactor, modify, ldiv_mod, DemotedFactor, demote, ldiv_f32, eigs, eigs_info, eigs_gen_info, interface_indices, schur_complement, condense, interface_solve, expand, interface_info  # noqa: F401,E402
from ._lib import DimensionMismatch, SingularException, DeviceError, UnsupportedError, NoConvergence  # noqa: F401,E402
from . import _lib  # noqa: F401,E402
from . import dist  # noqa: F401,E402
from .gmres import gmres, gmres_block, gmres_block_info  # noqa: F401,E402
from . import hss  # noqa: F401,E402
