"""Shared by tests/test_interface_host.py and tests/test_interface_gpu.py: grid problems whose tree keeps a chosen interface at the root."""
import numpy as np


def interface_ids(shape):
    """The middle grid line / plane across the first axis, plus DOFs 0, 7 and n - 1 (0-based, ascending)."""
    n = int(np.prod(shape))
    ids = np.arange(n, dtype=np.int64).reshape(shape, order="F")  # x fastest = ascending global id
    mid = ids[shape[0] // 2].reshape(-1)
    return np.unique(np.concatenate([mid, [0, 7, n - 1]]))


def interface_problem(hs, kind, shape, nmax, with_interface=True):
    """``A`` permuted to the factored (post-)order, its tree, and the interface in that order (the trailing block when there is one)."""
    A0 = hs.problems.grid_matrix(shape, kind).tocsc()
    n = A0.shape[0]
    iface0 = interface_ids(shape) if with_interface else np.zeros(0, dtype=np.int64)
    raw = hs.problems.graph_nested_dissection(A0, nmax, interface=iface0 if with_interface else None)
    arrays = hs.serialize_elimtree(raw)
    nd, nd_loc = hs.symfact(raw)
    perm = hs.postorder(nd)  # 1-based
    A = A0[perm - 1][:, perm - 1].tocsc()
    A.sort_indices()
    nd = hs.permuted(nd, hs.invperm(perm))
    inv = np.zeros(n, dtype=np.int64)
    inv[perm - 1] = np.arange(n)
    return dict(A=A, A0=A0, nd=nd, nd_loc=nd_loc, perm=perm, arrays=arrays, iface0=iface0, iface=np.sort(inv[iface0]), n=n)


def dense_schur(A, idx):
    """``A_bb - A_bi A_ii^-1 A_ib`` with SuperLU on ``A_ii``; also returns the interior ids."""
    import scipy.sparse.linalg as spla

    n = A.shape[0]
    mask = np.ones(n, dtype=bool)
    mask[idx] = False
    ii = np.flatnonzero(mask)
    A = A.tocsc()
    Aii = A[ii][:, ii].tocsc()
    Aib = A[ii][:, idx].toarray()
    Abi = A[idx][:, ii]
    Abb = A[idx][:, idx].toarray()
    return Abb - Abi @ spla.splu(Aii).solve(Aib), ii
