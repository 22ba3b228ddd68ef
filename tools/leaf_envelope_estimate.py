"""usage (no GPU): python tools/leaf_envelope_estimate.py NX NY NZ [poisson|helmholtz] -- multiply-adds of the leaf level inside the block envelope
(csrc/hs_envelope.h; block size G = 32, or the environment variable G) against the dense count, on the tree bench.py prepares (leaves of <= 4,096)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hsamd  # noqa: E402

hs = hsamd.load()
shape = tuple(int(x) for x in sys.argv[1:4])
kind = sys.argv[4] if len(sys.argv) > 4 else "poisson"
A, b, nd = hs.problems.make_problem(shape, kind=kind, nmax=4096, rhs="randn")
nd, nd_loc = hs.symfact(nd)
perm = hs.postorder(nd)
Acsr = A[perm - 1][:, perm - 1].tocsr()
nd = hs.permuted(nd, hs.invperm(perm))
G = int(os.environ.get("G", "32"))


def leaves(x):
    if x.left is None and x.right is None:
        yield x
    else:
        for c in (x.left, x.right):
            if c is not None:
                yield from leaves(c)


tot_d = tot_e = 0.0
seen = set()
for lf in leaves(nd):
    it, bd = np.asarray(lf.int) - 1, np.asarray(lf.bnd) - 1
    ni, nb = len(it), len(bd)
    idx = np.concatenate([it, bd])
    F = Acsr[idx][:, idx].tocoo()
    r, c = F.row, F.col
    nbk = (ni + nb + G - 1) // G
    fL, fU = np.arange(nbk), np.arange(nbk)  # (blocks counted straight through the front: an estimate, the library counts boundary blocks from ni)
    np.minimum.at(fL, r // G, c // G)
    np.minimum.at(fU, c // G, r // G)
    fl = 0.0
    for k in range((ni + G - 1) // G):
        rows = np.sum((np.arange(nbk) > k) & (fL <= k))
        cols = np.sum((np.arange(nbk) > k) & (fU <= k))
        fl += 2.0 * G ** 3 * rows * cols
    dense = 2 / 3 * ni ** 3 + 2 * ni * ni * nb + 2 * ni * nb * nb
    tot_d += dense
    tot_e += fl
    if (ni, nb) not in seen:
        seen.add((ni, nb))
        ii = (r < ni) & (c < ni)
        bw = int(np.max(np.abs(r[ii] - c[ii]))) if ni else 0
        print("leaf ni=%d nb=%d  interior bandwidth=%d  dense=%.3g  envelope(%d)=%.3g  ratio=%.3f" % (ni, nb, bw, dense, G, fl, fl / dense))
print("all leaves: dense %.4g  envelope %.4g  ratio %.3f" % (tot_d, tot_e, tot_e / tot_d))
