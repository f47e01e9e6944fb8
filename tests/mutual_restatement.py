"""The definition of the mutual nearest-neighbour flag (include/oryon_hip.h, K1m) in a few lines of numpy, and a brute-force float64
all-pairs matcher for tiny inputs.  Shared by test_match_mutual_cabi.py (CPU) and the GPU tests; never imports the code under test."""
import numpy as np


def mutual_flags(argmin, valid, rev_argmin):
    """mutual[i] = valid[i] && rev_argmin[argmin[i]] == i, for ONE pair: argmin / valid over its n_a anchor rows, rev_argmin over its
    n_q query rows."""
    argmin, valid, rev_argmin = np.asarray(argmin, np.int64), np.asarray(valid).astype(bool), np.asarray(rev_argmin, np.int64)
    if len(rev_argmin) == 0 or len(argmin) == 0:
        return np.zeros(len(argmin), dtype=bool)
    return valid & (rev_argmin[argmin] == np.arange(len(argmin)))


def brute_force(a, q, thr):
    """a [n_a, C], q [n_q, C] (any scale) -> dict of both directions of 0.5 (1 - cos) in float64, first index on ties, and the mutual
    flags written out as the definition's double loop (not through mutual_flags)."""
    a, q = np.asarray(a, np.float64), np.asarray(q, np.float64)
    an = a / np.linalg.norm(a, axis=1, keepdims=True)
    qn = q / np.linalg.norm(q, axis=1, keepdims=True)
    d = 0.5 * (1.0 - an @ qn.T)
    argmin, rev_argmin = d.argmin(axis=1), d.argmin(axis=0)               # numpy's argmin returns the first minimum
    valid = d.min(axis=1) < thr
    mutual = np.zeros(len(a), dtype=bool)
    for i in range(len(a)):
        j = int(argmin[i])
        mutual[i] = bool(valid[i]) and all(d[i, j] <= d[k, j] for k in range(len(a))) and not any(d[k, j] == d[i, j] for k in range(i))
    return dict(dist=d, argmin=argmin, valid=valid, rev_argmin=rev_argmin, min_dist=d.min(axis=1), rev_min_dist=d.min(axis=0), mutual=mutual)
