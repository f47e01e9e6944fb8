"""One-to-many correspondences (include/oryon_hip.h, K1n / K1k), stated twice in numpy.  Imports nothing under test.

ranks: the K ranks of every anchor of one pair, given a distance matrix.  expand: the rows the drawn slots emit, given their candidate
tables.  brute_force: the ranks from raw descriptors in float64, the candidate sets written as the loops they are."""
import numpy as np


def ranks(dist, roi_q, W_q, N, K):
    """dist [n_a, n_q] (any float dtype; float32 bits are compared as they are), roi_q [n_q] linear pixel indices in a map W_q wide,
    N the integer radius.  -> (cand_dist [K, n_a] dist.dtype, cand_argmin [K, n_a] int64).  Rank 1 is the argmin (first index on
    ties); rank r the minimum over the rows outside the discs round the pixels of ranks 1 .. r-1; (inf, -1) from the first rank
    that has no candidate on."""
    dist = np.asarray(dist)
    n_a, n_q = dist.shape
    roi_q = np.asarray(roi_q, dtype=np.int64)
    y, x = roi_q // W_q, roi_q % W_q
    cd = np.full((K, n_a), np.inf, dtype=dist.dtype)
    ca = np.full((K, n_a), -1, dtype=np.int64)
    for i in range(n_a):
        cand = np.ones(n_q, dtype=bool)
        for r in range(K):
            js = np.nonzero(cand)[0]
            if len(js) == 0:
                break
            k = int(np.argmin(dist[i, js]))                           # first candidate index on ties
            if r > 0 and not dist[i, js[k]] < np.inf:                 # nothing finite is left: no candidate row
                break
            j = int(js[k])
            cd[r, i], ca[r, i] = dist[i, j], j
            cand &= (y - y[j]) ** 2 + (x - x[j]) ** 2 >= N * N        # integers
    return cd, ca


def expand(slots, cand_dist, cand_argmin, thr, margin):
    """slots: n; cand_dist / cand_argmin [K, >= n]: the ranks of the anchor row in every slot.  thr: K1's float32 threshold (valid is
    d < thr), margin >= 0 a float32 slack.  -> (slot [n_rows], rank [n_rows]) int64 in (slot, rank) order: rank 1 always, rank
    r >= 2 iff c_r >= 0 and d_r < thr and d_r <= float32(d_1 + margin)."""
    cd = np.asarray(cand_dist).astype(np.float32)
    ca = np.asarray(cand_argmin)
    thr, margin = np.float32(thr), np.float32(margin)
    out_s, out_r = [], []
    for s in range(int(slots)):
        out_s.append(s)
        out_r.append(1)
        with np.errstate(invalid="ignore", over="ignore"):
            lim = np.float32(cd[0, s] + margin)                       # float32 sum, round to nearest
        for r in range(1, cd.shape[0]):
            if ca[r, s] >= 0 and cd[r, s] < thr and cd[r, s] <= lim:
                out_s.append(s)
                out_r.append(r + 1)
    return np.asarray(out_s, dtype=np.int64), np.asarray(out_r, dtype=np.int64)


def brute_force(a, q, roi_q, W_q, N, K):
    """Float64 all-pairs on raw descriptor rows a [n_a, C], q [n_q, C]: cosine distance 0.5 (1 - cos) and the K ranks.
    -> (cand_dist [K, n_a] float64, cand_argmin [K, n_a] int64)."""
    a, q = np.asarray(a, dtype=np.float64), np.asarray(q, dtype=np.float64)
    n_a, n_q = len(a), len(q)
    an = a / np.linalg.norm(a, axis=1, keepdims=True)
    qn = q / np.linalg.norm(q, axis=1, keepdims=True) if n_q else q
    cd = np.full((K, n_a), np.inf)
    ca = np.full((K, n_a), -1, dtype=np.int64)
    for i in range(n_a):
        d = [0.5 * (1.0 - float(an[i] @ qn[j])) for j in range(n_q)]
        centres = []
        for r in range(K):
            best, bj = np.inf, -1
            for j in range(n_q):
                yj, xj = divmod(int(roi_q[j]), W_q)
                outside = True
                for ys, xs in centres:
                    if (yj - ys) ** 2 + (xj - xs) ** 2 < N * N:
                        outside = False
                if outside and d[j] < best:
                    best, bj = d[j], j
            if bj < 0:
                break
            cd[r, i], ca[r, i] = best, bj
            centres.append(divmod(int(roi_q[bj]), W_q))
    return cd, ca
