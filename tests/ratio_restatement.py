"""The ratio test with an exclusion disc (include/oryon_hip.h, K1r), stated twice in numpy.  Imports nothing under test.

second_and_keep: the definition for one pair, given a distance matrix.  brute_force: the same from raw descriptors in float64, the
candidate set written as the double loop it is."""
import numpy as np


def second_and_keep(dist, roi_q, W_q, r, argmin, gate, ratio, min_dist=None):
    """dist [n_a, n_q] (any float dtype; float32 bits are compared as they are), roi_q [n_q] linear pixel indices in a map W_q wide,
    r the integer radius, argmin [n_a], gate [n_a] bool or None (all ones), ratio a float in (0, 1].
    -> (second_dist [n_a] dist.dtype, second_argmin [n_a] int64, keep [n_a] bool); min_dist defaults to dist[i, argmin[i]].
    The product ratio * second_dist is rounded to float32, the comparison is made on float32 values."""
    dist = np.asarray(dist)
    n_a, n_q = dist.shape
    roi_q = np.asarray(roi_q, dtype=np.int64)
    y, x = roi_q // W_q, roi_q % W_q
    second = np.full(n_a, np.inf, dtype=dist.dtype)
    sidx = np.zeros(n_a, dtype=np.int64)
    for i in range(n_a):
        if n_q == 0:
            continue
        j0 = int(argmin[i])
        cand = (y - y[j0]) ** 2 + (x - x[j0]) ** 2 >= r * r           # integers
        js = np.nonzero(cand)[0]
        if len(js) == 0:
            continue
        k = int(np.argmin(dist[i, js]))                               # first candidate index on ties
        if dist[i, js[k]] < np.inf:
            second[i], sidx[i] = dist[i, js[k]], js[k]
    if min_dist is None:
        min_dist = np.array([dist[i, int(argmin[i])] if n_q else np.inf for i in range(n_a)], dtype=dist.dtype)
    return second, sidx, keep_flags(min_dist, second, gate, ratio)


def keep_flags(min_dist, second_dist, gate, ratio):
    """keep[i] = gate[i] && min_dist[i] <= float32(ratio * second_dist[i]); gate None counts as all ones; inf keeps the row."""
    second_dist = np.asarray(second_dist)
    g = np.ones(len(second_dist), dtype=bool) if gate is None else np.asarray(gate).astype(bool)
    with np.errstate(invalid="ignore"):
        cut = np.float32(ratio) * second_dist.astype(np.float32)      # float32 product, round to nearest
        return g & (np.asarray(min_dist).astype(np.float32) <= cut)


def brute_force(a, q, roi_q, W_q, r, ratio, thr):
    """Float64 all-pairs on raw descriptor rows a [n_a, C], q [n_q, C]: cosine distance 0.5 (1 - cos), the nearest row, the nearest
    row outside the disc, keep with gate = min_dist < thr.  -> dict of min_dist, argmin, second_dist, second_argmin, keep."""
    a, q = np.asarray(a, dtype=np.float64), np.asarray(q, dtype=np.float64)
    n_a, n_q = len(a), len(q)
    an = a / np.linalg.norm(a, axis=1, keepdims=True)
    qn = q / np.linalg.norm(q, axis=1, keepdims=True) if n_q else q
    out = dict(min_dist=np.full(n_a, np.inf), argmin=np.zeros(n_a, dtype=np.int64), second_dist=np.full(n_a, np.inf),
               second_argmin=np.zeros(n_a, dtype=np.int64), keep=np.zeros(n_a, dtype=bool))
    for i in range(n_a):
        d = [0.5 * (1.0 - float(an[i] @ qn[j])) for j in range(n_q)]
        for j in range(n_q):
            if d[j] < out["min_dist"][i]:
                out["min_dist"][i], out["argmin"][i] = d[j], j
        if n_q:
            ys, xs = divmod(int(roi_q[out["argmin"][i]]), W_q)
            for j in range(n_q):
                yj, xj = divmod(int(roi_q[j]), W_q)
                if (yj - ys) ** 2 + (xj - xs) ** 2 >= r * r and d[j] < out["second_dist"][i]:
                    out["second_dist"][i], out["second_argmin"][i] = d[j], j
        out["keep"][i] = out["min_dist"][i] < thr and out["min_dist"][i] <= ratio * out["second_dist"][i]
    return out
