"""Seeded inputs of the PointDSC size / configuration sweep (helper of test_pdsc_restatement.py and test_gpu_pointdsc_sizes.py; not a
test module).

One generator makes every pair: `src` uniform in a cube (side `scale`; at side 1 about 2, 8 and 15 rows fall inside R = 0.1 of a row at
n = 640, 2176 and 4096, so the NMS decides something), `tgt` = R0 src + t0 + 3 mm of noise for 60 % of the rows and uniform for the
rest, unit feature rows, confidences quantised to 1/64 (exact ties) with zeros and negatives, and a few rows duplicated bit for bit in
every array (the matcher produces such duplicates; they are ties that only the index resolves).  Rows that would put an NMS distance
test within GAP of the radius are drawn again: a condition on the inputs, never a tolerance."""
import functools

import numpy as np

import pdsc_restatement as rs

GAP = 1e-6            # no NMS distance test that decides anything is closer than this to the radius
RADIUS = 0.1
N_DUP = 6


def rotation(rng, angle=None):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = rng.uniform(0.5, 2.5) if angle is None else angle
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


@functools.lru_cache(maxsize=None)
def make_case(n, seed=0, C=128, scale=1.0, radius=RADIUS):
    """dict(src, tgt [n,3], feat [n,C], conf [n], T_gt [4,4] float64, inlier [n] bool), all fp32 unless stated; read-only by
    convention (the cache hands the same arrays to every test)."""
    rng = np.random.default_rng(1000 * seed + n)
    R0, t0 = rotation(rng), rng.uniform(-0.5, 0.5, 3) * scale
    inlier = rng.random(n) < 0.6
    conf = (np.round(rng.uniform(-0.4, 1.6, n) * 64) / 64).astype(np.float32)
    conf[rng.random(n) < 0.05] = 0.0
    feat = rng.normal(size=(n, C)).astype(np.float32)
    feat /= np.linalg.norm(feat, axis=1, keepdims=True).astype(np.float32)
    src = np.empty((n, 3), np.float32)
    tgt = np.empty((n, 3), np.float32)
    dup = rng.choice(n, (min(N_DUP, n // 8), 2), replace=False)

    def draw(rows):
        src[rows] = (rng.random((len(rows), 3)) * scale).astype(np.float32)
        moved = src[rows].astype(np.float64) @ R0.T + t0 + rng.normal(size=(len(rows), 3)) * 0.003 * scale
        free = rng.random((len(rows), 3)) * scale + t0
        tgt[rows] = np.where(inlier[rows, None], moved, free).astype(np.float32)
        for a, b in dup:                      # row b is row a, bit for bit, in every array
            src[b], tgt[b], feat[b], conf[b], inlier[b] = src[a], tgt[a], feat[a], conf[a], inlier[a]
    draw(np.arange(n))
    for _ in range(20):
        bad = np.nonzero(rs.seeds(src, conf, radius, 0)["row_gap"] < GAP)[0]
        if not len(bad):
            break
        draw(bad)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R0, t0
    return dict(n=n, src=src, tgt=tgt, feat=feat, conf=conf, T_gt=T, inlier=inlier, dup=dup)


def perturbed(T, seed, angle=0.02, shift=0.01):
    """T_gt moved by a small rotation and translation: the start of the refinement tests (fp32 [4,4])."""
    rng = np.random.default_rng(seed)
    P = np.eye(4)
    P[:3, :3] = rotation(rng, angle)
    P[:3, 3] = rng.normal(size=3) * shift
    return (P @ T).astype(np.float32)


def seed_count(n, ratio):
    """S as the library computes it: int(double(n) * double(float(ratio)))."""
    return int(float(n) * rs.f32(ratio))
