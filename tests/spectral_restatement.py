"""Float64 restatement of the spectral pose solver (helper of test_spectral_restatement.py and test_gpu_spectral.py; not a test
module): the definition in the header of oryon_amd/csrc/spectral.hip, stage by stage, in numpy, with no tricks, returning every
intermediate.  Scalars the library holds in fp32 (thresholds, sigma, radius, ratio) are widened from fp32, as pdsc_restatement.f32
does.  The seeds, the weighted Kabsch and the residuals are pdsc_restatement's (the kernels are PointDSC's, unchanged)."""
import numpy as np

import pdsc_restatement as pr
from pdsc_restatement import NEAR, f32

DEFAULTS = dict(num_iterations=10, ratio=0.1, inlier_threshold=0.01, sigma_d=0.01, k=40, nms_radius=0.02)


# ------------------------------------------------------------------------------------------ inputs of the planted-pose cases
def planted(n, outlier_fraction, seed, cube=0.3, noise=0.001):
    """Uniform points in a cube of side `cube` (metres), a random rigid motion, Gaussian noise on the target, a random subset of rows
    (each with probability outlier_fraction) replaced by uniform random target points -> src, tgt fp32 [n,3], T [4,4], outlier mask."""
    r = np.random.default_rng(seed)
    src = r.uniform(-cube / 2, cube / 2, (n, 3))
    Q, _ = np.linalg.qr(r.normal(size=(3, 3)))
    Q *= np.sign(np.linalg.det(Q))
    t = r.uniform(-0.2, 0.2, 3)
    tgt = src @ Q.T + t + r.normal(scale=noise, size=(n, 3))
    o = r.random(n) < outlier_fraction
    tgt[o] = r.uniform(-cube / 2, cube / 2, (int(o.sum()), 3)) + t
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Q, t
    return src.astype(np.float32), tgt.astype(np.float32), T, o


def pose_error(T, G):
    """-> (rotation error in degrees, translation error in metres) of T against G."""
    R = T[:3, :3] @ G[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))), float(np.linalg.norm(T[:3, 3] - G[:3, 3]))


# ------------------------------------------------------------------------------------------ S1
def _lengths(p):
    """|p_i - p_j| as sqrt((dx dx + dy dy) + dz dz), every operation rounded once in p's dtype."""
    d = p[:, None, :] - p[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def compat(src, tgt, inlier_threshold):
    """C [n,n] bool: | |s_i - s_j| - |t_i - t_j| | < tau in float64, zero diagonal; gap = the smallest distance of an off-diagonal
    entry from the threshold (0 would be a tie; float64 leaves none in practice)."""
    s, t = np.asarray(src, np.float32).astype(np.float64), np.asarray(tgt, np.float32).astype(np.float64)
    diff = np.abs(_lengths(s) - _lengths(t))
    C = diff < f32(inlier_threshold)
    np.fill_diagonal(C, False)
    return C, diff


def pack_bits(C, n_cap):
    """[n,n] bool -> [n_cap, n_cap/32] uint32: bit j & 31 of word j >> 5 of row i; rows and columns >= n are 0."""
    full = np.zeros((n_cap, n_cap), bool)
    n = C.shape[0]
    full[:n, :n] = C
    return np.packbits(full, axis=1, bitorder="little").view("<u4").astype(np.uint32)


# ------------------------------------------------------------------------------------------ S2 / S5
def spatial_matrix(src, tgt, sigma_d, dtype=np.float64):
    """M_ij = max(0, 1 - (|s_i - s_j| - |t_i - t_j|)^2 / sigma_d^2), M_ii = 0, evaluated in `dtype` on the fp32 inputs."""
    s, t = np.asarray(src, np.float32).astype(dtype), np.asarray(tgt, np.float32).astype(dtype)
    d = _lengths(s) - _lengths(t)
    sig = dtype(np.float32(sigma_d))
    M = np.maximum(dtype(0), dtype(1) - d * d / (sig * sig))
    np.fill_diagonal(M, 0)
    return M


def confidence(src, tgt, sigma_d, num_iterations, dtype=np.float64):
    """v = 1; num_iterations times u = M v, v = u / (|u|_2 + 1e-6); no early exit -> v [n] in `dtype`."""
    M = spatial_matrix(src, tgt, sigma_d, dtype)
    v = np.ones(M.shape[0], dtype)
    for _ in range(num_iterations):
        u = M @ v
        v = u / (np.sqrt((u * u).sum(dtype=dtype)) + dtype(1e-6))
    return v


# ------------------------------------------------------------------------------------------ S4
def scores(C, seeds):
    """[S,n] int64: score_sj = C_sj (C C)_sj = C_sj popcount(row_s & row_j)."""
    Ci = np.asarray(C).astype(np.int64)
    seeds = np.asarray(seeds, np.int64)
    return Ci[seeds] * (Ci[seeds] @ Ci)


def consensus_sets(C, seeds, k):
    """-> sets [S,k'] int64 (the seed first, then the k' - 1 rows j != seed of the highest score, ties by ascending j), k' = min(k, n - 1),
    ties [S] bool: whether the last row taken and the first row left out have the same score (the tie rule decided)."""
    n = C.shape[0]
    kk = min(k, n - 1)
    sc = scores(C, seeds)
    sets, ties = [], []
    for s, row in zip(np.asarray(seeds, np.int64), sc):
        row = row.copy()
        row[s] = -1
        order = np.argsort(-row, kind="stable")
        sets.append(np.concatenate([[s], order[:max(kk - 1, 0)]])[:max(kk, 0)])
        ties.append(bool(kk >= 2 and kk - 1 < n - 1 and row[order[kk - 2]] == row[order[kk - 1]]))
    return np.array(sets, np.int64).reshape(len(sets), max(kk, 0)), np.array(ties, bool)


# ------------------------------------------------------------------------------------------ S5 - S8
def tail(sets, src, tgt, sigma_d, num_iterations, inlier_threshold, stop=None):
    """From the consensus sets: the local matrices, the per-seed power iteration with PointDSC's JOINT allclose exit (stop = None;
    else exactly iteration index `stop` is used, as a device that stopped there did), weights, weighted Kabsch, fitness, first argmax."""
    s64, t64 = np.asarray(src, np.float32).astype(np.float64), np.asarray(tgt, np.float32).astype(np.float64)
    sets = np.asarray(sets, np.int64)
    S, kk = sets.shape
    M = np.stack([spatial_matrix(s64[idx].astype(np.float32), t64[idx].astype(np.float32), sigma_d) for idx in sets]) if S else np.zeros((0, kk, kk))
    v = np.ones((S, kk, 1))
    last, margins, used = v, [], num_iterations - 1
    for it in range(num_iterations):
        v = M @ v
        v = v / (np.sqrt((v ** 2).sum(1, keepdims=True)) + 1e-6)
        margins.append(float((np.abs(v - last) - (1e-8 + 1e-5 * np.abs(last))).max()) if v.size else 0.0)
        if (stop is None and margins[-1] <= 0) or (stop is not None and it == stop):
            used = it
            break
        last = v
    w = v[:, :, 0]
    w = w / (w.sum(1, keepdims=True) + 1e-6)
    T = pr.kabsch(s64[sets], t64[sets], w)
    thr = f32(inlier_threshold)
    L2 = pr.residuals(T, s64, t64)
    fitness = (L2 < thr).mean(1)
    return dict(M=M, weights=w, T=T, fitness=fitness, best=int(np.argmax(fitness)) if S else -1, margins=margins, stop=used,
                near=(np.abs(L2 - thr) < NEAR).sum(1))


# ------------------------------------------------------------------------------------------ S9
def refine(T, src, tgt, tau, max_iter=20):
    """PointDSC's post_refinement (pdsc_restatement.refine) with tau given: re-fit on the rows inside tau with weights
    1 / (1 + (d / tau)^2) until the inlier count repeats."""
    T = np.asarray(T, np.float64)
    s, t = np.asarray(src, np.float32).astype(np.float64), np.asarray(tgt, np.float32).astype(np.float64)
    tau = f32(tau)
    prev, its = 0, 0
    for _ in range(max_iter):
        L2 = pr.residuals(T[None], s, t)[0]
        inl = L2 < tau
        cnt = int(inl.sum())
        if abs(cnt - prev) < 1:
            break
        prev = cnt
        its += 1
        T = pr.kabsch(s[inl][None], t[inl][None], (1 / (1 + (L2 / tau) ** 2))[inl][None])[0]
    return dict(T=T, iterations=its, inliers=prev)


def register(src, tgt, **cfg):
    """The whole solver out of the stages above -> every intermediate; T is the identity and status 2 (ORYON_PAIR_NO_CORR) without a seed."""
    c = dict(DEFAULTS, **cfg)
    n = np.asarray(src).shape[0]
    S = int(n * f32(c["ratio"]))
    out = dict(n_seeds=S, status=0)
    if n < 2 or S <= 0:
        out.update(T=np.eye(4), status=2)
        return out
    C, diff = compat(src, tgt, c["inlier_threshold"])
    conf = confidence(src, tgt, c["sigma_d"], c["num_iterations"])
    sd = pr.seeds(src, conf, c["nms_radius"], S)
    sets, ties = consensus_sets(C, sd["seeds"], c["k"])
    tl = tail(sets, src, tgt, c["sigma_d"], c["num_iterations"], c["inlier_threshold"])
    ref = refine(tl["T"][tl["best"]], src, tgt, c["inlier_threshold"])
    out.update(C=C, conf=conf, seeds=sd["seeds"], seed_info=sd, sets=sets, ties=ties, tail=tl, T0=tl["T"][tl["best"]], refine=ref, T=ref["T"])
    return out
