"""Float64 restatement of the PointDSC solver stages (helper of test_pdsc_restatement.py and test_gpu_pointdsc_sizes.py; not a test
module).

Every function takes the fp32 arrays the kernels get, widens them to float64 and evaluates the operation as the reference states it
(models/pointdsc/PointDSC.py, restated in fp32 by oracle/oryon_oracle.py), with no tricks.  Beside the result each returns the MARGINS of
its own discrete decisions - how far the nearest input is from flipping an NMS verdict, a neighbour list, the early exit of the power
iteration or an inlier test - so that a test can tell "the kernel decided differently" from "the inputs sit on a decision boundary".
Scalars that the library holds in fp32 (radius, sigma, thresholds) are widened from fp32 too."""
import numpy as np
import torch

NEAR = 1e-5           # a distance closer than this to a threshold may be classified either way by an fp32 evaluation


def f32(x):
    """The float64 value of x rounded to fp32 (what the library's config struct holds)."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------ seeds (PointDSC.py:199-217)
def seeds(src, conf, radius, S, chunk=512):
    """key_i = conf_i * [for all j: conf_i >= conf_j or d_ij >= R]; order = stable descending order of key; seeds = order[:S].
    gap = min |d_ij - R| over the pairs with conf_i < conf_j (the only pairs whose distance test decides anything).  Rows are
    processed `chunk` at a time: the [chunk, n, 3] difference block is the largest array (50 MB at n = 4096)."""
    src = np.asarray(src, np.float64)
    conf = np.asarray(conf, np.float64)
    n, R = src.shape[0], f32(radius)
    lm = np.ones(n, bool)
    row_gap = np.full(n, np.inf)
    for s in range(0, n, chunk):
        d = np.sqrt(((src[s:s + chunk, None, :] - src[None, :, :]) ** 2).sum(-1))
        ge = conf[s:s + chunk, None] >= conf[None, :]
        lm[s:s + chunk] = (ge | (d >= R)).all(1)
        less = conf[s:s + chunk, None] < conf[None, :]
        row_gap[s:s + chunk] = np.where(less, np.abs(d - R), np.inf).min(1)
    key = conf * lm
    order = np.argsort(-key, kind="stable")
    return dict(key=key, local_max=lm, order=order, seeds=order[:S], gap=float(row_gap.min()), row_gap=row_gap)


# ------------------------------------------------------------------------------------------ weighted Kabsch (common.py:7-45)
def kabsch(A, B, w):
    """[S,m,3] x2, [S,m] -> [S,4,4]: negative weights clipped, centroids over sum(w) + 1e-6, R = V diag(1, 1, det(V U^T)) U^T."""
    w = np.where(w < 0, 0.0, w)
    den = w.sum(1)[:, None, None] + 1e-6
    ca = (A * w[:, :, None]).sum(1, keepdims=True) / den
    cb = (B * w[:, :, None]).sum(1, keepdims=True) / den
    H = np.swapaxes(A - ca, 1, 2) @ (w[:, :, None] * (B - cb))
    U, _, Vt = np.linalg.svd(H)
    V = np.swapaxes(Vt, 1, 2)
    D = np.tile(np.eye(3), (A.shape[0], 1, 1))
    D[:, 2, 2] = np.linalg.det(V @ np.swapaxes(U, 1, 2))
    R = V @ D @ np.swapaxes(U, 1, 2)
    T = np.tile(np.eye(4), (A.shape[0], 1, 1))
    T[:, :3, :3] = R
    T[:, :3, 3] = cb[:, 0] - np.einsum("sij,sj->si", R, ca[:, 0])
    return T


def residuals(T, src, tgt):
    """[S,4,4] x [n,3] x [n,3] -> [S,n] distances |R src + t - tgt|."""
    pred = np.einsum("sij,nj->sni", T[:, :3, :3], src) + T[:, None, :3, 3]
    return np.sqrt(((pred - tgt[None]) ** 2).sum(-1))


# ------------------------------------------------------------------------------------------ hypotheses (PointDSC.py:234-358)
def hypotheses(seeds, feat, src, tgt, sigma, sigma_d, k, num_iterations, inlier_threshold):
    """oracle.seed_hypotheses step by step on the UN-normalised features the stage entry gets.  Per seed: knn [S,k], T [S,4,4],
    fitness, kgap (smallest of distance(rank k + 1) - distance(rank k) and distance(rank 1) - distance(rank 0); an exactly zero
    difference between bit-identical feature rows is a tie resolved by index, not a gap, and counts as infinite), near (rows whose
    residual is within NEAR of the threshold).  Per power iterate: margin = max(|v - last| - (1e-8 + 1e-5 |last|)) over all seeds
    and entries; the joint allclose test is `margin <= 0`."""
    seeds = np.asarray(seeds, np.int64)
    f_in = np.asarray(feat)
    feat = f_in.astype(np.float64)
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    n = feat.shape[0]
    k = min(k, n - 1)
    fn = feat / np.maximum(np.sqrt((feat ** 2).sum(1, keepdims=True)), 1e-12)          # F.normalize
    d = 2.0 - 2.0 * (fn[seeds] @ fn.T)
    order = np.argsort(d, axis=1, kind="stable")
    ds = np.take_along_axis(d, order, 1)
    idx = order[:, 1:k + 1]

    def gap(lo, hi):
        g = ds[:, hi] - ds[:, lo]
        same = (f_in[order[:, lo]] == f_in[order[:, hi]]).all(1)
        return np.where((g == 0) & same, np.inf, g)
    kgap = gap(0, 1)
    if k + 1 < n:
        kgap = np.minimum(kgap, gap(k, k + 1))
    sig2, sigd2 = f32(sigma) ** 2, f32(sigma_d) ** 2
    fk = fn[idx]
    fM = np.clip(1 - (1 - fk @ np.swapaxes(fk, 1, 2)) / sig2, 0, None)
    sk, tk = src[idx], tgt[idx]
    dS = np.sqrt(((sk[:, :, None, :] - sk[:, None, :, :]) ** 2).sum(-1))
    dT = np.sqrt(((tk[:, :, None, :] - tk[:, None, :, :]) ** 2).sum(-1))
    M = fM * np.clip(1 - (dS - dT) ** 2 / sigd2, 0, None)
    ar = np.arange(k)
    M[:, ar, ar] = 0
    v = np.ones((len(seeds), k, 1))
    last, margins = v, []
    for _ in range(num_iterations):
        v = M @ v
        v = v / (np.sqrt((v ** 2).sum(1, keepdims=True)) + 1e-6)
        margins.append(float((np.abs(v - last) - (1e-8 + 1e-5 * np.abs(last))).max()))
        if margins[-1] <= 0:
            break
        last = v
    w = v[:, :, 0]
    w = w / (w.sum(1, keepdims=True) + 1e-6)
    T = kabsch(sk, tk, w)
    thr = f32(inlier_threshold)
    L2 = residuals(T, src, tgt)
    fitness = (L2 < thr).mean(1)
    return dict(knn=idx, kgap=kgap, M=M, weights=w, T=T, fitness=fitness, best=int(np.argmax(fitness)), margins=margins,
                near=(np.abs(L2 - thr) < NEAR).sum(1))


# ------------------------------------------------------------------------------------------ refinement (PointDSC.py:403-438)
def refine(T, src, tgt, inlier_threshold, max_iter=20):
    """oracle.post_refinement: tau = 0.10 when the inlier threshold is 0.10 (as fp32), 1.2 otherwise; re-fit on the rows inside tau
    with weights 1 / (1 + (d / tau)^2) until the inlier count repeats.  near = the largest number of rows within NEAR of tau at any
    iterate; min_inliers = the smallest number of rows any re-fit was made from (below 3 the rotation is not determined)."""
    T = np.asarray(T, np.float64)
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    tau = f32(0.10) if np.float32(inlier_threshold) == np.float32(0.10) else f32(1.2)
    prev, near, its, fewest = 0, 0, 0, src.shape[0]
    for _ in range(max_iter):
        L2 = residuals(T[None], src, tgt)[0]
        near = max(near, int((np.abs(L2 - tau) < NEAR).sum()))
        inl = L2 < tau
        cnt = int(inl.sum())
        if abs(cnt - prev) < 1:
            break
        prev = cnt
        its += 1
        fewest = min(fewest, cnt)
        w = 1 / (1 + (L2 / tau) ** 2)
        T = kabsch(src[inl][None], tgt[inl][None], w[inl][None])[0]
    return dict(T=T, near=near, iterations=its, tau=tau, min_inliers=fewest)


# ------------------------------------------------------------------------------------------ encoder (PointDSC.py:27-77, 107-113)
def encoder(src, tgt, P, L):
    """oracle.encoder_forward + confidence_head on .double() parameters -> (feat [n,C], conf [n]) as float64 numpy."""
    from oracle import oryon_oracle as orc
    Pd = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in P.items()}
    s, t = torch.as_tensor(np.asarray(src)).double(), torch.as_tensor(np.asarray(tgt)).double()
    cp = torch.cat([s, t], dim=-1)
    cp = cp - cp.mean(0)
    SC, _ = orc.sc_matrix(s, t, float(P["sigma_spat"][0]))
    feat = orc.encoder_forward(cp, SC, Pd, L)
    return feat.numpy(), orc.confidence_head(feat, Pd).numpy()


def register(src, tgt, P, cfg):
    """The whole pipeline (oracle.pointdsc_forward) out of the float64 stages above."""
    n = np.asarray(src).shape[0]
    feat, conf = encoder(src, tgt, P, cfg["num_layers"])
    sd = seeds(src, conf, cfg["nms_radius"], int(n * f32(cfg["ratio"])))
    hyp = hypotheses(sd["seeds"], feat, src, tgt, float(P["sigma"][0]), float(P["sigma_spat"][0]), cfg["k"], cfg["num_iterations"],
                     cfg["inlier_threshold"])
    ref = refine(hyp["T"][hyp["best"]], src, tgt, cfg["inlier_threshold"])
    return dict(feat=feat, conf=conf, seeds=sd, hyp=hyp, refine=ref, T=ref["T"])
