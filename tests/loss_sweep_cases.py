"""Seeded inputs for the sweep of the loss kernels (tests/test_gpu_loss_sweep.py) and their float64 statements, numpy only.

A case is a dict: feat_a, feat_q [B,C,FH,FW] fp32, pix [B,N,4] int64 feature pixels (y_a, x_a, y_q, x_q; every coordinate inside its own
axis, which is what the kernels take), valid [B] int32, pool ([B,2,P] int64 linear pixels, or None = the whole map), pos_margin and
neg_margin.  Descriptors are white Gaussian noise unless the case says otherwise.  The query map is the anchor map turned by 180 degrees
plus per-pixel noise of a per-pixel scale in [0.3, 2.5]; seven correspondences of eight pair a pixel with its image under that turn, so
their d_pos straddles 0.2 (d_pos = 0.2 at a scale of about 1.3); the eighth has a query pixel of its own draw.

reference(name) adds what the float64 restatement (tests/feature_loss_restatement.py) says of the case, computed once and shared:
d_pos, d_neg, neg_idx; per row the gap between the lowest and the second-lowest float64 penalised cost and the lowest cost itself; and
`runs`, the (pos_margin, neg_margin) pairs the case is run at:
    (0.2, 0.9), (0.2, m)   m = the median of the case's finite d_neg (a case may name its own m, `neg_margin_2`);
    (p, 0.9)               only where every valid row of the case is one row (c255_n1, one_pixel), so that 0.2 cannot have rows on both
                           sides: p = that row's d_pos + 0.1.
tests/test_loss_sweep_cases.py asserts the premises on the CPU."""
import numpy as np

import feature_loss_restatement as fr

NEAR_TIE = 1e-5                # tools/gen_goldens.py floss: the smallest top-2 gap a recorded fixture may have
NEAR_TIE_CAP = 0.01            # at most this share of a case's rows may be near-tied
SCATTER_BLOCK = 256            # slots per block of feature_loss_grad_scatter_kernel


def noise_maps(rng, B, C, FH, FW):
    feat_a = rng.standard_normal((B, C, FH, FW))
    scale = rng.uniform(0.3, 2.5, (B, 1, FH, FW))
    feat_q = feat_a[:, :, ::-1, ::-1] + scale * rng.standard_normal((B, C, FH, FW))
    return feat_a.astype(np.float32), np.ascontiguousarray(feat_q).astype(np.float32)


def noise_pix(rng, B, N, FH, FW):
    ya, xa = rng.integers(0, FH, (B, N)), rng.integers(0, FW, (B, N))
    yq, xq = FH - 1 - ya, FW - 1 - xa
    own = np.arange(N)[None] % 8 == 7
    yq, xq = np.where(own, rng.integers(0, FH, (B, N)), yq), np.where(own, rng.integers(0, FW, (B, N)), xq)
    return np.stack([ya, xa, yq, xq], axis=-1).astype(np.int64)


def make_case(name, feat, pix, valid=None, pool=None, **extra):
    B = len(pix)
    valid = np.ones(B, np.int32) if valid is None else np.asarray(valid, np.int32)
    return dict(name=name, feat_a=feat[0], feat_q=feat[1], pix=pix, valid=valid, pool=pool, pos_margin=0.2, neg_margin=0.9, **extra)


def _noise(name, seed, B, C, FH, FW, N):
    rng = np.random.default_rng(seed)
    return make_case(name, noise_maps(rng, B, C, FH, FW), noise_pix(rng, B, N, FH, FW))


def c3_ragged():
    return _noise("c3_ragged", 103, 2, 3, 13, 17, 65)


def c5_wide():
    return _noise("c5_wide", 105, 1, 5, 12, 31, 64)


def c97():
    return _noise("c97", 197, 2, 97, 20, 20, 129)


def c255_n1():
    return _noise("c255_n1", 255, 1, 255, 12, 12, 1)


def c1():
    """One channel: every unit row is exactly +-1, every cost the same number in fp32 and in float64, and nearly every row a tie of a
    hundred candidates.  The anchor map is positive except the 2 x 2 block at (7..8, 7..8), where four positives sit: every pixel of
    their own sign lies inside their exclusion disc, so their negative has d_neg = 1 and all the others' has d_neg = 0."""
    rng = np.random.default_rng(101)
    feat_a, feat_q = noise_maps(rng, 1, 1, 16, 16)
    feat_a = np.abs(feat_a) + np.float32(0.01)
    feat_a[0, 0, 7:9, 7:9] *= -1
    pix = noise_pix(rng, 1, 64, 16, 16)
    pix[0, :4, 0], pix[0, :4, 1] = (7, 7, 8, 8), (7, 8, 7, 8)
    return make_case("c1", (feat_a, feat_q), pix, neg_margin_2=0.5)


def pool_table():
    """HW = 2025, a table of 130 positions per (pair, side): 118 distinct pixels and, at positions 0, 5, 63, 64, 70 and 123 .. 129 (both
    ends of the first 64-position tile, both ends of the second, the whole of the third), the entries -1, HW and 1 << 30, which name no
    pixel.  The table of (pair 1, side 1) names none at all."""
    rng = np.random.default_rng(2025)
    B, FH, FW, P = 2, 45, 45, 130
    feat = noise_maps(rng, B, 32, FH, FW)
    bad = np.array([0, 5, 63, 64, 70, 123, 124, 125, 126, 127, 128, 129])
    none = np.array([-1, FH * FW, 1 << 30], dtype=np.int64)
    pool = np.empty((B, 2, P), dtype=np.int64)
    for b in range(B):
        for side in (0, 1):
            pool[b, side] = rng.permutation(FH * FW)[:P]
            pool[b, side, bad] = none[np.arange(len(bad)) % 3]
    pool[1, 1] = none[rng.integers(0, 3, P)]
    return make_case("pool_table", feat, noise_pix(rng, B, 63, FH, FW), pool=pool, empty=(1, 1))


def n4096():
    return _noise("n4096", 4096, 1, 32, 40, 40, 4096)


def one_pixel():
    rng = np.random.default_rng(300)
    feat = noise_maps(rng, 1, 16, 24, 24)
    pix = np.tile(np.array([[[5, 17, 18, 6]]], dtype=np.int64), (1, 300, 1))
    feat[1][0, :, 18, 6] = feat[0][0, :, 5, 17] + np.float32(1.5) * rng.standard_normal(16).astype(np.float32)
    return make_case("one_pixel", feat, pix)


def b130():
    rng = np.random.default_rng(130)
    valid = (rng.random(130) < 0.75).astype(np.int32)
    valid[[0, 63, 64, 65, 129]] = 0
    valid[[1, 62, 66, 128]] = 1
    return make_case("b130", noise_maps(rng, 130, 4, 12, 12), noise_pix(rng, 130, 8, 12, 12), valid=valid)


def _gauss(x, sigma):
    r = int(4 * sigma)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for ax in (-2, -1):
        pad = [(0, 0)] * x.ndim
        pad[ax] = (r, r)
        x = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), ax, np.pad(x, pad, mode="reflect"))
    return x


def smooth():
    """Maps filtered with a Gaussian of sigma 2 (and scaled back to unit variance): neighbouring pixels are nearly parallel, so the
    hardest-negative search has near-ties.  The query is the turned anchor plus filtered noise, scaled 0.3 .. 2.5 from left to right."""
    rng = np.random.default_rng(22)
    B, C, FH, FW = 1, 16, 24, 24
    a, e = _gauss(rng.standard_normal((B, C, FH, FW)), 2.0), _gauss(rng.standard_normal((B, C, FH, FW)), 2.0)
    a, e = a / a.std(), e / e.std()
    q = a[:, :, ::-1, ::-1] + np.linspace(0.3, 2.5, FW)[None, None, None, :] * e
    return make_case("smooth", (a.astype(np.float32), np.ascontiguousarray(q).astype(np.float32)), noise_pix(rng, B, 300, FH, FW))


CASES = {f.__name__: f for f in (c3_ragged, c5_wide, c97, c255_n1, c1, pool_table, n4096, one_pixel, b130, smooth)}
TIE_EXEMPT = ("c1",)
_cache = {}


def candidates(case, b, side):
    """The pool positions of (pair, side) that name a pixel, as linear pixels in pool order."""
    HW = case["feat_a"].shape[2] * case["feat_a"].shape[3]
    if case["pool"] is None:
        return np.arange(HW)
    pl = case["pool"][b, side]
    return pl[(pl >= 0) & (pl < HW)]


def costs64(case, b, side, rows=None):
    """-> float64 penalised costs [rows, candidates] of (pair, side): float64 distance + the penalty (an fp32 quantity by definition)."""
    fmap = (case["feat_a"], case["feat_q"])[side][b].astype(np.float64)
    yx = case["pix"][b][:, 2 * side:2 * side + 2]
    d, pen = fr.penalised_costs(fmap, yx if rows is None else yx[rows], candidates(case, b, side), 5)
    return d + pen.astype(np.float64)


def restated(case):
    """-> r = fr.restate's dict of a case at its margins plus gap [B,2,N] (inf where there is no second candidate, NaN for an invalid pair
    or a table without candidates), low [B,2,N] and runs."""
    r = fr.restate(case["feat_a"], case["feat_q"], None, case["valid"], None, case["pool"], case["pos_margin"], case["neg_margin"], pix=case["pix"])
    B, N = case["pix"].shape[:2]
    gap, low = np.full((B, 2, N), np.nan), np.full((B, 2, N), np.nan)
    for b in range(B):
        for side in (0, 1):
            if case["valid"][b] != 1 or candidates(case, b, side).size == 0:
                continue
            c = costs64(case, b, side)
            two = np.partition(c, 1, axis=1)[:, :2] if c.shape[1] > 1 else np.concatenate([c, np.full_like(c, np.inf)], axis=1)
            gap[b, side], low[b, side] = two[:, 1] - two[:, 0], two[:, 0]
    keep = case["valid"] == 1
    runs = [(case["pos_margin"], case["neg_margin"])]
    if keep.any():
        runs.append((case["pos_margin"], case.get("neg_margin_2", float(np.nanmedian(r["d_neg"][keep])))))
        if len(np.unique(case["pix"][keep].reshape(-1, 4), axis=0)) == 1:
            runs.append((float(r["d_pos"][keep].max()) + 0.1, case["neg_margin"]))
    r.update(gap=gap, low=low, runs=runs)
    return r


def reference(name):
    """-> (case, restated(case)), computed once, shared, never modified."""
    if name not in _cache:
        case = CASES[name]()
        _cache[name] = (case, restated(case))
    return _cache[name]


def at_pixel(case, b, side, n, pixel):
    """-> (float64 penalised cost, float64 distance) of row n of (pair, side) at the candidate `pixel`."""
    fmap = (case["feat_a"], case["feat_q"])[side][b].astype(np.float64)
    d, pen = fr.penalised_costs(fmap, case["pix"][b][n:n + 1, 2 * side:2 * side + 2], np.array([pixel], dtype=np.int64), 5)
    return float(d[0, 0]) + float(pen[0, 0]), float(d[0, 0])


def slot_keys(case, neg_idx, b, side):
    """The 2 N pixel keys of (pair, side) in the scatter kernel's slot order: the positives' pixels, then the negatives' (-1: no pixel)."""
    FH, FW = case["feat_a"].shape[2:]
    pos = case["pix"][b, :, 2 * side] * FW + case["pix"][b, :, 2 * side + 1]
    neg = np.asarray(neg_idx[b, side], dtype=np.int64)
    return np.concatenate([pos, np.where((neg >= 0) & (neg < FH * FW), neg, -1)])


def slots_per_pixel(case, neg_idx):
    """-> [2,B,FH,FW] int: the number of slots of a valid pair on every pixel (K of the backward's bar)."""
    B, _, FH, FW = case["feat_a"].shape
    K = np.zeros((2, B, FH * FW), dtype=np.int64)
    for b in range(B):
        if case["valid"][b] == 1:
            for side in (0, 1):
                keys = slot_keys(case, neg_idx, b, side)
                K[side, b] = np.bincount(keys[keys >= 0], minlength=FH * FW)
    return K.reshape(2, B, FH, FW)


def dice_case(H, W):
    """-> (logits [3,H,W] fp32, gt [3,H,W] int32).  Logits 3 * randn with +-40 and +-200 planted at both ends of every image (exp(400)
    overflows: p is exactly 0 at -200) and no logit within 1e-3 of 0, so that no sigmoid lies within 1e-6 of the threshold 0.5, where
    expf and numpy's float32 exp may differ in the last bit.  Ground truth: image 0 all background, image 1 all object (1, 2 and 255:
    anything non-zero), image 2 random."""
    rng = np.random.default_rng(1000 * H + W)
    x = (3.0 * rng.standard_normal((3, H * W))).astype(np.float32)
    x = np.where(np.abs(x) < 1e-3, np.float32(1e-3) * np.where(x < 0, -1, 1), x).astype(np.float32)
    plant = np.array([-200.0, 40.0, -40.0, 200.0], dtype=np.float32)
    if H * W >= 8:
        x[:, :4], x[:, -4:] = plant, plant[::-1]
    else:
        x[:, 0] = plant[:3]
    gt = np.zeros((3, H * W), dtype=np.int32)
    gt[1] = np.array([1, 2, 255])[rng.integers(0, 3, H * W)]
    gt[2] = rng.integers(0, 2, H * W)
    return x.reshape(3, H, W), gt.reshape(3, H, W)


DICE_SIZES = ((1, 1), (1, 513), (97, 131), (192, 192))
