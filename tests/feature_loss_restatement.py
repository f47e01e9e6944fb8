"""A float64 statement of the validation step's losses (ISSUE "Definition"; the reference: losses.py:64-220, utils/losses/dice.py),
in numpy, written from the definition and not from the reference's code.  tests/test_feature_loss_restatement.py holds it against the
reference's recorded results (tests/golden/floss_*.npz); tests/test_gpu_feature_loss.py holds the HIP kernels against it and the goldens.

Given descriptor maps F_a, F_q [B,C,FH,FW], correspondences (y_a, x_a, y_q, x_q) in image pixels and the flags valid [B]:

  pixels     every coordinate is multiplied by (map size / image size) of its axis as a float32 product, truncated, clamped to its
             axis; then all four columns are clamped to [0, FH - 1]
  unit(v)    v / max(|v|, 1e-8)
  d(u, v)    0.5 (1 - <unit(u), unit(v)>)
  d_pos[n]   d(F_a[:, y_a, x_a], F_q[:, y_q, x_q])
  negative   per side, with p = the side's positive descriptor at pixel (y, x): over the pool positions j (every pixel in row-major order,
             or the listed pixels) the first minimiser of
                 float32(d(p, F[:, pool_j])) + 1e6 max(5 - sqrt(dy^2 + dx^2 + 1e-7), 0)        [the sum and the penalty in float32]
             The penalty is an fp32 quantity by definition; it vanishes for dy^2 + dx^2 >= 25.  A listed position that names no
             pixel (< 0 or >= FH FW) is no candidate; a side without any candidate has d_neg = NaN and pixel 0 on every row
  terms      per pair mean_n max(d_pos - m_pos, 0), mean_n max(m_neg - d_neg, 0) per side (a NaN distance is inside no margin: it
             adds 0, and the backward gives it no gradient); over the batch the mean of each over the valid pairs, 0 without any
  dice       p = 1 / (1 + exp(-2 x)); per image S_p, S_pp, S_pt, S_t;
             loss = 1/4 [mean_b(1 - (S_pt + 1) / (S_pp + S_t + 1)) + mean_b(1 - (S_qu + 1) / (S_qq + S_u + 1))], q = 1 - p, u = 1 - t
"""
import numpy as np

EPS = 1e-8


def feature_pixels(corrs, image_hw, feat_hw):
    """[..., 4] integer image pixels -> feature-map pixels (int64)."""
    c = np.asarray(corrs).astype(np.int64)
    out = np.empty_like(c)
    for col in range(4):
        ax = col % 2
        scaled = c[..., col].astype(np.float32) * np.float32(feat_hw[ax] / image_hw[ax])
        out[..., col] = np.clip(np.trunc(scaled).astype(np.int64), 0, feat_hw[ax] - 1)
    return np.clip(out, 0, feat_hw[0] - 1)


def unit(rows):
    rows = np.asarray(rows, dtype=np.float64)
    return rows / np.maximum(np.sqrt((rows * rows).sum(-1, keepdims=True)), EPS)


def penalty32(py, px, cy, cx, neg_kernel):
    dy = np.float32(py) - cy.astype(np.float32)
    dx = np.float32(px) - cx.astype(np.float32)
    pd = np.sqrt((dy * dy + dx * dx) + np.float32(1e-7), dtype=np.float32)
    return np.float32(1e6) * np.maximum(np.float32(neg_kernel) - pd, np.float32(0.0))


def penalised_costs(fmap, yx, pool, neg_kernel):
    """fmap [C,FH,FW], yx [N,2] feature pixels, pool [P] linear pixels that all name a pixel -> (d [N,P] float64, penalty [N,P] float32)."""
    C, FH, FW = fmap.shape
    rows = unit(fmap.reshape(C, FH * FW).T)
    pos = rows[yx[:, 0] * FW + yx[:, 1]]
    d = 0.5 * (1.0 - pos @ rows[pool].T)
    return d, penalty32(yx[:, 0:1], yx[:, 1:2], (pool // FW)[None], (pool % FW)[None], neg_kernel)


def hardest_negatives(fmap, yx, pool, neg_kernel):
    """fmap [C,FH,FW], yx [N,2] feature pixels, pool [P] linear pixels -> (position in the pool [N], distance [N], pixel [N]).
    A pool position that names no pixel (< 0 or >= FH FW) is no candidate; without any candidate: position -1, distance NaN, pixel 0."""
    HW = fmap.shape[1] * fmap.shape[2]
    pool = np.asarray(pool, dtype=np.int64)
    at = np.flatnonzero((pool >= 0) & (pool < HW))
    if at.size == 0:
        return np.full(len(yx), -1, dtype=np.int64), np.full(len(yx), np.nan), np.zeros(len(yx), dtype=np.int64)
    d, pen = penalised_costs(fmap, yx, pool[at], neg_kernel)
    where = np.argmin(d.astype(np.float32) + pen, axis=1)
    return at[where], d[np.arange(len(yx)), where], pool[at[where]]


def hinge(x):
    """max(x, 0) as the strict test x > 0 states it: a NaN distance (no candidate) is inside no margin and adds 0."""
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, 0.0)


def terms(d_pos, d_neg, valid, pos_margin, neg_margin):
    """d_pos [B,N], d_neg [B,2,N] -> (pair_terms [B,3], losses [3]); the rows of an invalid pair are 0."""
    keep = np.asarray([v == 1 for v in valid])
    pair_terms = np.stack([hinge(d_pos - pos_margin).mean(1), hinge(neg_margin - d_neg[:, 0]).mean(1), hinge(neg_margin - d_neg[:, 1]).mean(1)], axis=1)
    pair_terms[~keep] = 0.0
    return pair_terms, (pair_terms[keep].mean(0) if keep.any() else np.zeros(3))


def restate(feat_a, feat_q, corrs, valid, image_hw, pool=None, pos_margin=0.2, neg_margin=0.9, neg_kernel=5, per_positive=False, pix=None):
    """-> dict(d_pos [B,N], d_neg [B,2,N], neg_idx [B,2,N] linear pixels, pair_terms [B,3], losses (pos, neg_a, neg_q)).
    pool [B,2,P] linear pixels or None (the whole map); per_positive: pool [B,2,N] names every positive's negative directly.
    pix [B,N,4]: the feature pixels themselves, each inside its axis (what the kernels take); corrs and image_hw are then not read."""
    feat = (np.asarray(feat_a, dtype=np.float64), np.asarray(feat_q, dtype=np.float64))
    B, C, FH, FW = feat[0].shape
    pix = feature_pixels(corrs, image_hw, (FH, FW)) if pix is None else np.asarray(pix, dtype=np.int64)
    N = pix.shape[1]
    d_pos, d_neg, neg_idx = np.zeros((B, N)), np.zeros((B, 2, N)), np.zeros((B, 2, N), dtype=np.int64)
    for b in range(B):
        if valid[b] != 1:
            continue
        pa = unit(feat[0][b][:, pix[b, :, 0], pix[b, :, 1]].T)
        pq = unit(feat[1][b][:, pix[b, :, 2], pix[b, :, 3]].T)
        d_pos[b] = 0.5 * (1.0 - (pa * pq).sum(1))
        for side in (0, 1):
            yx = pix[b][:, 2 * side:2 * side + 2]
            if per_positive:
                rows = unit(feat[side][b].reshape(C, FH * FW).T)
                p = (pa, pq)[side]
                neg_idx[b, side] = np.asarray(pool[b, side], dtype=np.int64)
                d_neg[b, side] = 0.5 * (1.0 - (p * rows[neg_idx[b, side]]).sum(1))
            else:
                pl = np.arange(FH * FW) if pool is None else np.asarray(pool[b, side], dtype=np.int64)
                _, d_neg[b, side], neg_idx[b, side] = hardest_negatives(feat[side][b], yx, pl, neg_kernel)
    pair_terms, losses = terms(d_pos, d_neg, valid, pos_margin, neg_margin)
    return dict(pix=pix, d_pos=d_pos, d_neg=d_neg, neg_idx=neg_idx, pair_terms=pair_terms, losses=losses)


def resize_nearest(mask, out_hw):
    """[B,H,W] -> [B,h,w]: source index floor(i * (H / h)) with the ratio in float32, clipped (torch's 'nearest')."""
    B, H, W = mask.shape
    ys = np.minimum(np.floor(np.arange(out_hw[0], dtype=np.float32) * np.float32(H / out_hw[0])).astype(np.int64), H - 1)
    xs = np.minimum(np.floor(np.arange(out_hw[1], dtype=np.float32) * np.float32(W / out_hw[1])).astype(np.int64), W - 1)
    return mask[:, ys][:, :, xs]


def dice_sums(logits, gt):
    """logits [B,H,W], gt [B,H,W] at the same size -> [B,4] float64: S_p, S_pp, S_pt, S_t."""
    x = np.asarray(logits, dtype=np.float64).reshape(len(logits), -1)
    t = (np.asarray(gt).reshape(len(gt), -1) != 0).astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-2.0 * x))
    return np.stack([p.sum(1), (p * p).sum(1), (p * t).sum(1), t.sum(1)], axis=1)


def dice_loss(sums, hw):
    sp, spp, spt, st = (np.asarray(sums, dtype=np.float64)[:, i] for i in range(4))
    fg = 1.0 - (spt + 1.0) / (spp + st + 1.0)
    bg = 1.0 - ((hw - sp - st + spt) + 1.0) / ((hw - 2.0 * sp + spp) + (hw - st) + 1.0)
    return 0.25 * (fg.mean() + bg.mean())


def mask_terms(logits, gt, threshold):
    """logits [B,1,h,w] or [B,h,w], gt [B,H,W] -> (dice loss, mask [B,h,w] from the float32 sigmoid, iou [B])."""
    x = np.asarray(logits, dtype=np.float32)
    x = x[:, 0] if x.ndim == 4 else x
    g = np.asarray(gt)
    if g.shape[1:] != x.shape[1:]:
        g = resize_nearest(g, x.shape[1:])
    mask = (np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))) > np.float32(threshold)
    gb = g != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = (mask & gb).reshape(len(x), -1).sum(1).astype(np.float32) / (mask | gb).reshape(len(x), -1).sum(1).astype(np.float32)
    return dice_loss(dice_sums(x, g), x.shape[1] * x.shape[2]), mask.astype(np.int32), iou
