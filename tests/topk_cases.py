"""The planted-decoy pairs of the one-to-many matcher's tests: the case topk exists for.

synth.make_pair(index, 48, 48, 32), and for every anchor pixel inside mask_a that has a true query pixel (the generator's own `winner`
table) ONE other query pixel overwritten with an exact copy of the anchor's descriptor.  That pixel is taken from the query pixels owned
by anchor pixels OUTSIDE mask_a (so no anchor under test loses its true pixel), at least DECOY_MIN_PX from the true pixel, each used
once: the first free one in a permutation seeded by the index.  The nearest query descriptor of such an anchor is then the decoy (distance
~0), the nearest one outside a 5-pixel disc round it the true pixel (the generator's 0.05 N(0,1) noise away), and everything else is a
random descriptor.  conditions() states that in float64; the tests assert it before anything runs on a device."""
import numpy as np
import torch

PAIRS = (40, 41, 42, 43)
H = W = 48
C = 32
RADIUS = 5
DECOY_MIN_PX = 7
PLANTED = {40: 498, 41: 537, 42: 524, 43: 576}          # anchors with a true pixel and a decoy, out of 576

_cache = {}


def planted_pair(index):
    """-> dict: make_pair's entries with feat_q planted, `plain_feat_q` (untouched), `winner` [HW] int64 (-1: none), and the planted
    anchors' `anchor_px`, `true_px`, `decoy_px` [n] int64 linear pixel indices."""
    if index in _cache:
        return _cache[index]
    from oryon_amd import synth
    p = synth.make_pair(index, H, W, C)
    winner = synth._pair_geometry(index, H, W)[5].numpy()
    in_mask = p["mask_a"].reshape(-1).numpy() == 1
    q_px = np.nonzero(winner >= 0)[0]
    owner_in = in_mask[winner[q_px]]
    true_px, anchor_px = q_px[owner_in], winner[q_px[owner_in]]
    order = np.argsort(anchor_px)
    true_px, anchor_px = true_px[order], anchor_px[order]
    assert len(np.unique(anchor_px)) == len(anchor_px)                   # one true pixel per anchor
    pool = q_px[~owner_in]
    pool = pool[np.random.default_rng(5000 + index).permutation(len(pool))]
    free = np.ones(len(pool), dtype=bool)
    py, px = pool // W, pool % W
    decoy_px = np.full(len(anchor_px), -1, dtype=np.int64)
    for k, t in enumerate(true_px):
        ok = free & ((py - t // W) ** 2 + (px - t % W) ** 2 >= DECOY_MIN_PX ** 2)
        if ok.any():
            j = int(np.argmax(ok))
            decoy_px[k], free[j] = pool[j], False
    have = decoy_px >= 0
    anchor_px, true_px, decoy_px = anchor_px[have], true_px[have], decoy_px[have]
    fa = p["feat_a"].reshape(C, H * W)
    fq = p["feat_q"].reshape(C, H * W).clone()
    fq[:, torch.from_numpy(decoy_px)] = fa[:, torch.from_numpy(anchor_px)]
    out = dict(p, plain_feat_q=p["feat_q"], feat_q=fq.reshape(C, H, W), winner=winner, anchor_px=anchor_px, true_px=true_px,
               decoy_px=decoy_px)
    _cache[index] = out
    return out


def is_true_row(winner, rows):
    """rows [n,4] (y_a, x_a, y_q, x_q) -> bool [n]: the generator's winner of the query pixel is the anchor pixel"""
    rows = np.asarray(rows).astype(np.int64)
    return winner[rows[:, 2] * W + rows[:, 3]] == rows[:, 0] * W + rows[:, 1]


def conditions(index, ranks):
    """The float64 facts of one planted pair, asserted: rank 1 = decoy, rank 2 outside a RADIUS disc = true pixel, the gaps, and no
    rank-1 row a true correspondence.  ranks: topk_restatement.ranks.  -> dict of the measured figures."""
    p = planted_pair(index)
    roi_q = np.nonzero(p["mask_q"].reshape(-1).numpy() == 1)[0]
    row_of = {int(px): j for j, px in enumerate(roi_q)}
    a = p["feat_a"].reshape(C, H * W).numpy().astype(np.float64)[:, p["anchor_px"]].T
    q = p["feat_q"].reshape(C, H * W).numpy().astype(np.float64)[:, roi_q].T
    an, qn = a / np.linalg.norm(a, axis=1, keepdims=True), q / np.linalg.norm(q, axis=1, keepdims=True)
    dist = 0.5 * (1.0 - an @ qn.T)
    cd, ca = ranks(dist, roi_q, W, RADIUS, 3)
    n = len(p["anchor_px"])
    assert n == PLANTED[index], (index, n)
    decoy_row = np.array([row_of[int(x)] for x in p["decoy_px"]])
    true_row = np.array([row_of[int(x)] for x in p["true_px"]])
    assert np.array_equal(ca[0], decoy_row), f"pair {index}: rank 1 is not the decoy everywhere"
    assert np.array_equal(ca[1], true_row), f"pair {index}: rank 2 is not the true pixel everywhere"
    assert cd[0].max() <= 1e-12
    assert (cd[1] - cd[0]).min() >= 1e-4 and cd[1].max() <= 5e-3, (cd[1].min(), cd[1].max())
    assert (cd[2] - cd[1]).min() >= 0.05, (cd[2] - cd[1]).min()
    rows1 = np.stack([p["anchor_px"] // W, p["anchor_px"] % W, roi_q[ca[0]] // W, roi_q[ca[0]] % W], axis=1)
    assert not is_true_row(p["winner"], rows1).any(), f"pair {index}: a rank-1 row is a true correspondence"
    rows2 = np.stack([p["anchor_px"] // W, p["anchor_px"] % W, roi_q[ca[1]] // W, roi_q[ca[1]] % W], axis=1)
    assert is_true_row(p["winner"], rows2).all()
    return dict(n=n, d1_max=float(cd[0].max()), d2_min=float(cd[1].min()), d2_max=float(cd[1].max()), d3_min=float(cd[2].min()))
