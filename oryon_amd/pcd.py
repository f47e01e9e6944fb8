"""Drop-in counterparts of the reference's utils/pcd.py entry points on the hot path.

    nn_correspondences(feats1, feats2, mask1, mask2, threshold, max_corrs, subsample_source, corrs_device)
    lift_pcd(depth, camera, xy_idxs)
    torch_sample_select(t, n)

Same names, argument meaning, return types and failure behaviour as utils/pcd.py:177-216, :35-81 and
utils/misc.py:242-254; the arithmetic runs in liboryon_hip.so (K0 + K1 + K2').  The two random draws keep
the reference's host-side torch.multinomial on the global CPU generator, in the same order, so a seeded
run consumes the RNG stream exactly as the reference does with corrs_device='cpu'.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import ops
from ._lib import require_gpu


def torch_sample_select(t: Tensor, n: int) -> Tensor:
    """Exactly n indices into t's first dimension; replacement only when n > N (utils/misc.py:242-254).
    Always drawn from the global CPU generator (the reference's default corrs_device)."""
    N = t.shape[0]
    w = torch.ones(N, dtype=torch.float64)
    return torch.multinomial(w, n, replacement=(n > N))


def match_presample(feats1: Tensor, feats2: Tensor, mask1: Tensor, mask2: Tensor, threshold: float,
                    subsample_source: Optional[int] = None, half_descriptors: bool = False, mode: str = "exact",
                    mutual: bool = False, ratio: float = 0.0, ratio_radius: int = 5, topk: int = 1, topk_radius: int = 5):
    """Deterministic half of the matcher (utils/pcd.py:184-205) on the GPU.

    Returns dict(roi1 [N1,2] i64 (y,x), roi2 [N2,2] i64, min_dist [N1] f32, argmin [N1] i64, valid [N1] bool).
    When subsample_source is given and N1 exceeds it, the first RNG draw is made exactly as the reference does.
    mode: "exact" = full fp32-MFMA scan (K1); "screened16" = fp16-MFMA screening + exact fp32 re-scoring (K1s);
    "screened8" = int8-MFMA pre-screen in front of K1s (K1s8, the batched engine's default).  The screened modes return the same
    `valid` set and, on valid rows, the same argmin / min_dist bits; rows that provably cannot reach the threshold report
    valid = 0, argmin = 0 and the screening estimate of the distance.  Channels are zero-padded to the kernels' widths.
    "screened6" = the step engine's default route (K0 oryon_gather_mx6 -> oryon_match_corrs_mx6: MX-fp6 screen, lazy tail, K1x3 second
    level, device-RNG sampler): `valid` is exact on every row; `argmin` is exact on the SAMPLED rows only and `min_dist` only where the
    route needed the fp32 comparison (include/oryon_hip.h) - the dict additionally carries `corrs` [n_sel,4] i64 (y1,x1,y2,x2), the
    sampled correspondences (seed 1, max_corrs 500), and `status`.
    mutual=True: both directions from one fused exact scan (K1m, csrc/match_mutual.hip), whatever `mode` says - the screened modes
    carry no reverse screen.  The dict additionally carries `mutual` [N1] bool (valid & rev_argmin[argmin] == row), `rev_argmin` [N2]
    i64 and `rev_min_dist` [N2] f32: the nearest ANCHOR row of every query row, over the N1 rows matched - after subsample_source that
    is the subsample, not the whole mask.  With mutual=False the dict, its bytes and the RNG draws are what they always were.
    ratio > 0: the ratio test with an exclusion disc (K1r, csrc/match_second.hip) behind the exact scan, whatever `mode` says - the
    screened modes carry no second-minimum screen.  The dict additionally carries `second_dist` [N1] f32 and `second_argmin` [N1] i64,
    the best query row at least ratio_radius pixels away from the matched pixel (inf / 0 when there is none), and `keep` [N1] bool =
    gate & (min_dist <= ratio * second_dist), the gate being `mutual` when mutual=True and `valid` otherwise.  ratio = 0: off.
    topk = K > 1: the ranks of the one-to-many matcher (K1n, csrc/match_next.hip) behind the exact scan, whatever `mode` says.  The
    dict additionally carries `cand_dist` [K,N1] f32 and `cand_argmin` [K,N1] i64: rank 1 is (min_dist, argmin), rank r the best query
    row at least topk_radius pixels away from the pixels of all earlier ranks ((inf, -1) when there is none).  This is the per-sample
    reference form: K - 1 full scans over ALL N1 rows (the batched engine scans the drawn rows only).  Does not combine with mutual
    or ratio (a ValueError).  topk = 1: off - the dict, its bytes and the RNG draws are what they always were."""
    if mode not in ("exact", "screened16", "screened8", "screened6"):
        raise ValueError(f"match_presample: unknown mode {mode!r}")
    if not (0.0 <= ratio <= 1.0) or not (1 <= ratio_radius <= 1024):
        raise ValueError(f"match_presample: ratio {ratio!r} outside [0, 1] or ratio_radius {ratio_radius!r} outside [1, 1024]")
    if int(topk) != topk or not (1 <= topk <= 4) or not (1 <= topk_radius <= 1024):
        raise ValueError(f"match_presample: topk {topk!r} outside [1, 4] or topk_radius {topk_radius!r} outside [1, 1024]")
    if topk > 1 and (mutual or ratio > 0):
        raise ValueError("match_presample: topk > 1 does not combine with mutual (no reverse ranks) or ratio > 0 (the ratio test deletes "
                         "what topk keeps)")
    if mutual or ratio > 0 or topk > 1:
        mode = "exact"
    if mode != "exact" and not (0.0 < threshold <= 0.5):
        mode = "exact"                       # the screens' validity cut needs 1 - 2*threshold >= 0
    dev = require_gpu(feats1.device)
    W = feats1.shape[2]
    W2 = feats2.shape[2]
    if half_descriptors:
        # K1': the reference's corrs_device='cuda' branch rounds the descriptors to float16 first (utils/pcd.py:195-197); the
        # cosine itself is then evaluated exactly in fp32 on the rounded values (the reference's half arithmetic agrees with
        # this to ~4e-4 in distance, see tests/golden/g1_matcher_half.npz)
        feats1, feats2 = ops.round_to_f16(feats1.to(dev)), ops.round_to_f16(feats2.to(dev))
    f1 = feats1.to(torch.float32).contiguous()[None]
    f2 = feats2.to(torch.float32).contiguous()[None]
    roi1_lin, c1 = ops.roi_compact(mask1.to(dev))
    roi2_lin, c2 = ops.roi_compact(mask2.to(dev))
    n1, n2 = int(c1.item()), int(c2.item())          # the reference syncs here as well (shape of nonzero)
    roi1_lin = roi1_lin[:, :n1]
    if subsample_source is not None and n1 > subsample_source:
        idxs = torch_sample_select(roi1_lin[0], subsample_source).to(dev)
        roi1_lin = roi1_lin[:, idxs]
        n1 = subsample_source
        c1 = torch.full((1,), n1, dtype=torch.int32, device=dev)
    roi1_lin = roi1_lin.contiguous()
    out = dict(
        roi1=torch.stack((roi1_lin[0] // W, roi1_lin[0] % W), dim=1).to(torch.int64),
        roi2=torch.stack((roi2_lin[0, :n2] // W2, roi2_lin[0, :n2] % W2), dim=1).to(torch.int64))
    if n1 == 0 or n2 == 0:
        out.update(min_dist=torch.zeros(n1, device=dev), argmin=torch.zeros(n1, dtype=torch.int64, device=dev),
                   valid=torch.zeros(n1, dtype=torch.bool, device=dev))
        if mode == "screened6":
            out.update(corrs=torch.zeros((0, 4), dtype=torch.int64, device=dev), status=torch.tensor(1, device=dev))
        if mutual:
            out.update(mutual=torch.zeros(n1, dtype=torch.bool, device=dev), rev_argmin=torch.zeros(n2, dtype=torch.int64, device=dev),
                       rev_min_dist=torch.full((n2,), float("inf"), device=dev))
        if ratio > 0:
            out.update(second_dist=torch.full((n1,), float("inf"), device=dev), second_argmin=torch.zeros(n1, dtype=torch.int64, device=dev),
                       keep=torch.zeros(n1, dtype=torch.bool, device=dev))
        if topk > 1:
            out.update(cand_dist=torch.full((topk, n1), float("inf"), device=dev),
                       cand_argmin=torch.full((topk, n1), -1, dtype=torch.int64, device=dev))
        return out
    C = f1.shape[1]
    cap1, cap2 = ops.round_up(n1, ops.ROW_PAD), ops.round_up(n2, ops.ROW_PAD)
    if mode != "exact" and C > 512:
        mode = "exact"                       # the screening kernels are built for C_pad 128 / 256 / 512
    if mode == "screened6":
        c_pad = 256 if C <= 256 else 512
        a6, a_err, _, a_hat = ops.gather_mx6(f1, roi1_lin, c1, cap1, c_pad, want_f32=True)
        q6, q_err, q_norm, _ = ops.gather_mx6(f2, roi2_lin, c2, cap2, c_pad)
        corrs, n_valid, n_sel, status, min_dist, argmin, valid = ops.match_corrs_mx6(
            a_hat, a6, a_err, f2, roi1_lin, roi2_lin, q_norm, q6, q_err, c1, c2, threshold, W2, 500, 1, corr_rows=512)
        out.update(corrs=corrs[0, : int(n_sel.item())].to(torch.int64), status=status[0])
    elif mode == "screened8":
        c_pad = 256 if C <= 256 else 512
        a_hat, _, a8, a_sc, _ = ops.gather_normalise_q8(f1, roi1_lin, c1, cap1, c_pad)
        q_hat, _, q8, q_sc, q_eps = ops.gather_normalise_q8(f2, roi2_lin, c2, cap2, c_pad)
        min_dist, argmin, valid = ops.match_screened8(a_hat, q_hat, a8, q8, a_sc, q_sc, q_eps, c1, c2, threshold, C)
    elif mode == "screened16":
        c_pad = 128 if C <= 128 else (256 if C <= 256 else 512)
        a_hat, a16 = ops.gather_normalise(f1, roi1_lin, c1, cap1, c_pad=c_pad, want_f16=True)
        q_hat, q16 = ops.gather_normalise(f2, roi2_lin, c2, cap2, c_pad=c_pad, want_f16=True)
        min_dist, argmin, valid = ops.match_screened(a_hat, q_hat, a16, q16, c1, c2, threshold)
    elif mutual:
        a_hat = ops.gather_normalise(f1, roi1_lin, c1, cap1)
        q_hat = ops.gather_normalise(f2, roi2_lin, c2, cap2)
        min_dist, argmin, valid, rev_min_dist, rev_argmin, mut = ops.match_mutual(a_hat, q_hat, c1, c2, threshold)
        out.update(mutual=mut[0, :n1].bool(), rev_argmin=rev_argmin[0, :n2].to(torch.int64), rev_min_dist=rev_min_dist[0, :n2])
    else:
        a_hat = ops.gather_normalise(f1, roi1_lin, c1, cap1)
        q_hat = ops.gather_normalise(f2, roi2_lin, c2, cap2)
        min_dist, argmin, valid = ops.match(a_hat, q_hat, c1, c2, threshold)
    if ratio > 0:
        second_dist, second_argmin, keep = ops.match_second(a_hat, q_hat, c1, c2, roi2_lin.contiguous(), W2, ratio_radius, min_dist, argmin,
                                                            mut if mutual else valid, ratio)
        out.update(second_dist=second_dist[0, :n1], second_argmin=second_argmin[0, :n1].to(torch.int64), keep=keep[0, :n1].bool())
    if topk > 1:
        cand_dist = torch.empty((topk,) + tuple(min_dist.shape), dtype=torch.float32, device=dev)
        cand_argmin = torch.empty((topk,) + tuple(argmin.shape), dtype=torch.int32, device=dev)
        cand_dist[0], cand_argmin[0] = min_dist, argmin
        roi2_c = roi2_lin.contiguous()
        for r in range(1, topk):                         # rank r + 1: reads planes 0 .. r - 1, writes plane r
            ops.match_next(a_hat, q_hat, c1, c2, roi2_c, W2, topk_radius, cand_argmin[:r], out=(cand_dist[r], cand_argmin[r]))
        out.update(cand_dist=cand_dist[:, 0, :n1], cand_argmin=cand_argmin[:, 0, :n1].to(torch.int64))
    out.update(min_dist=min_dist[0, :n1], argmin=argmin[0, :n1].to(torch.int64), valid=valid[0, :n1].bool())
    return out


def nn_correspondences(feats1: Tensor, feats2: Tensor, mask1: Tensor, mask2: Tensor, threshold: float, max_corrs: int,
                       subsample_source: Optional[int], corrs_device: str = "cuda", mutual: bool = False) -> Optional[Tensor]:
    """Matches between two [D,H,W] feature maps restricted to mask==1; int64 [max_corrs,4] rows
    (y1,x1,y2,x2) on feats1.device, or None when at most one anchor pixel finds a match under the
    threshold (utils/pcd.py:177-216).  The contraction always runs on the GPU and the two
    host RNG draws are always made on the CPU generator.  corrs_device='cuda' selects the reference's fp16-descriptor
    branch (descriptors rounded to float16, utils/pcd.py:195-197); anything else its fp32 branch.
    mutual=True (no counterpart in the reference): the rows kept before the second draw are the MUTUAL nearest neighbours (valid, and
    the matched query pixel's nearest anchor - among the anchors that survived subsample_source - is this one); None when at most one
    row is mutual.  The same two host draws are made in the same order."""
    return nn_correspondences_filtered(feats1, feats2, mask1, mask2, threshold, max_corrs, subsample_source, corrs_device, mutual=mutual,
                                       ratio=0.0)


def nn_correspondences_filtered(feats1: Tensor, feats2: Tensor, mask1: Tensor, mask2: Tensor, threshold: float, max_corrs: int,
                                subsample_source: Optional[int], corrs_device: str = "cuda", mutual: bool = False, ratio: float = 0.0,
                                ratio_radius: int = 5) -> Optional[Tensor]:
    """`nn_correspondences` with the matcher's filters (no counterpart in the reference).  ratio > 0: the rows kept before the second
    draw are those that pass the ratio test with an exclusion disc of ratio_radius pixels (match_presample's `keep`: valid - or
    mutual, with mutual=True - and min_dist <= ratio * the best distance outside the disc); None when at most one row is kept.
    The same two host draws are made in the same order; with ratio = 0 this IS nn_correspondences."""
    orig_device = feats1.device
    pre = match_presample(feats1, feats2, mask1, mask2, threshold, subsample_source, half_descriptors=(corrs_device == "cuda"),
                          mutual=mutual, ratio=ratio, ratio_radius=ratio_radius)
    valid_corr = torch.nonzero(pre["keep"] if ratio > 0 else pre["mutual"] if mutual else pre["valid"]).squeeze(1)
    if valid_corr.shape[0] > 1:
        roi2 = pre["roi2"][pre["argmin"]]
        final_corrs = torch.cat((pre["roi1"][valid_corr], roi2[valid_corr]), dim=1)
        idxs = torch_sample_select(final_corrs, max_corrs).to(final_corrs.device)
        return final_corrs[idxs].to(orig_device)
    return None


def nn_correspondences_topk(feats1: Tensor, feats2: Tensor, mask1: Tensor, mask2: Tensor, threshold: float, max_corrs: int,
                            subsample_source: Optional[int], corrs_device: str = "cuda", topk: int = 1, topk_radius: int = 5,
                            topk_margin: float = 0.1) -> Optional[Tensor]:
    """`nn_correspondences` with up to topk rows per drawn anchor (no counterpart in the reference).  The same two host draws are
    made in the same order; every drawn row is then followed by its ranks 2..topk (match_presample's cand_*) that lie under the
    threshold (K1's `d < threshold` in float32) and within topk_margin of the nearest (d_r <= d_1 + margin, the sum rounded to
    float32; inf switches the margin off).  int64 [n,4] rows in (draw, rank) order, max_corrs <= n <= topk * max_corrs, or None as
    nn_correspondences.  The default radius (loss.neg_kernel_size) and margin (half of loss.pos_margin) are design choices.
    With topk = 1 this IS nn_correspondences."""
    if topk == 1:
        return nn_correspondences_filtered(feats1, feats2, mask1, mask2, threshold, max_corrs, subsample_source, corrs_device)
    if not (float(topk_margin) >= 0.0):
        raise ValueError(f"nn_correspondences_topk: topk_margin {topk_margin!r} is negative")
    orig_device = feats1.device
    pre = match_presample(feats1, feats2, mask1, mask2, threshold, subsample_source, half_descriptors=(corrs_device == "cuda"),
                          topk=topk, topk_radius=topk_radius)
    valid_corr = torch.nonzero(pre["valid"]).squeeze(1)
    if valid_corr.shape[0] <= 1:
        return None
    roi2 = pre["roi2"][pre["argmin"]]
    final_corrs = torch.cat((pre["roi1"][valid_corr], roi2[valid_corr]), dim=1)
    idxs = torch_sample_select(final_corrs, max_corrs).to(final_corrs.device)
    rows = valid_corr[idxs]                              # the anchor row of every draw
    dev = rows.device
    cd, ca = pre["cand_dist"][:, rows], pre["cand_argmin"][:, rows]                  # [K, n]
    lim = cd[0] + torch.tensor(topk_margin, dtype=torch.float32, device=dev)        # float32 sum
    take = (ca >= 0) & (cd < torch.tensor(threshold, dtype=torch.float32, device=dev)) & (cd <= lim[None])
    take[0] = True
    anchor = pre["roi1"][rows][None].expand(topk, -1, -1)
    query = pre["roi2"][ca.clamp(min=0)]
    query[0] = final_corrs[idxs][:, 2:]
    allrows = torch.cat((anchor, query), dim=2).transpose(0, 1)                      # [n, K, 4]: (draw, rank) order
    return allrows[take.transpose(0, 1)].to(orig_device)


def subpixel_offsets(feats1: Tensor, feats2: Tensor, corrs: Tensor, curv_min: float = 1e-4) -> Tuple[Tensor, Tensor]:
    """Sub-pixel refinement of the rows `nn_correspondences` (or one of its variants) returned, per sample (no counterpart in the
    reference; ops.subpix_refine, csrc/match_subpix.hip): feats1 / feats2 [D,H,W], corrs [n,4] (y1,x1,y2,x2) -> (offsets [n,2] float32
    (dy, dx) to add to (y2, x2), flags [n] uint8: 0 refined, 1 border, 2 flat or not a minimum, 3 minimum more than a pixel away) on
    feats1.device.  The fit reads the maps as given, in float32, whatever rounding the matcher applied to find the rows."""
    dev = require_gpu(feats1.device)
    n = corrs.shape[0]
    if n == 0:
        return torch.zeros((0, 2), dtype=torch.float32, device=dev), torch.zeros((0,), dtype=torch.uint8, device=dev)
    out = ops.subpix_refine(feats1.to(dev, torch.float32)[None].contiguous(), feats2.to(dev, torch.float32)[None].contiguous(),
                            corrs.to(dev).to(torch.int32).contiguous()[None], curv_min=curv_min)
    return out["offsets"][0], out["flags"][0]


def lift_pcd(depth: Tensor, camera: Tensor, xy_idxs: Optional[Tuple[Tensor, Tensor]] = None) -> Tensor:
    """Depth [H,W,1] (millimetres) + flattened K [9] -> [N,3] points (millimetres), fp32
    (utils/pcd.py:35-81).  With xy_idxs=(x_idx, y_idx) only those pixels are lifted; the caller divides
    by 1000 as pipeline.py:459-460 does."""
    dev = require_gpu(depth.device)
    H, W, D = depth.shape
    if D != 1:
        raise NotImplementedError("RGB-D lifting (D > 1) is off the registration path (utils/pcd.py:76-80)")
    d = depth[:, :, 0].to(torch.float32).contiguous()
    if xy_idxs is None:
        ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        x_idx, y_idx = xs.reshape(-1), ys.reshape(-1)
    else:
        x_idx, y_idx = xy_idxs[0].to(dev), xy_idxs[1].to(dev)
        if x_idx.numel() and (int(x_idx.min()) < 0 or int(x_idx.max()) >= W or int(y_idx.min()) < 0 or int(y_idx.max()) >= H):
            raise IndexError("lift_pcd: pixel index out of the depth image")
    cam = camera.reshape(9).to(torch.float32).to(dev)
    return ops.lift_points(d, cam, x_idx, y_idx)
