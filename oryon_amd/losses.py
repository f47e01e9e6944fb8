"""The reference's FeatureLoss (losses.py:12-263): the contrastive terms and the dice mask loss of a whole batch on the HIP kernels of
csrc/feature_loss.hip (ops.feature_loss, ops.mask_dice_sums), with the reference's names and return shapes, and their backward pass on
the kernels of csrc/feature_loss_grad.hip (ops.feature_loss_grad, ops.mask_dice_grad).

    FeatureLoss(args, device).forward(batch, net_output) -> (losses, results)
        losses  = {'mask', 'pos', 'neg'}                                                  (losses.py:124-128)
        results = {'neg_a', 'neg_q', 'mask_a', 'mask_q', 'logits_a', 'logits_q', 'iou_a', 'iou_q'}   (losses.py:130-139)
                  plus 'd_pos' [B,N], 'd_neg_a', 'd_neg_q' [B,N]: the per-correspondence distances (FMR follows from d_pos,
                  evaluation.fmr_from_distances) and 'pair_terms' [B,3]

What stays in Python is what the reference does once per batch: the coordinate rescale (the reference's own torch expressions, on the
device) and the random draws, which are made with the reference's calls in the reference's order so that a forward leaves the
generators exactly where the reference's forward - and Pipeline.feature_loss_rng_draws - leaves them.

Backward.  With grad enabled and a map (a mask logit tensor) that requires grad, the contrastive part (the dice loss) goes through a
torch.autograd.Function whose forward makes the same kernel calls and whose backward hands the upstream gradient to the gradient
kernel as a device tensor (no host read; definition: include/oryon_hip.h, oryon_feature_loss_grad / oryon_mask_dice_grad).  The index of
a negative is a constant; both functions are once_differentiable.  mask_type 'cross_entropy' is torch's own differentiable
BCEWithLogitsLoss; 'lovasz' and 'focal' raise.  Under no_grad, or for inputs that do not require grad, nothing differs from the
inference path: the same calls, the same bytes, the same random draws.  The entries of `results` are always detached."""
from __future__ import annotations

from typing import Dict, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib, ops

POOL_SIZE = 2000          # losses.py:196-197


def rescale_coords(coords: Tensor, orig_scale: Tuple[int, int], new_scale: Tuple[int, int]) -> Tensor:
    """utils/misc.py:93-122 on an integer [B,N,2|4] tensor of (y,x) columns: the product with the Python float new/orig is a float32
    tensor, the assignment into the integer column truncates it, then each column is clamped to its axis.  Returns a copy."""
    out = coords.clone()
    for col in range(out.shape[-1]):
        axis = col % 2
        out[:, :, col] = out[:, :, col] * (new_scale[axis] / orig_scale[axis])
        out[:, :, col] = torch.clamp(out[:, :, col], 0, new_scale[axis] - 1)
    return out


def featmap_corrs(corrs: Tensor, image_hw: Tuple[int, int], feat_hw: Tuple[int, int]) -> Tensor:
    """losses.py:77-78: ground-truth correspondences of the resized-image frame in feature-map pixels.  The second clamp is by FH - 1
    on all four columns, x included, as the reference has it."""
    out = rescale_coords(corrs, image_hw, feat_hw)
    return torch.clamp(out, min=0, max=feat_hw[0] - 1)


def batch_corrs(batch: Dict) -> Tensor:
    """batch['corrs'] as the [B,N,4] tensor the loss reads.  A collate hands a list over when the pairs' tables differ in length
    (data.DeviceCollate); the reference's forward has no meaning for that either, so it is an error that names the shapes."""
    corrs = batch["corrs"]
    if isinstance(corrs, Tensor):
        return corrs
    shapes = {tuple(c.shape) for c in corrs}
    if len(shapes) != 1:
        raise ValueError(f"batch['corrs'] holds tables of different shapes {sorted(shapes)}: the loss needs one [N,4] table per pair")
    return torch.stack(list(corrs))


def _dice_from_sums(sums: Tensor, hw: float) -> Tensor:
    sp, spp, spt, st = sums[:, 0], sums[:, 1], sums[:, 2], sums[:, 3]
    fg = 1.0 - (spt + 1.0) / (spp + st + 1.0)
    # background: p' t' = 1 - p - t + p t, p'^2 = 1 - 2 p + p^2, t' = 1 - t, summed over the image
    bg = 1.0 - ((hw - sp - st + spt) + 1.0) / ((hw - 2.0 * sp + spp) + (hw - st) + 1.0)
    return (0.25 * (fg.mean() + bg.mean())).to(torch.float32)


class _ContrastiveTerms(torch.autograd.Function):
    """maps -> (losses [3], d_pos, d_neg, neg_idx, pair_terms): ops.feature_loss forward, ops.feature_loss_grad backward."""

    @staticmethod
    def forward(ctx, feat_a, feat_q, corrs, valid, pool, pos_margin, neg_margin, neg_kernel, per_positive):
        out = ops.feature_loss(feat_a, feat_q, corrs, valid, pool, pos_margin, neg_margin, neg_kernel, pool_per_positive=per_positive)
        ctx.save_for_backward(feat_a, feat_q, corrs, valid, out["neg_idx"], out["d_pos"], out["d_neg"])
        ctx.margins = (pos_margin, neg_margin)
        rest = (out["d_pos"], out["d_neg"], out["neg_idx"], out["pair_terms"])
        ctx.mark_non_differentiable(*rest)
        return (out["losses"],) + rest

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        feat_a, feat_q, corrs, valid, neg_idx, d_pos, d_neg = ctx.saved_tensors
        g = g.to(feat_a.device, torch.float32).contiguous()
        grad_a, grad_q = ops.feature_loss_grad(feat_a, feat_q, corrs, valid, neg_idx, d_pos, d_neg, g, *ctx.margins)
        return (grad_a if ctx.needs_input_grad[0] else None, grad_q if ctx.needs_input_grad[1] else None) + (None,) * 7


class _DiceLoss(torch.autograd.Function):
    """logits -> dice loss from the sums of ops.mask_dice_sums: the closed form forward, ops.mask_dice_grad backward."""

    @staticmethod
    def forward(ctx, logits, gt, sums):
        ctx.save_for_backward(logits, gt, sums)
        return _dice_from_sums(sums, float(logits.shape[-2] * logits.shape[-1]))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logits, gt, sums = ctx.saved_tensors
        return ops.mask_dice_grad(logits, gt, sums, g.to(logits.device, torch.float32).reshape(1).contiguous()), None, None


class FeatureLoss:
    """Contrastive loss with positive and hardest-negative samples plus the mask loss (losses.py:12-141)."""

    def __init__(self, args, device: str):
        self.device = device
        self.args = args
        self.pos_margin = args.loss.pos_margin
        self.neg_margin = args.loss.neg_margin
        self.neg_kernel = args.loss.neg_kernel_size
        self.hard_negatives = args.loss.hard_negatives
        self.mask_th = args.test.mask_threshold
        self.mask_type = args.loss.mask_type
        if self.mask_type == "cross_entropy":
            self._bce = torch.nn.BCEWithLogitsLoss()
        elif self.mask_type in ("lovasz", "focal"):
            raise NotImplementedError(f"Mask loss function {self.mask_type} is not part of this build")
        elif self.mask_type != "dice":
            raise RuntimeError(f"Mask loss function {self.mask_type} not implemented.")

    # ------------------------------------------------------------------ losses.py:40-62
    def mask_loss(self, pred_logits: Tensor, gt: Tensor):
        """pred_logits [B,1,H1,W1] (or [B,H1,W1]), gt [B,H2,W2] -> (loss, pred_mask [B,H1,W1] int32, logits [B,H1,W1], iou [B]).
        The ground truth is resized with nearest interpolation to the logits' size.  'dice': DiceLoss(weight=[0.5, 0.5]) in closed
        form from the four sums of oryon_mask_dice_sums,
            loss = 1/4 [mean_b(1 - (S_pt + 1) / (S_pp + S_t + 1)) + mean_b(1 - (S_p't' + 1) / (S_p'p' + S_t' + 1))]
        with the background class p' = 1 - p, t' = 1 - t from the same sums and H W; the means are over all B images.  The loss is
        differentiable when pred_logits requires grad; the mask, the returned logits and the IoU never are."""
        dev = _lib.require_gpu(self.device)
        logits = (pred_logits.squeeze(1) if pred_logits.dim() == 4 else pred_logits).to(dev, torch.float32).contiguous()
        gt = gt.to(dev)
        if tuple(gt.shape[-2:]) != tuple(logits.shape[-2:]):
            gt = ops.mask_resize_nearest(gt, tuple(logits.shape[-2:]))
        sums, pred_mask, counts = ops.mask_dice_sums(logits.detach(), gt, self.mask_th)
        if self.mask_type == "dice":
            if torch.is_grad_enabled() and logits.requires_grad:
                loss = _DiceLoss.apply(logits, gt.to(torch.int32).contiguous(), sums)
            else:
                loss = _dice_from_sums(sums, float(logits.shape[-2] * logits.shape[-1]))
        else:
            loss = self._bce(logits, (gt != 0).to(torch.float32))
        iou = counts[:, 0].to(torch.float32) / counts[:, 1].to(torch.float32)         # 0 / 0 = NaN, as utils/metrics.py:38
        return loss, pred_mask, logits.detach(), iou

    # ------------------------------------------------------------------ losses.py:196-199, 254
    def draw_pool(self, featmap: Tensor, valid, n_corr: int):
        """The pool tables of one forward, drawn with the reference's calls in the reference's order: anchors first, then queries, one
        draw per pair with valid == 1.  -> (pool [B,2,n] int32 on the maps' device or None = the whole map, pool_per_positive)."""
        B, _, FH, FW = featmap.shape
        HW = FH * FW
        if self.hard_negatives and HW <= POOL_SIZE:
            return None, False
        n = POOL_SIZE if self.hard_negatives else n_corr
        pool = torch.zeros((B, 2, n), dtype=torch.int32, device=featmap.device)
        for side in (0, 1):
            for i_b in range(B):
                if valid[i_b] == 1:
                    if self.hard_negatives:           # torch_sample_select(featmap_i, 2000), utils/misc.py:242-254
                        idx = torch.multinomial(torch.ones(HW, dtype=float).to(featmap.device), POOL_SIZE, replacement=False)
                    else:                              # losses.py:254, the CPU generator
                        idx = torch.randint(0, HW, (n_corr,))
                    pool[i_b, side] = idx.to(featmap.device, torch.int32)
        return pool, not self.hard_negatives

    # ------------------------------------------------------------------ losses.py:64-141
    def forward(self, batch: Dict, net_output: Dict) -> Tuple[Dict, Dict]:
        dev = _lib.require_gpu(self.device)
        featmap_a = net_output["featmap_a"].to(dev, torch.float32).contiguous()
        featmap_q = net_output["featmap_q"].to(dev, torch.float32).contiguous()
        CH, CW = batch["anchor"]["rgb"].shape[2:]
        FH, FW = featmap_a.shape[2:]
        gt_corrs = featmap_corrs(batch_corrs(batch).to(dev), (CH, CW), (FH, FW))
        valid_host = batch["valid"].cpu().tolist() if isinstance(batch["valid"], Tensor) else list(batch["valid"])
        valid = torch.tensor([int(v) for v in valid_host], dtype=torch.int32, device=dev)
        pool, per_positive = self.draw_pool(featmap_a, valid_host, gt_corrs.shape[1])
        corrs32 = gt_corrs.to(torch.int32).contiguous()
        if torch.is_grad_enabled() and (featmap_a.requires_grad or featmap_q.requires_grad):
            keys = ("losses", "d_pos", "d_neg", "neg_idx", "pair_terms")
            out = dict(zip(keys, _ContrastiveTerms.apply(featmap_a, featmap_q, corrs32, valid, pool, self.pos_margin, self.neg_margin,
                                                         float(self.neg_kernel), per_positive)))
        else:
            out = ops.feature_loss(featmap_a, featmap_q, corrs32, valid, pool, self.pos_margin, self.neg_margin,
                                   float(self.neg_kernel), pool_per_positive=per_positive)
        mask_loss_a, pred_mask_a, pred_logits_a, iou_a = self.mask_loss(net_output["mask_a"], batch["anchor"]["mask"])
        mask_loss_q, pred_mask_q, pred_logits_q, iou_q = self.mask_loss(net_output["mask_q"], batch["query"]["mask"])
        losses = {"mask": 0.5 * (mask_loss_a + mask_loss_q), "pos": out["losses"][0], "neg": 0.5 * (out["losses"][1] + out["losses"][2])}
        idx = out["neg_idx"]
        neg_yx = torch.stack([torch.div(idx, FW, rounding_mode="floor"), idx % FW], dim=-1).to(torch.float32)       # [B,2,N,2] (y,x)
        results = {"neg_a": neg_yx[:, 0], "neg_q": neg_yx[:, 1], "mask_a": pred_mask_a, "mask_q": pred_mask_q, "logits_a": pred_logits_a,
                   "logits_q": pred_logits_q, "iou_a": iou_a, "iou_q": iou_q,
                   "d_pos": out["d_pos"], "d_neg_a": out["d_neg"][:, 0], "d_neg_q": out["d_neg"][:, 1], "pair_terms": out["pair_terms"]}
        return losses, results

    __call__ = forward
