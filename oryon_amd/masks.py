"""Mask clean-up for someone with one mask in hand (the façade over ops.mask_clean, as geo6d.pose_depth_score is over ops.pose_verify).

    clean_mask(mask, mode="largest", frac=0.25, fill_holes=False) -> the cleaned mask, same type and shape

The definition is include/oryon_hip.h's, oryon_mask_clean (csrc/mask_clean.hip): with fill_holes the enclosed holes of the foreground
(mask == 1) are filled, then of its 8-connected components the largest one is kept ('largest'; ties: the one that starts first in raster
order), or every one of at least frac x the largest area ('area'), or all of them ('all': only useful with fill_holes).  The reference
has no counterpart.  The work is done on the GPU; a numpy array or a CPU tensor is copied there and back."""
from __future__ import annotations

import numpy as np
import torch

from . import ops

MODES = ops.MASK_CLEAN_MODES


def clean_mask(mask, mode: str = "largest", frac: float = 0.25, fill_holes: bool = False, *, device="cuda"):
    """mask [H,W] or [n,H,W], a numpy array or a torch tensor on any device, of any integer or bool dtype: foreground = (mask == 1).
    -> the cleaned mask with 0 / 1 entries, of the type, dtype, device and shape given.  frac = 0.25 is a design choice, not tuned on
    data."""
    is_np = isinstance(mask, np.ndarray)
    if not is_np and not isinstance(mask, torch.Tensor):
        raise TypeError("clean_mask takes a numpy array or a torch tensor")
    t = torch.from_numpy(np.ascontiguousarray(mask)) if is_np else mask
    if t.dim() not in (2, 3):
        raise ValueError("clean_mask: mask is [H, W] or [n, H, W]")
    if t.is_floating_point() or t.is_complex():
        raise TypeError("clean_mask: an integer or bool mask (foreground = 1)")
    dev = t.device if t.is_cuda else torch.device(device)
    out = ops.mask_clean((t == 1).to(dev, torch.int32), mode=mode, frac=frac, fill_holes=fill_holes)
    out = out.to(t.device, t.dtype)
    return out.numpy() if is_np else out
