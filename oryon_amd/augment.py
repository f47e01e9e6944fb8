"""The reference's training augmentations (datasets.py:98-114 build_augs; utils/augmentations.py:17-127), host half: the random draws,
the box / correspondence bookkeeping of the flips and the per-image table the K-1a kernels read (csrc/augment.hip, include/oryon_hip.h).

The pixel arithmetic (torchvision's ColorJitter on the float64 image, the hue stage in float32) runs on the device only,
inside the resize launches of `DeviceCollate`; no CPU pixel path exists here.

`draw_pair_params` makes the reference's calls to Python's `random` and to torch's global generator, in the reference's order, for one
(anchor, query) pair: for each enabled transform in the order jitter, bright, hflip, vflip the anchor's gate `random.random() < 0.5`, the
anchor's parameter draws when the gate passed, then the same for the query.  A ColorJitter parameter draw is `torch.randperm(4)` followed
by one `torch.empty(1).uniform_(lo, hi)` per factor that is not None, in the order brightness, contrast, saturation, hue."""
from __future__ import annotations

import random
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3
AUG_SLOTS, AUG_STRIDE = 8, 18                         # ORYON_AUG_SLOTS, ORYON_AUG_STRIDE
AUG_HFLIP, AUG_VFLIP = 1, 2
NAMES = ("jitter", "bright", "hflip", "vflip")

# factor ranges by op id; None = the op is not part of the transform
JITTER_RANGES = ((0.875, 1.125), (0.5, 1.5), (0.5, 1.5), (-0.05, 0.05))     # ColorJitter(brightness=.125, contrast=.5, saturation=.5, hue=.05)
BRIGHT_RANGES = ((0.75, 1.25), None, None, None)                           # ColorJitter(brightness=.25, contrast=0, saturation=0, hue=0)


@dataclass
class ColorApplication:
    """One ColorJitter call: the ops run in the order of `fn_idx` (a permutation of the four ids), an op whose factor is None is skipped."""
    fn_idx: Tuple[int, int, int, int]
    factors: Tuple[Optional[float], Optional[float], Optional[float], Optional[float]]

    def ops(self) -> List[Tuple[int, float]]:
        return [(int(i), float(self.factors[int(i)])) for i in self.fn_idx if self.factors[int(i)] is not None]


@dataclass
class AugParams:
    """What was drawn for one image: up to two colour applications (jitter, then bright) and the two flip flags."""
    jitter: Optional[ColorApplication] = None
    bright: Optional[ColorApplication] = None
    hflip: bool = False
    vflip: bool = False

    def ops(self) -> List[Tuple[int, float]]:
        return [op for app in (self.jitter, self.bright) if app is not None for op in app.ops()]

    @property
    def identity(self) -> bool:
        return self.jitter is None and self.bright is None and not self.hflip and not self.vflip


def enabled(augs) -> Tuple[bool, bool, bool, bool]:
    """(jitter, bright, hflip, vflip) of the config's `augs` node (attributes or mapping: augs.rgb.<name>); None = all off."""
    if augs is None:
        return (False, False, False, False)
    rgb = augs["rgb"] if isinstance(augs, dict) else augs.rgb
    return tuple(bool(rgb[n] if isinstance(rgb, dict) else getattr(rgb, n)) for n in NAMES)


def draw_color(ranges) -> ColorApplication:
    """torchvision's ColorJitter.get_params: the permutation, then one uniform per live factor."""
    fn_idx = tuple(int(i) for i in torch.randperm(4))
    factors = tuple(None if r is None else float(torch.empty(1).uniform_(r[0], r[1])) for r in ranges)
    return ColorApplication(fn_idx, factors)


def draw_pair_params(augs) -> Tuple[AugParams, AugParams]:
    on = enabled(augs)
    pair = (AugParams(), AugParams())
    for name, live in zip(NAMES, on):
        if not live:
            continue
        for p in pair:
            if random.random() < 0.5:
                if name == "jitter":
                    p.jitter = draw_color(JITTER_RANGES)
                elif name == "bright":
                    p.bright = draw_color(BRIGHT_RANGES)
                elif name == "hflip":
                    p.hflip = True
                else:
                    p.vflip = True
    return pair


def build_table(params: Sequence[AugParams]) -> Tensor:
    """[n, AUG_STRIDE] float64 on the host, the layout of include/oryon_hip.h (K-1a): flip bits, a reserved zero, then the colour chain
    as (op id, factor) slots in execution order, -1 in the id of an empty slot."""
    table = torch.zeros((len(params), AUG_STRIDE), dtype=torch.float64)
    table[:, 2::2] = -1.0
    for i, p in enumerate(params):
        ops = p.ops()
        assert len(ops) <= AUG_SLOTS and sum(1 for op, _ in ops if op == OP_CONTRAST) <= 1, ops
        table[i, 0] = (AUG_HFLIP if p.hflip else 0) | (AUG_VFLIP if p.vflip else 0)
        for k, (op, f) in enumerate(ops):
            table[i, 2 + 2 * k], table[i, 3 + 2 * k] = op, f
    return table


def flip_box(box, hw_size, hflip: bool, vflip: bool) -> Tensor:
    """[y, x, h, w] of the mirrored image (utils/augmentations.py:64-65, 102-103); H, W = the sensor size."""
    H, W = int(hw_size[0]), int(hw_size[1])
    y, x, h, w = box
    if hflip:
        y, x, h, w = y, W - w - x, h, w
    if vflip:
        y, x, h, w = H - y - h, x, h, w
    return torch.tensor([y, x, h, w])


def flip_coords(coords: Tensor, hw_size, hflip: bool, vflip: bool) -> Tensor:
    """(y, x) correspondences [N,2] of the mirrored image (utils/augmentations.py:66, 105), a copy."""
    H, W = int(hw_size[0]), int(hw_size[1])
    out = coords.clone()
    if hflip:
        out[:, 1] = W - out[:, 1] - 1
    if vflip:
        out[:, 0] = H - out[:, 0] - 1
    return out
