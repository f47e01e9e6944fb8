"""Thin tensor-level wrappers over the C ABI (one function per entry point of include/oryon_hip.h).

Every wrapper takes torch CUDA tensors, allocates outputs with torch (plumbing) and launches the HIP
kernel on the current torch stream.  Nothing here computes: the arithmetic lives in liboryon_hip.so."""
from __future__ import annotations

import ctypes
import functools
import weakref
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

MATCH_TILE = 128
ROW_PAD = 256      # row capacities are multiples of 256; K0 zero-fills rows [n, round_up(n, 256)) of every map - rows beyond that
                   # are NOT written (the matchers never read past ceil(n / 256) * 256)
K_PAD = 32
AUG_SLOTS, AUG_STRIDE = 8, 18      # ORYON_AUG_SLOTS, ORYON_AUG_STRIDE (include/oryon_hip.h): the augmentation table of K-1a


def _on_tensor_device(fn):
    """Run the wrapped C-ABI call with the first tensor argument's GPU as the current HIP device: the library launches on the
    stream it is handed, but kernel attributes (dynamic-LDS opt-in) and hipMemsetAsync target the CURRENT device."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        for a in args:
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return wrapped


def round_up(x: int, m: int) -> int:
    return ((int(x) + m - 1) // m) * m


@_on_tensor_device
def round_to_f16(x: torch.Tensor) -> torch.Tensor:
    """fp32 CUDA tensor rounded to the nearest float16 value, returned as fp32 (K1' input rounding)."""
    _lib.require_gpu(x.device)
    x = x.to(torch.float32).contiguous()
    out = torch.empty_like(x)
    check(lib().oryon_round_to_f16_f32(ptr(x), ptr(out), x.numel(), stream_ptr(x.device)), "oryon_round_to_f16_f32")
    return out


@_on_tensor_device
def quick_gelu_bf16(x: torch.Tensor) -> torch.Tensor:
    """x * sigmoid(1.702 x) on a bf16 CUDA tensor in one pass (B1); used by the CLIP residual blocks at inference."""
    _lib.require_gpu(x.device)
    assert x.dtype == torch.bfloat16
    x = x.contiguous()
    y = torch.empty_like(x)
    check(lib().oryon_quick_gelu_bf16(ptr(x), ptr(y), x.numel(), stream_ptr(x.device)), "oryon_quick_gelu_bf16")
    return y


@_on_tensor_device
def add_layernorm_bf16(x: torch.Tensor, delta: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor, eps: float):
    """(x + delta, LayerNorm(x + delta)) for bf16 CUDA tensors in one pass (B2); delta None -> (x, LayerNorm(x)).
    Used by the CLIP residual blocks at inference."""
    _lib.require_gpu(x.device)
    assert x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and bias.dtype == torch.bfloat16
    D = x.shape[-1]
    x = x.contiguous()
    h = torch.empty_like(x)
    if delta is None:
        s_out = x
        check(lib().oryon_add_layernorm_bf16(ptr(x), None, ptr(weight), ptr(bias), x.numel() // D, D, eps, None, ptr(h),
                                             stream_ptr(x.device)), "oryon_add_layernorm_bf16")
    else:
        assert delta.shape == x.shape and delta.dtype == torch.bfloat16
        delta = delta.contiguous()
        s_out = delta                                  # the sum overwrites the branch output (a temporary of the caller)
        check(lib().oryon_add_layernorm_bf16(ptr(x), ptr(delta), ptr(weight), ptr(bias), x.numel() // D, D, eps, ptr(s_out), ptr(h),
                                             stream_ptr(x.device)), "oryon_add_layernorm_bf16")
    return s_out, h


@_on_tensor_device
def add_layernorm_f32(x: torch.Tensor, delta: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor, eps: float):
    """fp32 twin of add_layernorm_bf16 (the fp32 / fp16x3 inference path of the towers): (x + delta, LayerNorm(x + delta))."""
    _lib.require_gpu(x.device)
    assert x.dtype == torch.float32 and weight.dtype == torch.float32 and bias.dtype == torch.float32
    D = x.shape[-1]
    x = x.contiguous()
    h = torch.empty_like(x)
    if delta is None:
        s_out = x
        check(lib().oryon_add_layernorm_f32(ptr(x), None, ptr(weight), ptr(bias), x.numel() // D, D, eps, None, ptr(h),
                                            stream_ptr(x.device)), "oryon_add_layernorm_f32")
    else:
        assert delta.shape == x.shape and delta.dtype == torch.float32
        delta = delta.contiguous()
        s_out = delta
        check(lib().oryon_add_layernorm_f32(ptr(x), ptr(delta), ptr(weight), ptr(bias), x.numel() // D, D, eps, ptr(s_out), ptr(h),
                                            stream_ptr(x.device)), "oryon_add_layernorm_f32")
    return s_out, h


def add_layernorm(x, delta, weight, bias, eps):
    """Dispatch on the stream's dtype (bf16 or fp32)."""
    return (add_layernorm_bf16 if x.dtype == torch.bfloat16 else add_layernorm_f32)(x, delta, weight, bias, eps)


@_on_tensor_device
def swin_window_attention_bf16(qkv: torch.Tensor, pad_qkv: torch.Tensor, bias_t: torch.Tensor, heads: int, shift: int) -> torch.Tensor:
    """Shifted-window attention (window 7, head dim 32) on un-windowed q|k|v tokens [B,H,W,3C] bf16 -> [B,H,W,C] bf16 (B3)."""
    _lib.require_gpu(qkv.device)
    assert qkv.dtype == torch.bfloat16 and pad_qkv.dtype == torch.bfloat16 and bias_t.dtype == torch.float32
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    assert C3 == 3 * C and pad_qkv.numel() == C3 and bias_t.shape == (heads, 49, 49)
    qkv = qkv.contiguous()
    out = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=qkv.device)
    check(lib().oryon_swin_window_attention_bf16(ptr(qkv), ptr(pad_qkv.contiguous()), ptr(bias_t.contiguous()), B, H, W, C, heads, shift,
                                                 ptr(out), stream_ptr(qkv.device)), "oryon_swin_window_attention_bf16")
    return out


@_on_tensor_device
def swin_window_attention_f32(qkv: torch.Tensor, pad_qkv: torch.Tensor, bias_t: torch.Tensor, heads: int, shift: int) -> torch.Tensor:
    """The B3 kernel on fp32 tensors: [B,H,W,3C] fp32 -> [B,H,W,C] fp32 (fp32 evaluation of the Swin guidance tower)."""
    _lib.require_gpu(qkv.device)
    assert qkv.dtype == torch.float32 and pad_qkv.dtype == torch.float32 and bias_t.dtype == torch.float32
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    assert C3 == 3 * C and pad_qkv.numel() == C3 and bias_t.shape == (heads, 49, 49)
    qkv = qkv.contiguous()
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=qkv.device)
    check(lib().oryon_swin_window_attention_f32(ptr(qkv), ptr(pad_qkv.contiguous()), ptr(bias_t.contiguous()), B, H, W, C, heads, shift,
                                                ptr(out), stream_ptr(qkv.device)), "oryon_swin_window_attention_f32")
    return out


@_on_tensor_device
def fusion_class_layer(x_nhwc: torch.Tensor, text_guidance: torch.Tensor, params) -> torch.Tensor:
    """The class-aggregation layer of ImageTextFusion for T = 1 (see oryon_fusion_class_layer_f32): x [B,24,24,128] fp32 NHWC, text_guidance
    [B,128], params = the 14 fp32 parameter tensors (norm1 w/b, q w/b, k w/b, v w/b, norm2 w/b, MLP.0 w/b, MLP.2 w/b) -> [B,24,24,128]."""
    dev = _lib.require_gpu(x_nhwc.device)
    B = x_nhwc.shape[0]
    assert x_nhwc.dtype == torch.float32 and tuple(x_nhwc.shape[1:]) == (24, 24, 128) and tuple(text_guidance.shape) == (B, 128)
    x, tg = x_nhwc.contiguous(), text_guidance.to(torch.float32).contiguous()
    out = torch.empty_like(x)
    if B == 0:
        return out
    ps = [p.detach().to(torch.float32).contiguous() for p in params]
    shapes = [(128,), (128,), (128, 256), (128,), (128, 256), (128,), (128, 128), (128,), (128,), (128,), (512, 128), (512,), (128, 512), (128,)]
    assert [tuple(p.shape) for p in ps] == shapes, [tuple(p.shape) for p in ps]
    w = _lib.FusionClassWeights(*[ptr(p) for p in ps])
    check(lib().oryon_fusion_class_layer_f32(ptr(x), ptr(tg), ctypes.byref(w), B, ptr(out), stream_ptr(dev)), "oryon_fusion_class_layer_f32")
    return out


_conv24_images: dict = {}


def _conv24_image(weight: torch.Tensor) -> torch.Tensor:
    """Packed fp16 hi / lo fragment image of a conv weight [cout, cin, k, k], made once per live tensor and in-place version."""
    key = id(weight)
    hit = _conv24_images.get(key)
    if hit is not None and (hit[0]() is not weight or hit[1] != (weight._version, weight.data_ptr(), tuple(weight.shape))):
        hit = None
    if hit is None:
        cout, cin, k, _ = weight.shape
        nbytes = int(lib().oryon_conv24_image_bytes(cout, cin, k))
        if nbytes <= 0:
            raise _lib.OryonError(f"oryon_conv24_f16x3: unsupported weight shape {tuple(weight.shape)}")
        w = weight.detach().to(torch.float32).contiguous()
        img = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        check(lib().oryon_conv24_pack_f16x3(ptr(w), cout, cin, k, ptr(img), stream_ptr(w.device)), "oryon_conv24_pack_f16x3")
        if len(_conv24_images) > 64:
            _conv24_images.clear()
        ref = weakref.ref(weight, lambda _r, k_=key: _conv24_images.pop(k_, None))
        hit = _conv24_images[key] = (ref, (weight._version, weight.data_ptr(), tuple(weight.shape)), img)
    return hit[2]


def conv24_supported(x_nhwc: torch.Tensor, weight: torch.Tensor) -> bool:
    return (x_nhwc.is_cuda and x_nhwc.dtype == torch.float32 and x_nhwc.dim() == 4
            and tuple(x_nhwc.shape[1:3]) == (24, 24) and weight.dim() == 4 and weight.shape[2] == weight.shape[3] and weight.shape[2] in (3, 7)
            and weight.shape[0] % 64 == 0 and weight.shape[1] % 4 == 0 and x_nhwc.shape[3] == weight.shape[1])


@_on_tensor_device
def conv24_f16x3(x_nhwc: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], relu: bool = False) -> torch.Tensor:
    """act(conv2d(x, weight, bias, stride 1, padding k // 2)) for 24 x 24 maps: x [n,24,24,cin] fp32 NHWC, weight [cout,cin,k,k] (torch
    layout, k = 3 or 7) -> [n,24,24,cout] fp32 NHWC (ImageTextFusion's conv1 / guidance_projection; fp16x3 MFMA products, fp32-grade).
    Inference only: no autograd graph is recorded."""
    dev = _lib.require_gpu(x_nhwc.device)
    assert conv24_supported(x_nhwc, weight), (x_nhwc.shape, weight.shape)
    x = x_nhwc.contiguous()
    n, cout, cin, k = x.shape[0], weight.shape[0], weight.shape[1], weight.shape[2]
    img = _conv24_image(weight)
    b = None if bias is None else bias.detach().to(torch.float32).contiguous()
    y = torch.empty((n, 24, 24, cout), dtype=torch.float32, device=dev)
    if n == 0:
        return y
    check(lib().oryon_conv24_f16x3(ptr(x), n, cin, ptr(img), ptr(b), cout, k, int(relu), ptr(y), stream_ptr(dev)), "oryon_conv24_f16x3")
    return y


@_on_tensor_device
def fusion_window_attention(qk: torch.Tensor, v: torch.Tensor, heads: int, window: int, shift: int) -> torch.Tensor:
    """Shifted-window attention of ImageTextFusion's guided Swin blocks on un-windowed tokens: qk [B,H,W,2C] (q | k projections),
    v [B,H,W,C] fp32 -> [B,H,W,C] fp32 (roll, windows, masked softmax attention, windows back, roll back in one kernel; fp16x3 MFMA products,
    fp32-grade)."""
    _lib.require_gpu(qk.device)
    B, H, W, C2 = qk.shape
    C = C2 // 2
    assert qk.dtype == torch.float32 and v.dtype == torch.float32 and tuple(v.shape) == (B, H, W, C) and C2 == 2 * C
    qk, v = qk.contiguous(), v.contiguous()
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=qk.device)
    if B == 0:
        return out
    check(lib().oryon_fusion_window_attention_f32(ptr(qk), ptr(v), B, H, W, C, heads, window, shift, ptr(out), stream_ptr(qk.device)),
          "oryon_fusion_window_attention_f32")
    return out


@_on_tensor_device
def rgb_resize_bilinear(rgb_hwc: torch.Tensor, out_hw: Tuple[int, int]) -> torch.Tensor:
    """uint8 [n,HI,WI,3] -> fp32 [n,3,HO,WO] in [0,1] (K-1: /255., CHW, bilinear align_corners=False, fp64 arithmetic)."""
    _lib.require_gpu(rgb_hwc.device)
    assert rgb_hwc.dtype == torch.uint8 and rgb_hwc.dim() == 4 and rgb_hwc.shape[3] == 3
    rgb_hwc = rgb_hwc.contiguous()
    n, HI, WI = rgb_hwc.shape[:3]
    out = torch.empty((n, 3, int(out_hw[0]), int(out_hw[1])), dtype=torch.float32, device=rgb_hwc.device)
    check(lib().oryon_rgb_resize_bilinear(ptr(rgb_hwc), n, HI, WI, int(out_hw[0]), int(out_hw[1]), ptr(out), stream_ptr(rgb_hwc.device)),
          "oryon_rgb_resize_bilinear")
    return out


def _flip_table(table: torch.Tensor, n: int, device) -> torch.Tensor:
    """The per-image augmentation table [n, AUG_STRIDE] float64 (include/oryon_hip.h, K-1a; oryon_amd.augment.build_table) on `device`."""
    assert table.dtype == torch.float64 and tuple(table.shape) == (n, AUG_STRIDE) and table.device == device, (table.dtype, table.shape, table.device)
    return table.contiguous()


@_on_tensor_device
def rgb_augment_resize(rgb_hwc: torch.Tensor, table: torch.Tensor, out_hw: Tuple[int, int]) -> torch.Tensor:
    """uint8 [n,HI,WI,3] + table [n, AUG_STRIDE] float64 (flip bits and the colour chain of every image) -> fp32 [n,3,HO,WO]: K-1a,
    rgb_resize_bilinear of the flipped, colour-jittered images in two launches (gray mean for the contrast op, then the fused resize)."""
    _lib.require_gpu(rgb_hwc.device)
    assert rgb_hwc.dtype == torch.uint8 and rgb_hwc.dim() == 4 and rgb_hwc.shape[3] == 3
    rgb_hwc = rgb_hwc.contiguous()
    n, HI, WI = rgb_hwc.shape[:3]
    table = _flip_table(table, n, rgb_hwc.device)
    out = torch.empty((n, 3, int(out_hw[0]), int(out_hw[1])), dtype=torch.float32, device=rgb_hwc.device)
    ws_bytes = int(lib().oryon_rgb_augment_workspace_bytes(n))
    ws = _lib.workspace(rgb_hwc.device, ws_bytes)
    check(lib().oryon_rgb_augment_resize(ptr(rgb_hwc), ptr(table), n, HI, WI, int(out_hw[0]), int(out_hw[1]), ptr(ws), ws_bytes, ptr(out),
                                         stream_ptr(rgb_hwc.device)), "oryon_rgb_augment_resize")
    return out


@_on_tensor_device
def resize_bilinear(x: torch.Tensor, out_hw: Tuple[int, int], round_output: bool = False, flip_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [n,HI,WI] -> fp32 [n,HO,WO], torch bilinear (align_corners=False); round_output mimics torchvision on integer images.
    flip_table [n, AUG_STRIDE] float64: image i is mirrored as the flip bits of row i say before the resize (K-1a)."""
    _lib.require_gpu(x.device)
    x = x.to(torch.float32).contiguous()
    n, HI, WI = x.shape
    out = torch.empty((n, int(out_hw[0]), int(out_hw[1])), dtype=torch.float32, device=x.device)
    if flip_table is not None:
        check(lib().oryon_resize_bilinear_f32_flip(ptr(x), ptr(_flip_table(flip_table, n, x.device)), n, HI, WI, int(out_hw[0]), int(out_hw[1]),
                                                   int(round_output), ptr(out), stream_ptr(x.device)), "oryon_resize_bilinear_f32_flip")
        return out
    check(lib().oryon_resize_bilinear_f32(ptr(x), n, HI, WI, int(out_hw[0]), int(out_hw[1]), int(round_output), ptr(out),
                                          stream_ptr(x.device)), "oryon_resize_bilinear_f32")
    return out


@_on_tensor_device
def roi_compact(mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """mask [n_maps, H, W] (or [H,W]) int32 -> (roi [n_maps, HW] int32 linear indices, count [n_maps] int32)."""
    if mask.dim() == 2:
        mask = mask[None]
    _lib.require_gpu(mask.device)
    mask = mask.to(torch.int32).contiguous()
    n_maps, HW = mask.shape[0], mask.shape[1] * mask.shape[2]
    roi = torch.empty((n_maps, HW), dtype=torch.int32, device=mask.device)
    count = torch.empty((n_maps,), dtype=torch.int32, device=mask.device)
    check(lib().oryon_roi_compact(ptr(mask), n_maps, HW, ptr(roi), ptr(count), stream_ptr(mask.device)), "oryon_roi_compact")
    return roi, count


@_on_tensor_device
def mask_from_logits(logits: torch.Tensor, threshold: float) -> torch.Tensor:
    _lib.require_gpu(logits.device)
    logits = logits.to(torch.float32).contiguous()
    out = torch.empty(logits.shape, dtype=torch.int32, device=logits.device)
    check(lib().oryon_mask_from_logits(ptr(logits), logits.numel(), float(threshold), ptr(out), stream_ptr(logits.device)),
          "oryon_mask_from_logits")
    return out


@_on_tensor_device
def mask_resize_nearest(mask: torch.Tensor, out_hw: Tuple[int, int], flip_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 masks [n,HI,WI] -> int32 [n,HO,WO] with torch's legacy 'nearest' index rule.
    flip_table [n, AUG_STRIDE] float64: mask i is mirrored as the flip bits of row i say before the resize (K-1a)."""
    if mask.dim() == 2:
        mask = mask[None]
    _lib.require_gpu(mask.device)
    m = mask.to(torch.uint8).contiguous()
    n, HI, WI = m.shape
    out = torch.empty((n, int(out_hw[0]), int(out_hw[1])), dtype=torch.int32, device=m.device)
    if flip_table is not None:
        check(lib().oryon_mask_resize_nearest_flip(ptr(m), ptr(_flip_table(flip_table, n, m.device)), n, HI, WI, int(out_hw[0]), int(out_hw[1]),
                                                   ptr(out), stream_ptr(m.device)), "oryon_mask_resize_nearest_flip")
        return out
    check(lib().oryon_mask_resize_nearest(ptr(m), n, HI, WI, int(out_hw[0]), int(out_hw[1]), ptr(out), stream_ptr(m.device)),
          "oryon_mask_resize_nearest")
    return out


@_on_tensor_device
def roi_subsample_(roi: torch.Tensor, count: torch.Tensor, max_keep: int, seed: int, map_key: Optional[torch.Tensor] = None) -> None:
    """In-place device-RNG subsample of every ROI list to at most max_keep entries (order preserved)."""
    _lib.require_gpu(roi.device)
    check(lib().oryon_roi_subsample(ptr(roi), ptr(count), roi.shape[0], roi.shape[1], int(max_keep), int(seed) & (2**64 - 1),
                                    ptr(map_key), stream_ptr(roi.device)), "oryon_roi_subsample")


@_on_tensor_device
def gather_normalise(feat: torch.Tensor, roi: torch.Tensor, count: torch.Tensor, rows_cap: int, c_pad: Optional[int] = None,
                     want_f16: bool = False):
    """feat [n_maps,C,H,W] fp32, roi [n_maps, stride] -> [n_maps, rows_cap, C_pad] unit rows (rows_cap % 256 == 0);
    with want_f16 also the IEEE-half copy used by the screening pass (returns (f32, f16))."""
    _lib.require_gpu(feat.device)
    assert feat.dtype == torch.float32 and feat.is_contiguous()
    n_maps, C = feat.shape[0], feat.shape[1]
    HW = feat.shape[2] * feat.shape[3]
    Cp = int(c_pad) if c_pad else round_up(C, K_PAD)
    out = torch.empty((n_maps, rows_cap, Cp), dtype=torch.float32, device=feat.device)
    out16 = torch.empty((n_maps, rows_cap, Cp), dtype=torch.float16, device=feat.device) if want_f16 else None
    check(lib().oryon_gather_normalise_f32(ptr(feat), n_maps, C, HW, ptr(roi), roi.shape[1], ptr(count), rows_cap, Cp,
                                           ptr(out), ptr(out16), stream_ptr(feat.device)), "oryon_gather_normalise_f32")
    return (out, out16) if want_f16 else out


def unpermute_k(x: torch.Tensor) -> torch.Tensor:
    """K0 stores every descriptor row with k permuted inside groups of 8 (position 8g+4h+j holds k = 8g+2j+h, the order
    the MFMA A/B operands consume 16-byte chunks in; the format's definition is kperm_k in csrc/match_exact.h).  Returns the rows in
    natural k order (tests / debugging only)."""
    Cp = x.shape[-1]
    pos = torch.arange(Cp, device=x.device)
    g, r = pos // 8, pos % 8
    k_at_pos = 8 * g + 2 * (r % 4) + r // 4
    out = torch.empty_like(x)
    out[..., k_at_pos] = x
    return out


@_on_tensor_device
def match(a_hat: torch.Tensor, q_hat: torch.Tensor, n_a: torch.Tensor, n_q: torch.Tensor, threshold: float):
    """a_hat [B,cap_a,Cp], q_hat [B,cap_q,Cp] -> (min_dist [B,cap_a] f32, argmin [B,cap_a] i32, valid [B,cap_a] u8)."""
    dev = _lib.require_gpu(a_hat.device)
    B, cap_a, Cp = a_hat.shape
    cap_q = q_hat.shape[1]
    assert q_hat.shape[0] == B and q_hat.shape[2] == Cp
    min_dist = torch.empty((B, cap_a), dtype=torch.float32, device=dev)
    argmin = torch.empty((B, cap_a), dtype=torch.int32, device=dev)
    valid = torch.empty((B, cap_a), dtype=torch.uint8, device=dev)
    wsb = lib().oryon_match_workspace_bytes(B, cap_a)
    ws = _lib.workspace(dev, wsb)
    check(lib().oryon_match_f32(ptr(a_hat), ptr(q_hat), B, Cp, cap_a, cap_q, ptr(n_a), ptr(n_q), float(threshold),
                                ptr(min_dist), ptr(argmin), ptr(valid), ptr(ws), wsb, stream_ptr(dev)), "oryon_match_f32")
    return min_dist, argmin, valid


@_on_tensor_device
def match_mutual(a_hat: torch.Tensor, q_hat: torch.Tensor, n_a: torch.Tensor, n_q: torch.Tensor, threshold: float):
    """Both directions of `match` from one scan (K1m): -> (min_dist [B,cap_a] f32, argmin [B,cap_a] i32, valid [B,cap_a] u8,
    rev_min_dist [B,cap_q] f32, rev_argmin [B,cap_q] i32, mutual [B,cap_a] u8).  The first three are `match(a_hat, q_hat, ...)`, the
    next two the first two of `match(q_hat, a_hat, n_q, n_a, ...)`, bit for bit; mutual = valid & (rev_argmin[argmin] == row)."""
    dev = _lib.require_gpu(a_hat.device)
    B, cap_a, Cp = a_hat.shape
    cap_q = q_hat.shape[1]
    assert q_hat.shape[0] == B and q_hat.shape[2] == Cp
    min_dist = torch.empty((B, cap_a), dtype=torch.float32, device=dev)
    argmin = torch.empty((B, cap_a), dtype=torch.int32, device=dev)
    valid = torch.empty((B, cap_a), dtype=torch.uint8, device=dev)
    rev_min_dist = torch.empty((B, cap_q), dtype=torch.float32, device=dev)
    rev_argmin = torch.empty((B, cap_q), dtype=torch.int32, device=dev)
    mutual = torch.empty((B, cap_a), dtype=torch.uint8, device=dev)
    wsb = lib().oryon_match_mutual_workspace_bytes(B, cap_a, cap_q)
    ws = _lib.workspace(dev, wsb)
    check(lib().oryon_match_mutual_f32(ptr(a_hat), ptr(q_hat), B, Cp, cap_a, cap_q, ptr(n_a), ptr(n_q), float(threshold), ptr(min_dist),
                                       ptr(argmin), ptr(valid), ptr(rev_min_dist), ptr(rev_argmin), ptr(mutual), ptr(ws), wsb,
                                       stream_ptr(dev)), "oryon_match_mutual_f32")
    return min_dist, argmin, valid, rev_min_dist, rev_argmin, mutual


@_on_tensor_device
def match_second(a_hat: torch.Tensor, q_hat: torch.Tensor, n_a: torch.Tensor, n_q: torch.Tensor, roi_q: torch.Tensor, W_q: int, radius: int,
                 min_dist: torch.Tensor, argmin: torch.Tensor, gate: Optional[torch.Tensor], ratio: float):
    """The ratio test with an exclusion disc (K1r): -> (second_dist [B,cap_a] f32, second_argmin [B,cap_a] i32, keep [B,cap_a] u8).
    second_* is the best query row at least `radius` pixels (integer L2, in a map W_q wide; roi_q [B,stride] i32 holds the query rows'
    linear pixel indices) away from the pixel of argmin's row; keep = gate & (min_dist <= ratio * second_dist), the product rounded
    to float32.  min_dist / argmin: `match` or `match_mutual` on the same operands; gate: their valid or mutual, None for all ones."""
    dev = _lib.require_gpu(a_hat.device)
    B, cap_a, Cp = a_hat.shape
    cap_q = q_hat.shape[1]
    assert q_hat.shape[0] == B and q_hat.shape[2] == Cp
    assert roi_q.dtype == torch.int32 and roi_q.dim() == 2 and roi_q.shape[0] == B
    assert min_dist.dtype == torch.float32 and argmin.dtype == torch.int32 and min_dist.shape == (B, cap_a) and argmin.shape == (B, cap_a)
    assert gate is None or (gate.dtype == torch.uint8 and gate.shape == (B, cap_a))
    second_dist = torch.empty((B, cap_a), dtype=torch.float32, device=dev)
    second_argmin = torch.empty((B, cap_a), dtype=torch.int32, device=dev)
    keep = torch.empty((B, cap_a), dtype=torch.uint8, device=dev)
    wsb = lib().oryon_match_second_workspace_bytes(B, cap_a)
    ws = _lib.workspace(dev, wsb)
    check(lib().oryon_match_second_f32(ptr(a_hat), ptr(q_hat), B, Cp, cap_a, cap_q, ptr(n_a), ptr(n_q), ptr(roi_q), roi_q.shape[1], int(W_q),
                                       int(radius), ptr(min_dist), ptr(argmin), ptr(gate), float(ratio), ptr(second_dist),
                                       ptr(second_argmin), ptr(keep), ptr(ws), wsb, stream_ptr(dev)), "oryon_match_second_f32")
    return second_dist, second_argmin, keep


@_on_tensor_device
def match_next(a_hat: torch.Tensor, q_hat: torch.Tensor, n_a: torch.Tensor, n_q: torch.Tensor, roi_q: torch.Tensor, W_q: int, radius: int,
               prev_argmin: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """One rank of the one-to-many matcher (K1n): -> (next_dist [B,cap_a] f32, next_argmin [B,cap_a] i32), the best query row outside
    the discs of `radius` pixels round the pixels of the earlier ranks prev_argmin [n_prev,B,cap_a] i32 (n_prev 1..3); index -1 and
    inf where no row is left.  out: the two tensors to write (e.g. the next plane of a [K,B,cap_a] table) instead of fresh ones."""
    dev = _lib.require_gpu(a_hat.device)
    B, cap_a, Cp = a_hat.shape
    cap_q = q_hat.shape[1]
    assert q_hat.shape[0] == B and q_hat.shape[2] == Cp
    assert a_hat.dtype == torch.float32 and q_hat.dtype == torch.float32
    assert roi_q.dtype == torch.int32 and roi_q.dim() == 2 and roi_q.shape[0] == B
    assert prev_argmin.dtype == torch.int32 and prev_argmin.dim() == 3 and prev_argmin.shape[1:] == (B, cap_a)
    if out is None:
        out = (torch.empty((B, cap_a), dtype=torch.float32, device=dev), torch.empty((B, cap_a), dtype=torch.int32, device=dev))
    next_dist, next_argmin = out
    assert next_dist.dtype == torch.float32 and next_argmin.dtype == torch.int32 and next_dist.shape == (B, cap_a) == next_argmin.shape
    wsb = lib().oryon_match_next_workspace_bytes(B, cap_a)
    ws = _lib.workspace(dev, wsb)
    check(lib().oryon_match_next_f32(ptr(a_hat), ptr(q_hat), B, Cp, cap_a, cap_q, ptr(n_a), ptr(n_q), ptr(roi_q), roi_q.shape[1], int(W_q),
                                     int(radius), ptr(prev_argmin), prev_argmin.shape[0], ptr(next_dist), ptr(next_argmin), ptr(ws), wsb,
                                     stream_ptr(dev)), "oryon_match_next_f32")
    return next_dist, next_argmin


@_on_tensor_device
def topk_corrs(a_hat: torch.Tensor, q_hat: torch.Tensor, roi_a: torch.Tensor, roi_q: torch.Tensor, n_a: torch.Tensor, n_q: torch.Tensor,
               min_dist: torch.Tensor, argmin: torch.Tensor, valid: torch.Tensor, threshold: float, W: int, max_corrs: int, seed: int,
               topk: int, radius: int, margin: float, pair_key=None, corr_rows: Optional[int] = None, tables: bool = False):
    """One-to-many correspondences (K1k): the draws of `select_corrs`, then up to `topk` rows per drawn anchor.
    -> dict(corrs [B,corr_rows,4] i32, rank [B,corr_rows] u8, n_valid, n_sel, status, n_rows [B] i32); corr_rows defaults to
    topk * max_corrs, rows >= n_rows stay zero.  tables (topk > 1): also sel_rows [B,cap_s] i32 and cand_dist f32 / cand_argmin i32
    [topk,B,cap_s], cap_s = round_up(max_corrs, 128), slots >= n_sel as allocated (NaN / -2)."""
    dev = _lib.require_gpu(a_hat.device)
    B, cap_a, Cp = a_hat.shape
    cap_q = q_hat.shape[1]
    K = int(topk)
    assert q_hat.shape[0] == B and q_hat.shape[2] == Cp and a_hat.dtype == torch.float32 and q_hat.dtype == torch.float32
    assert roi_a.dtype == torch.int32 and roi_q.dtype == torch.int32 and roi_a.dim() == 2 and roi_q.dim() == 2
    assert min_dist.dtype == torch.float32 and argmin.dtype == torch.int32 and valid.dtype == torch.uint8
    assert min_dist.shape == (B, cap_a) == argmin.shape == valid.shape
    corr_rows = int(corr_rows or K * int(max_corrs))
    cap_s = round_up(max_corrs, MATCH_TILE)
    out = dict(corrs=torch.zeros((B, corr_rows, 4), dtype=torch.int32, device=dev),
               rank=torch.zeros((B, corr_rows), dtype=torch.uint8, device=dev),
               n_valid=torch.empty((B,), dtype=torch.int32, device=dev), n_sel=torch.empty((B,), dtype=torch.int32, device=dev),
               status=torch.empty((B,), dtype=torch.int32, device=dev), n_rows=torch.empty((B,), dtype=torch.int32, device=dev))
    if tables and K > 1:
        out["sel_rows"] = torch.full((B, cap_s), -2, dtype=torch.int32, device=dev)
        out["cand_dist"] = torch.full((K, B, cap_s), float("nan"), dtype=torch.float32, device=dev)
        out["cand_argmin"] = torch.full((K, B, cap_s), -2, dtype=torch.int32, device=dev)
    wsb = lib().oryon_topk_corrs_workspace_bytes(B, Cp, cap_a, int(max_corrs), K)
    ws = _lib.workspace(dev, wsb, "oryon_topk_corrs_workspace_bytes")
    check(lib().oryon_topk_corrs(ptr(a_hat), ptr(q_hat), B, Cp, cap_a, cap_q, ptr(roi_a), ptr(roi_q), roi_a.shape[1], roi_q.shape[1],
                                 ptr(n_a), ptr(n_q), ptr(min_dist), ptr(argmin), ptr(valid), float(threshold), int(W), int(max_corrs),
                                 corr_rows, int(seed) & (2**64 - 1), ptr(pair_key), K, int(radius), float(margin), ptr(out["corrs"]),
                                 ptr(out["rank"]), ptr(out["n_valid"]), ptr(out["n_sel"]), ptr(out["status"]), ptr(out["n_rows"]),
                                 ptr(out.get("sel_rows")), ptr(out.get("cand_dist")), ptr(out.get("cand_argmin")), ptr(ws), wsb,
                                 stream_ptr(dev)), "oryon_topk_corrs")
    return out


@_on_tensor_device
def match_screened(a_hat, q_hat, a16, q16, n_a, n_q, threshold: float):
    """fp16-screened, fp32-exact matcher (K1s).  Same outputs as `match` on every row that can be valid."""
    dev = _lib.require_gpu(a_hat.device)
    B, cap_a, Cp = a_hat.shape
    cap_q = q_hat.shape[1]
    assert a16.dtype == torch.float16 and q16.dtype == torch.float16 and a16.shape == a_hat.shape and q16.shape == q_hat.shape
    min_dist = torch.empty((B, cap_a), dtype=torch.float32, device=dev)
    argmin = torch.empty((B, cap_a), dtype=torch.int32, device=dev)
    valid = torch.empty((B, cap_a), dtype=torch.uint8, device=dev)
    wsb = lib().oryon_match_screened_workspace_bytes(B, Cp, cap_a)
    ws = _lib.workspace(dev, wsb)
    check(lib().oryon_match_screened(ptr(a_hat), ptr(q_hat), ptr(a16), ptr(q16), B, Cp, cap_a, cap_q, ptr(n_a), ptr(n_q),
                                     float(threshold), ptr(min_dist), ptr(argmin), ptr(valid), ptr(ws), wsb, stream_ptr(dev)),
          "oryon_match_screened")
    return min_dist, argmin, valid


@_on_tensor_device
def gather_normalise_q8(feat: torch.Tensor, roi: torch.Tensor, count: torch.Tensor, rows_cap: int, c_pad: int, want_f16: bool = False):
    """K0 with int8 copies: -> (rows fp32 k-permuted, rows fp16 | None, rows int8, slice_scale [n, rows_cap/16], eps_max [n])."""
    dev = _lib.require_gpu(feat.device)
    feat = feat.to(torch.float32).contiguous()
    n_maps, C, H, W = feat.shape
    assert c_pad in (256, 512) and C <= c_pad and rows_cap % ROW_PAD == 0
    out = torch.empty((n_maps, rows_cap, c_pad), dtype=torch.float32, device=dev)
    out16 = torch.empty((n_maps, rows_cap, c_pad), dtype=torch.float16, device=dev) if want_f16 else None
    out8 = torch.empty((n_maps, rows_cap, c_pad), dtype=torch.int8, device=dev)
    scale = torch.ones((n_maps, rows_cap // 16), dtype=torch.float32, device=dev)
    eps = torch.empty((n_maps,), dtype=torch.float32, device=dev)
    check(lib().oryon_gather_normalise_q8(ptr(feat), n_maps, C, H * W, ptr(roi), roi.shape[1], ptr(count), rows_cap, c_pad, ptr(out),
                                          ptr(out16), ptr(out8), ptr(scale), ptr(eps), stream_ptr(dev)), "oryon_gather_normalise_q8")
    return out, out16, out8, scale, eps


LAYOUT_NCHW, LAYOUT_NHWC = 0, 1


def map_layout(feat: torch.Tensor):
    """(tensor whose storage the C ABI can read, layout code) for a logical [n,C,H,W] descriptor map: contiguous -> NCHW,
    torch.channels_last -> NHWC (zero-copy), anything else is made contiguous first."""
    if feat.is_contiguous():
        return feat, LAYOUT_NCHW
    if feat.dim() == 4 and feat.is_contiguous(memory_format=torch.channels_last):
        return feat, LAYOUT_NHWC
    return feat.contiguous(), LAYOUT_NCHW


@_on_tensor_device
def gather_q8(feat: torch.Tensor, roi: torch.Tensor, count: torch.Tensor, rows_cap: int, c_pad: int, want_f32: bool = False,
              round_f16: bool = False):
    """K0v3 (gather8.hip): ROI rows of [n,C,H,W] fp32 maps (contiguous or channels_last) -> (rows int8 [n,rows_cap,c_pad],
    slice_scale [n,rows_cap/16], eps_max [n], row_norm [n,rows_cap], rows fp32 k-permuted [n,rows_cap,c_pad] | None)."""
    dev = _lib.require_gpu(feat.device)
    assert feat.dtype == torch.float32 and feat.dim() == 4
    feat, layout = map_layout(feat)
    n_maps, C, H, W = feat.shape
    assert c_pad in (256, 512) and C <= c_pad and rows_cap % ROW_PAD == 0
    out8 = torch.empty((n_maps, rows_cap, c_pad), dtype=torch.int8, device=dev)
    scale = torch.empty((n_maps, rows_cap // 16), dtype=torch.float32, device=dev)
    eps = torch.empty((n_maps,), dtype=torch.float32, device=dev)
    norm = torch.empty((n_maps, rows_cap), dtype=torch.float32, device=dev)
    out32 = torch.empty((n_maps, rows_cap, c_pad), dtype=torch.float32, device=dev) if want_f32 else None
    check(lib().oryon_gather_q8(feat.data_ptr(), n_maps, C, H * W, layout, ptr(roi), roi.shape[1], ptr(count), rows_cap, c_pad, ptr(out8),
                                ptr(scale), ptr(eps), ptr(norm), ptr(out32), int(bool(round_f16)), stream_ptr(dev)), "oryon_gather_q8")
    return out8, scale, eps, norm, out32


@_on_tensor_device
def gather_mx6(feat: torch.Tensor, roi: torch.Tensor, count: torch.Tensor, rows_cap: int, c_pad: int, want_f32: bool = False,
               round_f16: bool = False):
    """K0 with MX-fp6 screening operands (oryon_gather_mx6): -> (rows uint8 [n,rows_cap,c_pad] of 32-byte slots, err_max [n] fp32,
    row_norm [n,rows_cap], rows fp32 k-permuted | None)."""
    dev = _lib.require_gpu(feat.device)
    assert feat.dtype == torch.float32 and feat.dim() == 4
    feat, layout = map_layout(feat)
    n_maps, C, H, W = feat.shape
    assert c_pad in (256, 512) and C <= c_pad and rows_cap % ROW_PAD == 0
    out6 = torch.empty((n_maps, rows_cap, c_pad), dtype=torch.uint8, device=dev)
    err = torch.empty((n_maps,), dtype=torch.float32, device=dev)
    norm = torch.empty((n_maps, rows_cap), dtype=torch.float32, device=dev)
    out32 = torch.empty((n_maps, rows_cap, c_pad), dtype=torch.float32, device=dev) if want_f32 else None
    check(lib().oryon_gather_mx6(feat.data_ptr(), n_maps, C, H * W, layout, ptr(roi), roi.shape[1], ptr(count), rows_cap, c_pad, ptr(out6),
                                 ptr(err), ptr(norm), ptr(out32), int(bool(round_f16)), stream_ptr(dev)), "oryon_gather_mx6")
    return out6, err, norm, out32


import threading

_raw_ws = {}                      # (device, stream) -> cached matcher workspace (holds room for the rarely used fp32 fall-back rows)
_raw_ws_lock = threading.Lock()   # the C entry points issue ~15 dependent launches on the workspace and ctypes releases the GIL: two host
                                  # threads that launch on ONE stream must not interleave their sequences on the shared buffer


def release_workspaces() -> None:
    """Drop the cached matcher workspaces (they pin the largest size ever requested per (device, stream) for the life of the process)."""
    with _raw_ws_lock:
        _raw_ws.clear()


def _cached_raw_ws(dev, wsb: int):
    """The cached workspace of the current stream, grown to wsb bytes.  Call with _raw_ws_lock held, and keep it until the launches
    that use the buffer are issued."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _raw_ws.get(key)
    if ws is None or ws.numel() < wsb:
        ws = _raw_ws[key] = _lib.workspace(dev, wsb)
    return ws


def _match_corrs(entry: str, a_hat, feat_a, a_norm, a_rows, a_aux, feat_q, roi_a, roi_q, q_norm, q_rows, q_aux, n_a, n_q, threshold, W,
                 max_corrs, seed, pair_key, corr_rows, n_undecided, round_f16, force_eager=None, cached_ws=False):
    """Every oryon_match_corrs_* entry: allocates the outputs and makes the call.  The entries share everything but the operand block
    between feat_q's geometry and B and the leading anchor rows: a_hat, or (a_hat None) feat_a + a_norm for the `_araw` entries;
    a_aux / q_aux are the pointer arguments that follow a_rows / q_rows in the C signature (include/oryon_hip.h).  force_eager: the
    argument only oryon_match_corrs_i8 has (None: the entry has none).  cached_ws: the per-stream workspace under _raw_ws_lock
    instead of a fresh allocation."""
    dev = _lib.require_gpu(a_rows.device)
    feat_q, layout = map_layout(feat_q)
    if a_hat is None:
        feat_a, layout_a = map_layout(feat_a)
        assert layout_a == layout and feat_a.shape[1:] == feat_q.shape[1:], "anchor and query maps share C, H, W and the memory layout"
        lead = (feat_a.data_ptr(), ptr(a_norm))
    else:
        lead = (ptr(a_hat),)
    B, cap_a, Cp = a_rows.shape
    cap_q = q_rows.shape[1]
    C_true, HW = feat_q.shape[1], feat_q.shape[2] * feat_q.shape[3]
    corr_rows = int(corr_rows or max_corrs)
    min_dist = torch.empty((B, cap_a), dtype=torch.float32, device=dev)
    argmin = torch.empty((B, cap_a), dtype=torch.int32, device=dev)
    valid = torch.empty((B, cap_a), dtype=torch.uint8, device=dev)
    corrs = torch.zeros((B, corr_rows, 4), dtype=torch.int32, device=dev)
    n_valid = torch.empty((B,), dtype=torch.int32, device=dev)
    n_sel = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    wsb = lib().oryon_match_corrs_i8_workspace_bytes(B, Cp, cap_a, cap_q, corr_rows)
    eager = () if force_eager is None else (int(bool(force_eager)),)

    def call(ws):
        check(getattr(lib(), entry)(*lead, ptr(a_rows), *[ptr(t) for t in a_aux], feat_q.data_ptr(), C_true, HW, layout, ptr(roi_a),
                                    roi_a.shape[1], ptr(roi_q), roi_q.shape[1], ptr(q_norm), ptr(q_rows), *[ptr(t) for t in q_aux], B, Cp,
                                    cap_a, cap_q, ptr(n_a), ptr(n_q), float(threshold), int(W), int(max_corrs), corr_rows,
                                    int(seed) & (2**64 - 1), ptr(pair_key), *eager, ptr(min_dist), ptr(argmin), ptr(valid), ptr(corrs),
                                    ptr(n_valid), ptr(n_sel), ptr(status), ptr(n_undecided), int(bool(round_f16)), ptr(ws), ws.numel(),
                                    stream_ptr(dev)), entry)

    if cached_ws:
        with _raw_ws_lock:
            call(_cached_raw_ws(dev, wsb))
    else:
        call(_lib.workspace(dev, wsb))
    return corrs, n_valid, n_sel, status, min_dist, argmin, valid


@_on_tensor_device
def match_corrs_mx6(a_hat, a6, a_err, feat_q, roi_a, roi_q, q_norm, q6, q_err, n_a, n_q, threshold: float, W: int, max_corrs: int,
                    seed: int, pair_key=None, corr_rows: Optional[int] = None, n_undecided=None, round_f16: bool = False):
    """oryon_match_corrs_mx6: the lazy matcher + sampler on MX-fp6 operands; same outputs as match_corrs_i8."""
    return _match_corrs("oryon_match_corrs_mx6", a_hat, None, None, a6, (a_err,), feat_q, roi_a, roi_q, q_norm, q6, (q_err,), n_a, n_q,
                        threshold, W, max_corrs, seed, pair_key, corr_rows, n_undecided, round_f16)


@_on_tensor_device
def match_screened8_raw(a_hat, a8, a_scale, feat_q, roi_q, q_norm, q8, q_scale, q_eps, n_a, n_q, threshold: float, n_undecided=None,
                        round_f16: bool = False):
    """K1s8 on K0v3 operands: no fp32 copy of the query rows exists; the exact re-scoring reads candidates from the raw map feat_q
    ([B,C,H,W] contiguous or channels_last).  Same outputs as `match_screened8`."""
    dev = _lib.require_gpu(a_hat.device)
    feat_q, layout = map_layout(feat_q)
    B, cap_a, Cp = a_hat.shape
    cap_q = q8.shape[1]
    C_true, HW = feat_q.shape[1], feat_q.shape[2] * feat_q.shape[3]
    min_dist = torch.empty((B, cap_a), dtype=torch.float32, device=dev)
    argmin = torch.empty((B, cap_a), dtype=torch.int32, device=dev)
    valid = torch.empty((B, cap_a), dtype=torch.uint8, device=dev)
    wsb = lib().oryon_match_screened8_raw_workspace_bytes(B, Cp, cap_a, cap_q)
    # the workspace holds room for the (rarely used) fp32 fall-back rows of every pair: cached per (device, stream) instead of
    # being re-requested from the allocator on every call
    with _raw_ws_lock:
        ws = _cached_raw_ws(dev, wsb)
        check(lib().oryon_match_screened8_raw(ptr(a_hat), ptr(a8), ptr(a_scale), feat_q.data_ptr(), C_true, HW, layout, ptr(roi_q),
                                              roi_q.shape[1], ptr(q_norm), ptr(q8), ptr(q_scale), ptr(q_eps), B, Cp, cap_a, cap_q, ptr(n_a),
                                              ptr(n_q), float(threshold), ptr(min_dist), ptr(argmin), ptr(valid), ptr(n_undecided),
                                              int(bool(round_f16)), ptr(ws), ws.numel(), stream_ptr(dev)), "oryon_match_screened8_raw")
    return min_dist, argmin, valid


@_on_tensor_device
def match_corrs_i8(a_hat, a8, a_scale, feat_q, roi_a, roi_q, q_norm, q8, q_scale, q_eps, n_a, n_q, threshold: float, W: int, max_corrs: int,
                   seed: int, pair_key=None, corr_rows: Optional[int] = None, force_eager: bool = False, n_undecided=None,
                   round_f16: bool = False):
    """Lazy K1s8 + K1b (oryon_match_corrs_i8): -> (corrs [B,corr_rows,4] i32, n_valid [B], n_sel [B], status [B], min_dist, argmin, valid).
    Same correspondences as select_corrs(match_screened8_raw(...)); min_dist / argmin are exact only on sampled rows unless force_eager."""
    return _match_corrs("oryon_match_corrs_i8", a_hat, None, None, a8, (a_scale,), feat_q, roi_a, roi_q, q_norm, q8, (q_scale, q_eps), n_a, n_q,
                        threshold, W, max_corrs, seed, pair_key, corr_rows, n_undecided, round_f16, force_eager=force_eager, cached_ws=True)


@_on_tensor_device
def match_corrs_i8_araw(feat_a, a_norm, a8, a_scale, feat_q, roi_a, roi_q, q_norm, q8, q_scale, q_eps, n_a, n_q, threshold: float, W: int,
                        max_corrs: int, seed: int, pair_key=None, corr_rows: Optional[int] = None, n_undecided=None, round_f16: bool = False):
    """oryon_match_corrs_i8_araw: match_corrs_i8 (lazy route) without materialised fp32 anchor rows - the raw anchor map and K0's anchor
    norms instead of a_hat; same outputs, bit for bit."""
    return _match_corrs("oryon_match_corrs_i8_araw", None, feat_a, a_norm, a8, (a_scale,), feat_q, roi_a, roi_q, q_norm, q8, (q_scale, q_eps),
                        n_a, n_q, threshold, W, max_corrs, seed, pair_key, corr_rows, n_undecided, round_f16)


@_on_tensor_device
def match_corrs_mx6_araw(feat_a, a_norm, a6, a_err, feat_q, roi_a, roi_q, q_norm, q6, q_err, n_a, n_q, threshold: float, W: int, max_corrs: int,
                         seed: int, pair_key=None, corr_rows: Optional[int] = None, n_undecided=None, round_f16: bool = False):
    """oryon_match_corrs_mx6_araw: match_corrs_mx6 without materialised fp32 anchor rows; same outputs, bit for bit."""
    return _match_corrs("oryon_match_corrs_mx6_araw", None, feat_a, a_norm, a6, (a_err,), feat_q, roi_a, roi_q, q_norm, q6, (q_err,), n_a, n_q,
                        threshold, W, max_corrs, seed, pair_key, corr_rows, n_undecided, round_f16)


@_on_tensor_device
def match_corrs_mx6_x3_araw(feat_a, a_norm, a6, a_err, feat_q, roi_a, roi_q, q_norm, q6, q_err, q_hi_lo, q_lo_max, n_a, n_q, threshold: float,
                            W: int, max_corrs: int, seed: int, pair_key=None, corr_rows: Optional[int] = None, n_undecided=None,
                            round_f16: bool = False):
    """oryon_match_corrs_mx6_x3_araw: the matcher on K0's hi / lo query rows (oryon_gather_mx6_x3) without materialised fp32 anchor rows."""
    return _match_corrs("oryon_match_corrs_mx6_x3_araw", None, feat_a, a_norm, a6, (a_err,), feat_q, roi_a, roi_q, q_norm, q6,
                        (q_err, q_hi_lo, q_lo_max), n_a, n_q, threshold, W, max_corrs, seed, pair_key, corr_rows, n_undecided, round_f16)


@_on_tensor_device
def match_screened8(a_hat, q_hat, a8, q8, a_scale, q_scale, q_eps, n_a, n_q, threshold: float, c_true: int, n_undecided=None):
    """int8 pre-screen + fp16 screen + exact fp32 re-scoring (K1s8).  Same outputs as `match_screened`.
    n_undecided: optional int32 [B] tensor receiving the number of anchors the int8 stage handed to the fp16 stage."""
    dev = _lib.require_gpu(a_hat.device)
    B, cap_a, Cp = a_hat.shape
    cap_q = q_hat.shape[1]
    min_dist = torch.empty((B, cap_a), dtype=torch.float32, device=dev)
    argmin = torch.empty((B, cap_a), dtype=torch.int32, device=dev)
    valid = torch.empty((B, cap_a), dtype=torch.uint8, device=dev)
    wsb = lib().oryon_match_screened8_workspace_bytes(B, Cp, cap_a, cap_q)
    ws = _lib.workspace(dev, wsb)
    check(lib().oryon_match_screened8(ptr(a_hat), ptr(q_hat), ptr(a8), ptr(q8), ptr(a_scale), ptr(q_scale), ptr(q_eps),
                                      B, int(c_true), Cp, cap_a, cap_q, ptr(n_a), ptr(n_q), float(threshold), ptr(min_dist), ptr(argmin),
                                      ptr(valid), ptr(n_undecided), ptr(ws), wsb, stream_ptr(dev)), "oryon_match_screened8")
    return min_dist, argmin, valid


@_on_tensor_device
def select_corrs(roi_a, roi_q, n_a, n_q, argmin, valid, W: int, max_corrs: int, seed: int, pair_key=None,
                 corr_rows: Optional[int] = None):
    """Device-RNG correspondence sampling -> (corrs [B,corr_rows,4] i32, n_valid [B], n_sel [B], status [B])."""
    dev = _lib.require_gpu(roi_a.device)
    B, cap_a = argmin.shape
    corr_rows = int(corr_rows or max_corrs)
    corrs = torch.zeros((B, corr_rows, 4), dtype=torch.int32, device=dev)
    n_valid = torch.empty((B,), dtype=torch.int32, device=dev)
    n_sel = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    scratch = torch.empty((B, cap_a), dtype=torch.int32, device=dev)
    check(lib().oryon_select_corrs(ptr(roi_a), ptr(roi_q), roi_a.shape[1], roi_q.shape[1], ptr(n_a), ptr(n_q), ptr(argmin),
                                   ptr(valid), cap_a, B, int(W), int(max_corrs), corr_rows, int(seed) & (2**64 - 1),
                                   ptr(pair_key), ptr(scratch), ptr(corrs), ptr(n_valid), ptr(n_sel), ptr(status),
                                   stream_ptr(dev)), "oryon_select_corrs")
    return corrs, n_valid, n_sel, status


@_on_tensor_device
def lift_pairs(corrs: torch.Tensor, n_corr: Optional[torch.Tensor], feat_hw, depth_a: torch.Tensor, depth_q: torch.Tensor,
               cam_a: torch.Tensor, cam_q: torch.Tensor, status: Optional[torch.Tensor] = None):
    """corrs [B,n_cap,4] i32, depth_* [B,H,W] f32 (mm), cam_* [B,9] f32 -> (pcd_a, pcd_q [B,n_cap,3] metres, n_out [B])."""
    dev = _lib.require_gpu(corrs.device)
    B, n_cap = corrs.shape[0], corrs.shape[1]
    assert corrs.dtype == torch.int32 and depth_a.dtype == torch.float32 and depth_q.dtype == torch.float32
    assert cam_a.dtype == torch.float32 and cam_a.shape == (B, 9) and cam_q.shape == (B, 9)
    pa = torch.empty((B, n_cap, 3), dtype=torch.float32, device=dev)      # the kernel zeroes the rows past the lifted count
    pq = torch.empty((B, n_cap, 3), dtype=torch.float32, device=dev)
    n_out = torch.empty((B,), dtype=torch.int32, device=dev)
    check(lib().oryon_lift_pairs(ptr(corrs), ptr(n_corr), B, n_cap, int(feat_hw[0]), int(feat_hw[1]),
                                 ptr(depth_a.contiguous()), depth_a.shape[1], depth_a.shape[2],
                                 ptr(depth_q.contiguous()), depth_q.shape[1], depth_q.shape[2],
                                 ptr(cam_a.contiguous()), ptr(cam_q.contiguous()), ptr(status), ptr(pa), ptr(pq), ptr(n_out),
                                 stream_ptr(dev)), "oryon_lift_pairs")
    return pa, pq, n_out


SUBPIX_FLAGS = ("refined", "border", "flat", "outside")      # the flag values 0..3 of oryon_subpix_refine, the order of counts[..., f]


@_on_tensor_device
def subpix_refine(feat_a: torch.Tensor, feat_q: torch.Tensor, corrs: torch.Tensor, n_corr: Optional[torch.Tensor] = None,
                  status: Optional[torch.Tensor] = None, curv_min: float = 1e-4):
    """Sub-pixel refinement of selected correspondences (csrc/match_subpix.hip; definition: include/oryon_hip.h, oryon_subpix_refine).
    feat_* [B,C,FH,FW] fp32 (contiguous or channels_last, both of one layout), corrs [B,n_cap,4] i32, n_corr / status [B] i32 or None
    -> dict(offsets [B,n_cap,2] fp32 (dy, dx), flags [B,n_cap] uint8, counts [B,4] i32 in the order of SUBPIX_FLAGS)."""
    dev = _lib.require_gpu(feat_a.device)
    assert feat_a.dtype == torch.float32 and feat_q.dtype == torch.float32 and feat_a.dim() == 4 and feat_a.shape == feat_q.shape
    assert corrs.dtype == torch.int32 and corrs.dim() == 3 and corrs.shape[0] == feat_a.shape[0] and corrs.shape[2] == 4
    feat_a, layout = map_layout(feat_a)
    feat_q, layout_q = map_layout(feat_q)
    if layout_q != layout:                       # one layout argument: the odd one out is copied
        feat_a, feat_q, layout = feat_a.contiguous(), feat_q.contiguous(), LAYOUT_NCHW
    B, C, FH, FW = feat_a.shape
    n_cap = corrs.shape[1]
    offsets = torch.empty((B, n_cap, 2), dtype=torch.float32, device=dev)      # the kernel writes every row
    flags = torch.empty((B, n_cap), dtype=torch.uint8, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    check(lib().oryon_subpix_refine(feat_a.data_ptr(), feat_q.data_ptr(), B, C, FH, FW, layout, ptr(corrs), ptr(n_corr), ptr(status), n_cap,
                                    float(curv_min), ptr(offsets), ptr(flags), ptr(counts), stream_ptr(dev)), "oryon_subpix_refine")
    return dict(offsets=offsets, flags=flags, counts=counts)


@_on_tensor_device
def lift_pairs_subpix(corrs: torch.Tensor, n_corr: Optional[torch.Tensor], feat_hw, depth_a: torch.Tensor, depth_q: torch.Tensor,
                      cam_a: torch.Tensor, cam_q: torch.Tensor, status: Optional[torch.Tensor] = None,
                      offsets: Optional[torch.Tensor] = None, depth_jump: float = 0.02):
    """lift_pairs on refined query coordinates (oryon_lift_pairs_subpix): offsets [B,n_cap,2] fp32 (dy, dx; None = zeros), depth_jump
    in metres (the four depths under a bilinear read may differ by no more) -> (pcd_a, pcd_q [B,n_cap,3] metres, n_out [B])."""
    dev = _lib.require_gpu(corrs.device)
    B, n_cap = corrs.shape[0], corrs.shape[1]
    assert corrs.dtype == torch.int32 and depth_a.dtype == torch.float32 and depth_q.dtype == torch.float32
    assert cam_a.dtype == torch.float32 and cam_a.shape == (B, 9) and cam_q.shape == (B, 9)
    assert offsets is None or (offsets.dtype == torch.float32 and tuple(offsets.shape) == (B, n_cap, 2))
    pa = torch.empty((B, n_cap, 3), dtype=torch.float32, device=dev)      # the kernel zeroes the rows past the lifted count
    pq = torch.empty((B, n_cap, 3), dtype=torch.float32, device=dev)
    n_out = torch.empty((B,), dtype=torch.int32, device=dev)
    check(lib().oryon_lift_pairs_subpix(ptr(corrs), ptr(offsets), ptr(n_corr), B, n_cap, int(feat_hw[0]), int(feat_hw[1]),
                                        ptr(depth_a.contiguous()), depth_a.shape[1], depth_a.shape[2],
                                        ptr(depth_q.contiguous()), depth_q.shape[1], depth_q.shape[2],
                                        ptr(cam_a.contiguous()), ptr(cam_q.contiguous()), ptr(status), float(depth_jump) * 1000.0,
                                        ptr(pa), ptr(pq), ptr(n_out), stream_ptr(dev)), "oryon_lift_pairs_subpix")
    return pa, pq, n_out


@_on_tensor_device
def lift_points(depth: torch.Tensor, cam9: torch.Tensor, x_idx: torch.Tensor, y_idx: torch.Tensor) -> torch.Tensor:
    """depth [H,W] f32, cam9 [9] f32, pixel indices [n] -> [n,3] f32 in the depth's unit."""
    dev = _lib.require_gpu(depth.device)
    n = x_idx.shape[0]
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if n == 0:                                   # empty tensors have no storage: the C entry refuses their NULL pointers
        return out
    xi = x_idx.to(torch.int32).contiguous()
    yi = y_idx.to(torch.int32).contiguous()
    check(lib().oryon_lift_points(ptr(depth), depth.shape[0], depth.shape[1], ptr(cam9.contiguous()), ptr(xi), ptr(yi), n,
                                  ptr(out), stream_ptr(dev)), "oryon_lift_points")
    return out


@_on_tensor_device
def kabsch_batched(A: torch.Tensor, B: torch.Tensor, w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[nb,m,3] x2 (+ [nb,m]) fp32 -> [nb,4,4] fp32."""
    dev = _lib.require_gpu(A.device)
    A = A.to(torch.float32).contiguous()
    B = B.to(torch.float32).contiguous()
    w = None if w is None else w.to(torch.float32).contiguous()
    nb, m = A.shape[0], A.shape[1]
    T = torch.empty((nb, 4, 4), dtype=torch.float32, device=dev)
    check(lib().oryon_kabsch_batched(ptr(A), ptr(B), ptr(w), nb, m, ptr(T), stream_ptr(dev)), "oryon_kabsch_batched")
    return T


@_on_tensor_device
def ransac_register(src: torch.Tensor, tgt: torch.Tensor, n: torch.Tensor, max_iter: int = 10000, match_err: float = 0.001,
                    fix_percent: float = 0.9999, sample_idx: Optional[torch.Tensor] = None, seed: int = 1,
                    pair_key: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None, want_counts: bool = False,
                    workspace: Optional[torch.Tensor] = None):
    """src, tgt [B,n_cap,3] fp32 (metres, n_cap <= 2048), n [B] int32 -> dict(T [B,4,4], winner [B], exited [B], status [B],
    counts [B,max_iter] | None).  sample_idx [B,max_iter,4] int32 names the rows of every draw; None = the device RNG keyed by
    (seed, pair_key).  Hypothesis numbering and the zero / identity results: include/oryon_hip.h, oryon_ransac_register."""
    dev = _lib.require_gpu(src.device)
    assert src.dtype == torch.float32 and tgt.dtype == torch.float32 and src.shape == tgt.shape and src.shape[2] == 3
    assert n.dtype == torch.int32 and (status is None or status.dtype == torch.int32) and (pair_key is None or pair_key.dtype == torch.int64)
    B, n_cap = src.shape[0], src.shape[1]
    max_iter = int(max_iter)
    if sample_idx is not None:
        assert sample_idx.dtype == torch.int32 and tuple(sample_idx.shape) == (B, max_iter, 4)
    ws = _lib.workspace(dev, lib().oryon_ransac_workspace_bytes(B, n_cap, max_iter),
                        f"oryon_ransac_workspace_bytes({B}, {n_cap}, {max_iter})" if B > 0 else None, workspace,
                        "shape not supported (n_cap <= 2048, max_iter > 0)")
    T = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    winner = torch.empty((B,), dtype=torch.int32, device=dev)
    exited = torch.empty((B,), dtype=torch.int32, device=dev)
    st_out = torch.empty((B,), dtype=torch.int32, device=dev)
    counts = torch.empty((B, max_iter), dtype=torch.int32, device=dev) if want_counts else None
    check(lib().oryon_ransac_register(ptr(src), ptr(tgt), ptr(n), B, n_cap, max_iter, float(match_err), float(fix_percent), ptr(sample_idx),
                                      int(seed) & (2**64 - 1), ptr(pair_key), ptr(status), ptr(ws), ws.numel(), ptr(T), ptr(winner),
                                      ptr(exited), ptr(counts), ptr(st_out), stream_ptr(dev)), "oryon_ransac_register")
    return dict(T=T, winner=winner, exited=exited, status=st_out, counts=counts)


# oryon_spectral_config_t's defaults: object-scale (metres), chosen from one synthetic experiment, not from real data (csrc/spectral.hip)
SPECTRAL_DEFAULTS = dict(num_iterations=10, ratio=0.1, inlier_threshold=0.01, sigma_d=0.01, k=40, nms_radius=0.02)


def spectral_config(**cfg) -> "_lib.SpectralConfig":
    unknown = set(cfg) - set(SPECTRAL_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown spectral solver option(s): {sorted(unknown)}")
    c = dict(SPECTRAL_DEFAULTS, **cfg)
    return _lib.SpectralConfig(num_iterations=int(c["num_iterations"]), ratio=float(c["ratio"]), inlier_threshold=float(c["inlier_threshold"]),
                               sigma_d=float(c["sigma_d"]), k=int(c["k"]), nms_radius=float(c["nms_radius"]))


def _spectral_args(src, tgt, n, status, workspace, cfg):
    dev = _lib.require_gpu(src.device)
    assert src.dtype == torch.float32 and tgt.dtype == torch.float32 and src.shape == tgt.shape and src.dim() == 3 and src.shape[2] == 3
    assert n.dtype == torch.int32 and (status is None or status.dtype == torch.int32)
    B, n_cap = src.shape[0], src.shape[1]
    c = spectral_config(**cfg)
    ws = _lib.workspace(dev, lib().oryon_spectral_workspace_bytes(ctypes.byref(c), B, n_cap),
                        f"oryon_spectral_workspace_bytes(B={B}, n_cap={n_cap})" if B > 0 else None, workspace,
                        "shape or configuration not supported (n_cap % 128 == 0, n_cap <= 2048, 2 <= k <= 63, 1 <= num_iterations <= 16)")
    return dev, B, n_cap, c, ws


@_on_tensor_device
def spectral_register(src: torch.Tensor, tgt: torch.Tensor, n: torch.Tensor, status: Optional[torch.Tensor] = None,
                      want_labels: bool = False, workspace: Optional[torch.Tensor] = None, **cfg):
    """src, tgt [B,n_cap,3] fp32 (metres; n_cap a multiple of 128, <= 2048), n [B] int32 -> dict(T [B,4,4], status [B],
    labels [B,n_cap] uint8 | None).  cfg: the fields of oryon_spectral_config_t (SPECTRAL_DEFAULTS).  No weights, no random numbers;
    definition: csrc/spectral.hip."""
    dev, B, n_cap, c, ws = _spectral_args(src, tgt, n, status, workspace, cfg)
    T = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    st_out = torch.empty((B,), dtype=torch.int32, device=dev)
    labels = torch.empty((B, n_cap), dtype=torch.uint8, device=dev) if want_labels else None
    check(lib().oryon_spectral_register(ctypes.byref(c), ptr(src), ptr(tgt), ptr(n), B, n_cap, ptr(status), ptr(ws), ws.numel(), ptr(T),
                                        ptr(labels), ptr(st_out), stream_ptr(dev)), "oryon_spectral_register")
    return dict(T=T, status=st_out, labels=labels)


SPECTRAL_STAGES = ("compat", "conf", "seeds", "n_seeds", "sets", "scores", "Mmat", "close", "seed_T", "fitness", "best", "T0", "T", "status")


@_on_tensor_device
def spectral_stages(src: torch.Tensor, tgt: torch.Tensor, n: torch.Tensor, status: Optional[torch.Tensor] = None,
                    out: Optional[dict] = None, workspace: Optional[torch.Tensor] = None, **cfg):
    """oryon_spectral_stages: the kernels of spectral_register with every intermediate returned (shapes: include/oryon_hip.h).
    out: name -> caller's buffer for any of SPECTRAL_STAGES (contiguous, the stage's dtype and shape); the rest are allocated."""
    dev, B, n_cap, c, ws = _spectral_args(src, tgt, n, status, workspace, cfg)
    S_cap, k, nit = int(float(n_cap) * float(c.ratio)) + 1, c.k, c.num_iterations
    i32, f32 = torch.int32, torch.float32
    spec = dict(compat=(i32, (B, n_cap, n_cap // 32)), conf=(f32, (B, n_cap)), seeds=(i32, (B, S_cap)), n_seeds=(i32, (B,)),
                sets=(i32, (B, S_cap, k)), scores=(i32, (B, S_cap, n_cap)), Mmat=(f32, (B, S_cap, k, k)), close=(i32, (B, S_cap, nit)),
                seed_T=(f32, (B, S_cap, 4, 4)), fitness=(f32, (B, S_cap)), best=(i32, (B,)), T0=(f32, (B, 4, 4)), T=(f32, (B, 4, 4)),
                status=(i32, (B,)))
    r = {}
    for name, (dt, shape) in spec.items():
        t = (out or {}).get(name)
        if t is None:
            t = torch.empty(shape, dtype=dt, device=dev)
        assert t.dtype == dt and tuple(t.shape) == shape, name
        r[name] = t
    check(lib().oryon_spectral_stages(ctypes.byref(c), ptr(src), ptr(tgt), ptr(n), B, n_cap, ptr(status), ptr(ws), ws.numel(),
                                      *(ptr(r[k_]) for k_ in SPECTRAL_STAGES), stream_ptr(dev)), "oryon_spectral_stages")
    return r


@_on_tensor_device
def feature_loss(feat_a: torch.Tensor, feat_q: torch.Tensor, corrs: torch.Tensor, valid: torch.Tensor, pool: Optional[torch.Tensor] = None,
                 pos_margin: float = 0.2, neg_margin: float = 0.9, neg_kernel: float = 5.0, pool_per_positive: bool = False,
                 workspace: Optional[torch.Tensor] = None):
    """feat_a, feat_q [B,C,FH,FW] fp32, corrs [B,N,4] int32 feature-map pixels (y_a,x_a,y_q,x_q), valid [B] int32 ->
    dict(d_pos [B,N], d_neg [B,2,N], neg_idx [B,2,N] int32 linear pixels, pair_terms [B,3], losses [3] = pos, neg_a, neg_q).
    pool [B,2,n_pool] int32 linear pixels: the candidates of the hardest-negative search (None = the whole map, row-major), or with
    pool_per_positive the negative of every positive itself ([B,2,N]).  Definition: include/oryon_hip.h, oryon_feature_loss."""
    dev = _lib.require_gpu(feat_a.device)
    assert feat_a.dtype == torch.float32 and feat_q.dtype == torch.float32 and feat_a.shape == feat_q.shape and feat_a.dim() == 4
    assert corrs.dtype == torch.int32 and corrs.dim() == 3 and corrs.shape[2] == 4 and corrs.shape[0] == feat_a.shape[0]
    assert valid.dtype == torch.int32 and tuple(valid.shape) == (feat_a.shape[0],)
    B, C, FH, FW = feat_a.shape
    N = corrs.shape[1]
    n_pool = 0
    if pool is not None:
        assert pool.dtype == torch.int32 and pool.dim() == 3 and tuple(pool.shape[:2]) == (B, 2)
        n_pool = pool.shape[2]
    ws = _lib.workspace(dev, lib().oryon_feature_loss_workspace_bytes(B, N, n_pool),
                        f"oryon_feature_loss_workspace_bytes({B}, {N}, {n_pool})" if B > 0 else None, workspace)
    d_pos = torch.empty((B, N), dtype=torch.float32, device=dev)
    d_neg = torch.empty((B, 2, N), dtype=torch.float32, device=dev)
    neg_idx = torch.empty((B, 2, N), dtype=torch.int32, device=dev)
    pair_terms = torch.empty((B, 3), dtype=torch.float32, device=dev)
    losses = torch.empty((3,), dtype=torch.float32, device=dev)
    check(lib().oryon_feature_loss(ptr(feat_a), ptr(feat_q), B, C, FH, FW, ptr(corrs), N, ptr(valid), ptr(pool), n_pool,
                                   1 if pool_per_positive else 0, float(pos_margin), float(neg_margin), float(neg_kernel), ptr(ws), ws.numel(),
                                   ptr(d_pos), ptr(d_neg), ptr(neg_idx), ptr(pair_terms), ptr(losses), stream_ptr(dev)), "oryon_feature_loss")
    return dict(d_pos=d_pos, d_neg=d_neg, neg_idx=neg_idx, pair_terms=pair_terms, losses=losses)


@_on_tensor_device
def mask_dice_sums(logits: torch.Tensor, gt: torch.Tensor, threshold: float):
    """logits [B,H,W] fp32, gt [B,H,W] (non-zero = object, at the logits' size) -> (sums [B,4] float64 = sum p, sum p^2, sum p t, sum t
    with p = sigmoid(2 logits); mask [B,H,W] int32 = sigmoid(logits) > threshold; counts [B,2] int32 = |mask and gt|, |mask or gt|)."""
    dev = _lib.require_gpu(logits.device)
    assert logits.dim() == 3 and gt.shape == logits.shape
    logits = logits.to(torch.float32).contiguous()
    gt = gt.to(dev).to(torch.int32).contiguous()
    B, H, W = logits.shape
    sums = torch.empty((B, 4), dtype=torch.float64, device=dev)
    mask = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    check(lib().oryon_mask_dice_sums(ptr(logits), ptr(gt), B, H, W, float(threshold), ptr(sums), ptr(mask), ptr(counts), stream_ptr(dev)),
          "oryon_mask_dice_sums")
    return sums, mask, counts


@_on_tensor_device
def feature_loss_grad(feat_a: torch.Tensor, feat_q: torch.Tensor, corrs: torch.Tensor, valid: torch.Tensor, neg_idx: torch.Tensor,
                      d_pos: torch.Tensor, d_neg: torch.Tensor, g: torch.Tensor, pos_margin: float = 0.2, neg_margin: float = 0.9,
                      workspace: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """The backward pass of ops.feature_loss: feat_a, feat_q, corrs, valid as there, neg_idx / d_pos / d_neg = that call's outputs,
    g [3] fp32 on the device = the gradients of its `losses` -> (grad_a, grad_q) [B,C,FH,FW] fp32.  `out`: two contiguous fp32 buffers of
    that shape to write into.  Definition: include/oryon_hip.h, oryon_feature_loss_grad."""
    dev = _lib.require_gpu(feat_a.device)
    assert feat_a.dtype == torch.float32 and feat_q.dtype == torch.float32 and feat_a.shape == feat_q.shape and feat_a.dim() == 4
    B, C, FH, FW = feat_a.shape
    assert corrs.dtype == torch.int32 and corrs.dim() == 3 and corrs.shape[2] == 4 and corrs.shape[0] == B
    N = corrs.shape[1]
    assert valid.dtype == torch.int32 and tuple(valid.shape) == (B,)
    assert neg_idx.dtype == torch.int32 and tuple(neg_idx.shape) == (B, 2, N)
    assert d_pos.dtype == torch.float32 and tuple(d_pos.shape) == (B, N) and d_neg.dtype == torch.float32 and tuple(d_neg.shape) == (B, 2, N)
    assert g.dtype == torch.float32 and g.numel() == 3 and g.device == feat_a.device
    ws = _lib.workspace(dev, lib().oryon_feature_loss_grad_workspace_bytes(B, C, N),
                        f"oryon_feature_loss_grad_workspace_bytes({B}, {C}, {N})" if B > 0 else None, workspace,
                        "shape not supported (C <= 256, n_corr <= 4096)")
    if out is None:
        out = (torch.empty((B, C, FH, FW), dtype=torch.float32, device=dev), torch.empty((B, C, FH, FW), dtype=torch.float32, device=dev))
    grad_a, grad_q = out
    assert all(t.dtype == torch.float32 and tuple(t.shape) == (B, C, FH, FW) for t in out)
    check(lib().oryon_feature_loss_grad(ptr(feat_a), ptr(feat_q), B, C, FH, FW, ptr(corrs), N, ptr(valid), ptr(neg_idx), ptr(d_pos), ptr(d_neg),
                                        ptr(g), float(pos_margin), float(neg_margin), ptr(ws), ws.numel(), ptr(grad_a), ptr(grad_q),
                                        stream_ptr(dev)), "oryon_feature_loss_grad")
    return grad_a, grad_q


@_on_tensor_device
def mask_dice_grad(logits: torch.Tensor, gt: torch.Tensor, sums: torch.Tensor, g_mask: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward pass of the dice loss behind ops.mask_dice_sums: logits [B,H,W] fp32, gt [B,H,W] at the logits' size, sums [B,4]
    float64 = that call's output, g_mask [1] fp32 on the device -> grad_logits [B,H,W] fp32.  Definition: oryon_mask_dice_grad."""
    dev = _lib.require_gpu(logits.device)
    assert logits.dim() == 3 and gt.shape == logits.shape and logits.dtype == torch.float32
    B, H, W = logits.shape
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (B, 4)
    assert g_mask.dtype == torch.float32 and g_mask.numel() == 1 and g_mask.device == logits.device
    gt = gt.to(dev).to(torch.int32).contiguous()
    grad = out if out is not None else torch.empty((B, H, W), dtype=torch.float32, device=dev)
    assert grad.dtype == torch.float32 and tuple(grad.shape) == (B, H, W)
    check(lib().oryon_mask_dice_grad(ptr(logits), ptr(gt), B, H, W, ptr(sums), ptr(g_mask), ptr(grad), stream_ptr(dev)),
          "oryon_mask_dice_grad")
    return grad


@_on_tensor_device
def pose_metrics(pred_pose: torch.Tensor, gt_pose: torch.Tensor, model_pts: torch.Tensor, pts_offset: Optional[torch.Tensor] = None,
                 model_of_pair: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pred/gt [B,4,4] (metres), model_pts [M,3] (or the concatenation of several models with pts_offset [n+1] int32 and
    model_of_pair [B] int32) -> [B,4] = (ADD, ADD-S, rotation error deg, translation error cm), all on the device (f3)."""
    dev = _lib.require_gpu(pred_pose.device)
    B = pred_pose.shape[0]
    pred = pred_pose.to(dev, torch.float32).reshape(B, 16).contiguous()
    gt = gt_pose.to(dev, torch.float32).reshape(B, 16).contiguous()
    pts = model_pts.to(dev, torch.float32).contiguous()
    if pts_offset is None:
        pts_offset = torch.tensor([0, pts.shape[0]], dtype=torch.int32, device=dev)
    off_host = pts_offset.cpu()
    n_models = off_host.numel() - 1
    max_pts = int((off_host[1:] - off_host[:-1]).max()) if n_models > 0 else 0
    ws = torch.empty((B, 2), dtype=torch.float32, device=dev)
    out = torch.empty((B, 4), dtype=torch.float32, device=dev)
    mop = None if model_of_pair is None else model_of_pair.to(dev, torch.int32).contiguous()
    off_dev = pts_offset.to(dev, torch.int32).contiguous()
    check(lib().oryon_pose_metrics(ptr(pred), ptr(gt), B, ptr(pts), ptr(off_dev), n_models, max(1, max_pts),
                                   ptr(mop), ptr(ws), ptr(out), stream_ptr(dev)), "oryon_pose_metrics")
    return out


@_on_tensor_device
def pose_bop_errors(pred_pose: torch.Tensor, gt_pose: torch.Tensor, K: torch.Tensor, model_pts_mm: torch.Tensor, pts_offset: torch.Tensor,
                    syms: torch.Tensor, sym_offset: torch.Tensor, model_of_pair: Optional[torch.Tensor] = None,
                    max_points: int = 3) -> torch.Tensor:
    """MSSD (mm) and MSPD (px) of a batch of pairs on the device -> [B,2] float64 (utils/evaluator.py:258-275 +
    bop_toolkit_lib/pose_error.py:370-427).  pred / gt [B,4,4] metres, K [B,3,3]; model_pts_mm [sum M,3] millimetres with pts_offset
    [n+1]; syms [sum S,3,4] with sym_offset [n+1]; everything is handed over as float64 (the poses are rounded to float16 inside).
    max_points = 3 is the reference's behaviour (first three model points only, see include/oryon_hip.h); 0 = all points."""
    dev = _lib.require_gpu(pred_pose.device if pred_pose.is_cuda else model_pts_mm.device)
    B = pred_pose.shape[0]
    f64 = lambda t, shape: t.to(dev, torch.float64).reshape(shape).contiguous()
    pred, gt, Kc = f64(pred_pose, (B, 16)), f64(gt_pose, (B, 16)), f64(K, (B, 9))
    pts, sy = f64(model_pts_mm, (-1, 3)), f64(syms, (-1, 12))
    po, so = pts_offset.to(torch.int32).cpu(), sym_offset.to(torch.int32).cpu()
    n_models = po.numel() - 1
    max_syms = int((so[1:] - so[:-1]).max())
    ws = _lib.workspace(dev, lib().oryon_pose_bop_workspace_bytes(B, max_syms))
    out = torch.empty((B, 2), dtype=torch.float64, device=dev)
    mop = None if model_of_pair is None else model_of_pair.to(dev, torch.int32).contiguous()
    po_d, so_d = po.to(dev), so.to(dev)               # named: a temporary would be freed (and its block re-used) before the launch
    check(lib().oryon_pose_bop_errors(ptr(pred), ptr(gt), ptr(Kc), B, ptr(pts), ptr(po_d), ptr(sy), ptr(so_d), n_models, max_syms,
                                      ptr(mop), int(max_points), ptr(ws), ptr(out), stream_ptr(dev)), "oryon_pose_bop_errors")
    return out



def _mesh_args(dev, verts_mm, faces, vert_offset, face_offset):
    """Device copies of a (concatenated) mesh and what the C ABI wants to know about it."""
    verts = verts_mm.to(dev, torch.float32).reshape(-1, 3).contiguous()
    fc = faces.to(dev, torch.int32).reshape(-1, 3).contiguous()
    vo = (torch.tensor([0, verts.shape[0]]) if vert_offset is None else vert_offset).to(torch.int32).cpu()
    fo = (torch.tensor([0, fc.shape[0]]) if face_offset is None else face_offset).to(torch.int32).cpu()
    assert vo.numel() == fo.numel() and int(vo[-1]) == verts.shape[0] and int(fo[-1]) == fc.shape[0]
    n_models = fo.numel() - 1
    max_faces = max(1, int((fo[1:] - fo[:-1]).max()))
    return verts, fc, vo.to(dev), fo.to(dev), n_models, max_faces


@_on_tensor_device
def render_depth(pose: torch.Tensor, K: torch.Tensor, verts_mm: torch.Tensor, faces: torch.Tensor, H: int, W: int,
                 vert_offset: Optional[torch.Tensor] = None, face_offset: Optional[torch.Tensor] = None,
                 model_of_image: Optional[torch.Tensor] = None, return_route_counts: bool = False):
    """Depth images [N,H,W] float32 (millimetres, 0 = background) of triangle meshes on the device (f3, csrc/vsd.hip; replaces the
    OpenGL depth render of bop_toolkit_lib/renderer_vispy.py:512-617).  pose [N,4,4] (rotation, translation in millimetres), K [N,3,3];
    verts_mm [V,3] and faces [F,3] (zero-based) of one model, or the concatenation of several with vert_offset / face_offset [n+1]
    (face indices local to their model) and model_of_image [N].  return_route_counts: also the workspace's two counters as a host
    tuple (triangles drawn one wave each, triangles drawn one thread each) - a host sync, for tests."""
    dev = _lib.require_gpu(pose.device if pose.is_cuda else verts_mm.device)
    N = pose.shape[0]
    P = pose.to(dev, torch.float32).reshape(N, 16).contiguous()
    Kc = K.to(dev, torch.float32).reshape(N, 9).contiguous()
    verts, fc, vo_d, fo_d, n_models, max_faces = _mesh_args(dev, verts_mm, faces, vert_offset, face_offset)
    moi = None if model_of_image is None else model_of_image.to(dev, torch.int32).contiguous()
    ws = _lib.workspace(dev, lib().oryon_render_depth_workspace_bytes(N, max_faces))
    depth = torch.empty((N, int(H), int(W)), dtype=torch.float32, device=dev)
    check(lib().oryon_render_depth(ptr(P), ptr(Kc), N, ptr(verts), ptr(vo_d), ptr(fc), ptr(fo_d), n_models, max_faces, ptr(moi), int(H),
                                   int(W), ptr(ws), ptr(depth), stream_ptr(dev)), "oryon_render_depth")
    if return_route_counts:
        large, small = ws[:8].view(torch.int32).tolist() if N > 0 else (0, 0)
        return depth, (large, small)
    return depth


@_on_tensor_device
def vsd_counts(pred_pose: torch.Tensor, gt_pose: torch.Tensor, K: torch.Tensor, depth_test: torch.Tensor, verts_mm: torch.Tensor,
               faces: torch.Tensor, diameter_mm: torch.Tensor, vert_offset: Optional[torch.Tensor] = None,
               face_offset: Optional[torch.Tensor] = None, model_of_pair: Optional[torch.Tensor] = None, delta: float = 15.0,
               taus=None) -> torch.Tensor:
    """The integer counts behind VSD for B pairs -> [B, 2 + n_tau] int32 = (n_union, n_inter, n_cost[tau]...) (f3, csrc/vsd.hip;
    bop_toolkit_lib/pose_error.py:17-93 behind the float16 pose rounding of utils/evaluator.py:263-266).  pred / gt [B,4,4] metres,
    K [B,3,3], depth_test [B,H,W] millimetres, mesh as render_depth, diameter_mm [B]; taus default to the evaluator's
    arange(0.05, 0.51, 0.05).  evaluation.vsd_errors turns the counts into the errors."""
    dev = _lib.require_gpu(depth_test.device if depth_test.is_cuda else verts_mm.device)
    B, H, W = depth_test.shape
    f64 = lambda t, shape: t.to(dev, torch.float64).reshape(shape).contiguous()
    pred, gt, Kc, diam = f64(pred_pose, (B, 16)), f64(gt_pose, (B, 16)), f64(K, (B, 9)), f64(diameter_mm, (B,))
    dt = depth_test.to(dev, torch.float32).contiguous()
    if taus is None:
        import numpy as np
        taus = np.arange(0.05, 0.51, 0.05)
    taus_d = torch.as_tensor(taus, dtype=torch.float64).to(dev).contiguous()
    n_tau = taus_d.numel()
    verts, fc, vo_d, fo_d, n_models, max_faces = _mesh_args(dev, verts_mm, faces, vert_offset, face_offset)
    mop = None if model_of_pair is None else model_of_pair.to(dev, torch.int32).contiguous()
    ws = _lib.workspace(dev, lib().oryon_vsd_workspace_bytes(B, H, W, max_faces))
    counts = torch.empty((B, 2 + n_tau), dtype=torch.int32, device=dev)
    check(lib().oryon_vsd_counts(ptr(pred), ptr(gt), ptr(Kc), ptr(dt), B, H, W, ptr(verts), ptr(vo_d), ptr(fc), ptr(fo_d), n_models, max_faces,
                                 ptr(mop), ptr(diam), float(delta), ptr(taus_d), n_tau, ptr(ws), ptr(counts), stream_ptr(dev)),
          "oryon_vsd_counts")
    return counts


def _host_counts(n, B: int, cap: int, what: str):
    """Counts given on the host (None, ints, lists, CPU tensors) -> a [B] int32 CPU tensor, checked against the capacity BEFORE anything
    touches the GPU (the kernels read a device count above its capacity as the capacity; here it is the caller's mistake).  Device
    tensors pass through unchecked: reading them back would synchronise."""
    if isinstance(n, torch.Tensor) and n.is_cuda:
        if n.dtype != torch.int32 or tuple(n.shape) != (B,):
            raise ValueError(f"{what}: device counts must be [B] int32, got {tuple(n.shape)} {n.dtype}")
        return n
    t = torch.full((B,), cap, dtype=torch.int64) if n is None else torch.as_tensor(n, dtype=torch.int64).reshape(-1)
    if t.numel() != B:
        raise ValueError(f"{what}: {t.numel()} counts for {B} pairs")
    if bool((t < 0).any()) or bool((t > cap).any()):
        raise ValueError(f"{what}: counts {t.tolist()} outside [0, cap = {cap}]")
    return t.to(torch.int32)


def _gt_device(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cuda")


def pcd_nearest(src: torch.Tensor, dst: torch.Tensor, n_src=None, n_dst=None):
    """All-pairs nearest neighbour in 3-D, float64 (g1, csrc/gt_corrs.hip; torch.cdist + argmin of make_toyl_test.py:68-72 without the
    distance matrix).  src [B,cap_src,3], dst [B,cap_dst,3] (or [n,3]: one pair) float64; n_src / n_dst [B] rows in use (None = all)
    -> (idx [B,cap_src] int32 = the first minimiser, d2 [B,cap_src] float64 = its squared distance); rows >= n_src[b] are not written.
    Definition: include/oryon_hip.h, oryon_gt_corrs."""
    if src.dim() == 2:
        src, dst = src[None], dst[None]
    if src.dim() != 3 or dst.dim() != 3 or src.shape[2] != 3 or dst.shape[2] != 3 or src.shape[0] != dst.shape[0]:
        raise ValueError(f"pcd_nearest: src {tuple(src.shape)} / dst {tuple(dst.shape)} are not [B,n,3] clouds of one batch")
    B, cap_src, cap_dst = src.shape[0], src.shape[1], dst.shape[1]
    if cap_src < 1 or cap_dst < 1:
        raise ValueError("pcd_nearest: a capacity of 0 rows (pass one row and a count of 0)")
    ns, nd = _host_counts(n_src, B, cap_src, "pcd_nearest n_src"), _host_counts(n_dst, B, cap_dst, "pcd_nearest n_dst")
    dev = _lib.require_gpu(_gt_device(src, dst))
    with torch.cuda.device(dev):
        src, dst = src.to(dev, torch.float64).contiguous(), dst.to(dev, torch.float64).contiguous()
        ns, nd = ns.to(dev).contiguous(), nd.to(dev).contiguous()
        idx = torch.empty((B, cap_src), dtype=torch.int32, device=dev)
        d2 = torch.empty((B, cap_src), dtype=torch.float64, device=dev)
        check(lib().oryon_pcd_nearest_f64(ptr(src), ptr(ns), ptr(dst), ptr(nd), B, cap_src, cap_dst, ptr(idx), ptr(d2), stream_ptr(dev)),
              "oryon_pcd_nearest_f64")
    return idx, d2


def gtc_lift(depth: torch.Tensor, pix: torch.Tensor, n, cam9: torch.Tensor, pose: Optional[torch.Tensor] = None):
    """Lift listed pixels (g1): depth [B,H,W] fp32 millimetres, pix [B,cap] int32 linear pixels, n [B], cam9 [B,9] float64, pose [B,12]
    float64 rows of [R | t] or None -> (xyz [B,cap,3] float64 metres, yx [B,cap,2] int32); rows >= n[b] are not written."""
    B, H, W = depth.shape
    if pix.dim() != 2 or pix.shape[0] != B or pix.shape[1] < 1:
        raise ValueError(f"gtc_lift: pix {tuple(pix.shape)} is not [B = {B}, cap >= 1]")
    cap = pix.shape[1]
    nn = _host_counts(n, B, cap, "gtc_lift n")
    dev = _lib.require_gpu(_gt_device(depth, pix))
    with torch.cuda.device(dev):
        depth, pix = depth.to(dev, torch.float32).contiguous(), pix.to(dev, torch.int32).contiguous()
        cam = cam9.to(dev, torch.float64).reshape(B, 9).contiguous()
        T = None if pose is None else pose.to(dev, torch.float64).reshape(B, 12).contiguous()
        nn = nn.to(dev).contiguous()
        xyz = torch.empty((B, cap, 3), dtype=torch.float64, device=dev)
        yx = torch.empty((B, cap, 2), dtype=torch.int32, device=dev)
        check(lib().oryon_gtc_lift(ptr(depth), B, H, W, ptr(pix), ptr(nn), cap, ptr(cam), ptr(T), ptr(xyz), ptr(yx), stream_ptr(dev)),
              "oryon_gtc_lift")
    return xyz, yx


def gt_corrs(depth_a: torch.Tensor, depth_q: torch.Tensor, pix_a: torch.Tensor, n_a, pix_q: torch.Tensor, n_q, cam_a: torch.Tensor,
             cam_q: torch.Tensor, pose_aq: torch.Tensor, threshold: float, status: Optional[torch.Tensor] = None, want_nn: bool = False):
    """Ground-truth correspondences of B pairs (g1, csrc/gt_corrs.hip).  depth_* [B,H,W] fp32 millimetres; pix_* [B,cap] int32 pixel
    lists (roi_compact, or drawn through the reference's 20 000-point table) with n_* [B]; cam_* [B,9] or [B,3,3] float64; pose_aq
    [B,4,4] or [B,12] float64 (metres) -> dict(corrs [B,cap_a,4] int32 (y_a,x_a,y_q,x_q), n_corr [B] int32, idx / d2 [B,cap_a] | None)."""
    B = depth_a.shape[0]
    if depth_a.dim() != 3 or depth_q.dim() != 3 or depth_q.shape[0] != B:
        raise ValueError("gt_corrs: depth maps are [B,H,W]")
    if pix_a.dim() != 2 or pix_q.dim() != 2 or pix_a.shape[0] != B or pix_q.shape[0] != B or pix_a.shape[1] < 1 or pix_q.shape[1] < 1:
        raise ValueError(f"gt_corrs: pixel lists {tuple(pix_a.shape)} / {tuple(pix_q.shape)} are not [B = {B}, cap >= 1]")
    if not float(threshold) >= 0.0:
        raise ValueError(f"gt_corrs: threshold {threshold} is not >= 0")
    cap_a, cap_q = pix_a.shape[1], pix_q.shape[1]
    na, nq = _host_counts(n_a, B, cap_a, "gt_corrs n_a"), _host_counts(n_q, B, cap_q, "gt_corrs n_q")
    pose = pose_aq.reshape(B, -1)
    pose = pose[:, :12] if pose.shape[1] == 16 else pose
    if pose.shape[1] != 12:
        raise ValueError("gt_corrs: pose_aq is [B,4,4] or [B,12]")
    dev = _lib.require_gpu(_gt_device(depth_a, pix_a))
    with torch.cuda.device(dev):
        da, dq = depth_a.to(dev, torch.float32).contiguous(), depth_q.to(dev, torch.float32).contiguous()
        pa, pq = pix_a.to(dev, torch.int32).contiguous(), pix_q.to(dev, torch.int32).contiguous()
        ca, cq = cam_a.to(dev, torch.float64).reshape(B, 9).contiguous(), cam_q.to(dev, torch.float64).reshape(B, 9).contiguous()
        T = pose.to(dev, torch.float64).contiguous()
        na, nq = na.to(dev).contiguous(), nq.to(dev).contiguous()
        st = None if status is None else status.to(dev, torch.int32).contiguous()
        ws = _lib.workspace(dev, lib().oryon_gt_corrs_workspace_bytes(B, cap_a, cap_q),
                            f"oryon_gt_corrs_workspace_bytes({B}, {cap_a}, {cap_q})" if B > 0 else None)
        corrs = torch.empty((B, cap_a, 4), dtype=torch.int32, device=dev)
        n_corr = torch.empty((B,), dtype=torch.int32, device=dev)
        idx = torch.empty((B, cap_a), dtype=torch.int32, device=dev) if want_nn else None
        d2 = torch.empty((B, cap_a), dtype=torch.float64, device=dev) if want_nn else None
        check(lib().oryon_gt_corrs(ptr(da), ptr(dq), B, da.shape[1], da.shape[2], dq.shape[1], dq.shape[2], ptr(pa), ptr(na), cap_a, ptr(pq),
                                   ptr(nq), cap_q, ptr(ca), ptr(cq), ptr(T), float(threshold), ptr(st), ptr(ws), ws.numel(), ptr(corrs),
                                   ptr(n_corr), ptr(idx), ptr(d2), stream_ptr(dev)), "oryon_gt_corrs")
    return dict(corrs=corrs, n_corr=n_corr, idx=idx, d2=d2)


ICP_MAX_ROWS, ICP_MAX_ITER = 8192, 1000      # ORYON_ICP_MAX_ROWS, ORYON_ICP_MAX_ITER (include/oryon_hip.h)


def _icp_requirer(who: str):
    def require(cond: bool, check_name: str, detail: str = "") -> None:
        if not cond:
            raise ValueError(f"{who}: {check_name}" + (f" ({detail})" if detail else ""))
    return require


def _icp_check_counts(req, B: int, n_src=None, n_dst=None, status=None) -> None:
    """The [B] int32 tensors of a refiner, in the order given; None: not passed."""
    for name, t in (("n_src", n_src), ("n_dst", n_dst), ("status", status)):
        if t is not None:
            req(t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (B,), f"{name} is [B] int32", f"{tuple(t.shape)} {t.dtype}")
            req(t.is_contiguous(), f"{name}.is_contiguous")


def _icp_check_start(req, B: int, T_init, device, others, max_iter, tolerance, max_dist) -> int:
    """T_init, one device over `others` (status may be None among them), and the scalars both refiners share -> int(max_iter)."""
    req(T_init.dtype == torch.float32, "T_init.dtype == float32", str(T_init.dtype))
    req(tuple(T_init.shape) == (B, 4, 4), "T_init.shape == [B,4,4]", str(tuple(T_init.shape)))
    req(T_init.is_contiguous(), "T_init.is_contiguous")
    req(all(t.device == device for t in others + (T_init,) if t is not None), "one device")
    max_iter = int(max_iter)
    req(1 <= max_iter <= ICP_MAX_ITER, f"1 <= max_iter <= {ICP_MAX_ITER}", str(max_iter))
    req(float(tolerance) >= 0.0, "tolerance >= 0", str(tolerance))
    req(float(max_dist) >= 0.0, "max_dist >= 0", str(max_dist))
    return max_iter


def _icp_outputs(dev, B: int, cap_src: int, need: int, what: str, workspace=None, want_idx: bool = False):
    """What every refiner call writes: dict(T, T64, iters, mean_err, n_kept, idx | None, status), and the workspace."""
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    ws = _lib.workspace(dev, need, what, workspace)
    out = dict(T=new((B, 4, 4), torch.float32), T64=new((B, 3, 4), torch.float64), iters=new((B,), torch.int32),
               mean_err=new((B,), torch.float64), n_kept=new((B,), torch.int32), idx=new((B, cap_src), torch.int32) if want_idx else None,
               status=new((B,), torch.int32))
    return out, ws


def icp_refine(src: torch.Tensor, dst: torch.Tensor, n_src: torch.Tensor, n_dst: torch.Tensor, T_init: torch.Tensor, max_iter: int = 20,
               tolerance: float = 1e-3, max_dist: float = float("inf"), status: Optional[torch.Tensor] = None, want_idx: bool = False,
               workspace: Optional[torch.Tensor] = None):
    """ICP refinement of B poses (g2, csrc/icp.hip; definition: include/oryon_hip.h, oryon_icp_refine).  src [B,cap_src,3], dst
    [B,cap_dst,3] float64 metres, n_src / n_dst [B] int32, T_init [B,4,4] fp32, status [B] int32 or None - all contiguous device tensors
    of exactly these dtypes: nothing is converted or copied here, a tensor that does not fit is rejected with the name of the check.
    Runs on the current stream with no host round trip -> dict(T [B,4,4] fp32, T64 [B,3,4] float64, iters [B] int32, mean_err [B]
    float64, n_kept [B] int32, idx [B,cap_src] int32 | None, status [B] int32)."""
    req = _icp_requirer("icp_refine")
    for name, t in (("src", src), ("dst", dst), ("n_src", n_src), ("n_dst", n_dst), ("T_init", T_init)):
        req(isinstance(t, torch.Tensor) and t.is_cuda, f"{name}.is_cuda")
    req(src.dtype == torch.float64, "src.dtype == float64", str(src.dtype))
    req(dst.dtype == torch.float64, "dst.dtype == float64", str(dst.dtype))
    req(src.dim() == 3 and src.shape[2] == 3 and src.shape[1] >= 1, "src.shape == [B,cap_src,3]", str(tuple(src.shape)))
    B = src.shape[0]
    req(B >= 1, "B >= 1")
    req(dst.dim() == 3 and dst.shape[2] == 3 and dst.shape[1] >= 1 and dst.shape[0] == B, "dst.shape == [B,cap_dst,3]", str(tuple(dst.shape)))
    cap_src, cap_dst = src.shape[1], dst.shape[1]
    req(src.is_contiguous(), "src.is_contiguous")
    req(dst.is_contiguous(), "dst.is_contiguous")
    _icp_check_counts(req, B, n_src, n_dst, status)
    max_iter = _icp_check_start(req, B, T_init, src.device, (dst, n_src, n_dst, status), max_iter, tolerance, max_dist)
    req(cap_src <= ICP_MAX_ROWS and cap_dst <= ICP_MAX_ROWS, f"cap <= {ICP_MAX_ROWS}", f"{cap_src}, {cap_dst}")
    dev = _lib.require_gpu(src.device)
    with torch.cuda.device(dev):
        o, ws = _icp_outputs(dev, B, cap_src, lib().oryon_icp_workspace_bytes(B, cap_src, cap_dst),
                             f"oryon_icp_workspace_bytes({B}, {cap_src}, {cap_dst})", workspace, want_idx)
        check(lib().oryon_icp_refine(ptr(src), ptr(n_src), cap_src, ptr(dst), ptr(n_dst), cap_dst, B, ptr(T_init), max_iter, float(tolerance),
                                     float(max_dist), ptr(status), ptr(ws), ws.numel(), ptr(o["T"]), ptr(o["T64"]), ptr(o["iters"]),
                                     ptr(o["mean_err"]), ptr(o["n_kept"]), ptr(o["idx"]), ptr(o["status"]), stream_ptr(dev)), "oryon_icp_refine")
    return o


def icp_best_fit(A: torch.Tensor, Bp: torch.Tensor, n: torch.Tensor):
    """The rigid fit of ICP's step 4 over given correspondences (g2, oryon_icp_best_fit): A, Bp [B,cap,3] float64 (row i of A corresponds
    to row i of Bp), n [B] int32, contiguous device tensors -> dict(T [B,4,4] fp32, T64 [B,3,4] float64, fitted [B] int32,
    mean_err [B] float64 = the pairs' mean distance before the fit)."""
    for name, t in (("A", A), ("Bp", Bp)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 3 and t.shape[2] == 3 and t.is_contiguous()):
            raise ValueError(f"icp_best_fit: {name} is a contiguous [B,cap,3] float64 device tensor")
    B, cap = A.shape[0], A.shape[1]
    if tuple(Bp.shape) != tuple(A.shape) or not (1 <= cap <= ICP_MAX_ROWS) or B < 1:
        raise ValueError(f"icp_best_fit: A {tuple(A.shape)} / Bp {tuple(Bp.shape)}: one shape, 1 <= cap <= {ICP_MAX_ROWS}")
    if not (n.is_cuda and n.dtype == torch.int32 and tuple(n.shape) == (B,) and n.is_contiguous()):
        raise ValueError("icp_best_fit: n is [B] int32")
    dev = _lib.require_gpu(A.device)
    with torch.cuda.device(dev):
        o, ws = _icp_outputs(dev, B, cap, lib().oryon_icp_workspace_bytes(B, cap, cap), None)
        check(lib().oryon_icp_best_fit(ptr(A), ptr(Bp), ptr(n), cap, B, ptr(ws), ws.numel(), ptr(o["T"]), ptr(o["T64"]), ptr(o["iters"]),
                                       ptr(o["mean_err"]), stream_ptr(dev)), "oryon_icp_best_fit")
    return dict(T=o["T"], T64=o["T64"], fitted=o["iters"], mean_err=o["mean_err"])


def icp_plane_refine(src: torch.Tensor, n_src: torch.Tensor, depth: torch.Tensor, mask: torch.Tensor, cam9: torch.Tensor,
                     T_init: torch.Tensor, max_iter: int = 20, tolerance: float = 1e-5, max_dist: float = 0.02, normal_jump: float = 0.02,
                     status: Optional[torch.Tensor] = None, want_idx: bool = False, workspace: Optional[torch.Tensor] = None):
    """Point-to-plane ICP of B source clouds onto the queries' depth maps (g3, csrc/icp_plane.hip; definition: include/oryon_hip.h,
    oryon_icp_plane_refine).  src [B,cap_src,3] float64 metres, n_src [B] int32, depth [B,H,W] fp32 millimetres, mask [B,H,W] int32
    (1 = object), cam9 [B,9] float64, T_init [B,4,4] fp32, status [B] int32 or None - all contiguous device tensors of exactly these
    dtypes: nothing is converted or copied here, a tensor that does not fit is rejected with the name of the check.  max_dist and
    normal_jump in metres.  Runs on the current stream with no host round trip -> dict(T [B,4,4] fp32, T64 [B,3,4] float64, iters [B]
    int32, mean_err [B] float64, n_kept [B] int32, idx [B,cap_src] int32 | None (py W + px of a kept row, -1 otherwise), status [B])."""
    req = _icp_requirer("icp_plane_refine")
    for name, t in (("src", src), ("n_src", n_src), ("depth", depth), ("mask", mask), ("cam9", cam9), ("T_init", T_init)):
        req(isinstance(t, torch.Tensor) and t.is_cuda, f"{name}.is_cuda")
    req(src.dtype == torch.float64, "src.dtype == float64", str(src.dtype))
    req(src.dim() == 3 and src.shape[2] == 3 and src.shape[1] >= 1, "src.shape == [B,cap_src,3]", str(tuple(src.shape)))
    B, cap_src = src.shape[0], src.shape[1]
    req(B >= 1, "B >= 1")
    req(src.is_contiguous(), "src.is_contiguous")
    _icp_check_counts(req, B, n_src=n_src, status=status)
    req(depth.dtype == torch.float32, "depth.dtype == float32", str(depth.dtype))
    req(depth.dim() == 3 and depth.shape[0] == B, "depth.shape == [B,H,W]", str(tuple(depth.shape)))
    H, W = depth.shape[1], depth.shape[2]
    req(H >= 3 and W >= 3 and H * W < 2 ** 31, "H, W >= 3 and H W < 2^31", f"{H} x {W}")
    req(depth.is_contiguous(), "depth.is_contiguous")
    req(mask.dtype == torch.int32, "mask.dtype == int32", str(mask.dtype))
    req(tuple(mask.shape) == (B, H, W), "mask.shape == depth.shape", str(tuple(mask.shape)))
    req(mask.is_contiguous(), "mask.is_contiguous")
    req(cam9.dtype == torch.float64, "cam9.dtype == float64", str(cam9.dtype))
    req(tuple(cam9.shape) == (B, 9), "cam9.shape == [B,9]", str(tuple(cam9.shape)))
    req(cam9.is_contiguous(), "cam9.is_contiguous")
    max_iter = _icp_check_start(req, B, T_init, src.device, (n_src, depth, mask, cam9, status), max_iter, tolerance, max_dist)
    req(float(normal_jump) >= 0.0, "normal_jump >= 0", str(normal_jump))
    req(cap_src <= ICP_MAX_ROWS, f"cap_src <= {ICP_MAX_ROWS}", str(cap_src))
    dev = _lib.require_gpu(src.device)
    with torch.cuda.device(dev):
        o, ws = _icp_outputs(dev, B, cap_src, lib().oryon_icp_plane_workspace_bytes(B, cap_src),
                             f"oryon_icp_plane_workspace_bytes({B}, {cap_src})", workspace, want_idx)
        check(lib().oryon_icp_plane_refine(ptr(src), ptr(n_src), cap_src, ptr(depth), ptr(mask), H, W, ptr(cam9), B, ptr(T_init), max_iter,
                                           float(tolerance), float(max_dist), float(normal_jump), ptr(status), ptr(ws), ws.numel(), ptr(o["T"]),
                                           ptr(o["T64"]), ptr(o["iters"]), ptr(o["mean_err"]), ptr(o["n_kept"]), ptr(o["idx"]),
                                           ptr(o["status"]), stream_ptr(dev)), "oryon_icp_plane_refine")
    return o


POSE_VERIFY_CLASSES, POSE_VERIFY_MAX_POSES = 7, 16      # ORYON_POSE_VERIFY_CLASSES, ORYON_POSE_VERIFY_MAX_POSES (include/oryon_hip.h)
POSE_VERIFY_NAMES = ("behind", "outside", "unknown", "occluded", "violation", "off", "hit")      # the classes in the order of counts[..., c]
POSE_VERIFY_HIT = POSE_VERIFY_NAMES.index("hit")


def pose_verify(src: torch.Tensor, n_src: torch.Tensor, depth: torch.Tensor, mask: torch.Tensor, cam9: torch.Tensor, poses: torch.Tensor,
                tol: float = 0.01, status: Optional[torch.Tensor] = None, want_cls: bool = False, workspace: Optional[torch.Tensor] = None):
    """Depth-consistency verification of K candidate poses per pair (g4, csrc/pose_verify.hip; definition: include/oryon_hip.h,
    oryon_pose_verify).  src [B,cap_src,3] float64 metres, n_src [B] int32, depth [B,H,W] fp32 millimetres, mask [B,H,W] int32
    (1 = object), cam9 [B,9] float64, poses [B,K,4,4] fp32 ([B,4,4]: K = 1), status [B] int32 or None - all contiguous device tensors
    of exactly these dtypes: nothing is converted or copied here, a tensor that does not fit is rejected with the name of the check.
    tol in metres.  Runs on the current stream with no host round trip -> dict(counts [B,K,7] int32 (BEHIND, OUTSIDE, UNKNOWN, OCCLUDED,
    VIOLATION, OFF, HIT), best [B] int32, score [B,K] float64 = counts[HIT] / max(n_src, 1), and with want_cls cls [B,K,cap_src]
    int32: the class of every row, -1 beyond the count)."""
    req = _icp_requirer("pose_verify")
    for name, t in (("src", src), ("n_src", n_src), ("depth", depth), ("mask", mask), ("cam9", cam9), ("poses", poses)):
        req(isinstance(t, torch.Tensor) and t.is_cuda, f"{name}.is_cuda")
    req(src.dtype == torch.float64, "src.dtype == float64", str(src.dtype))
    req(src.dim() == 3 and src.shape[2] == 3 and src.shape[1] >= 1, "src.shape == [B,cap_src,3]", str(tuple(src.shape)))
    B, cap_src = src.shape[0], src.shape[1]
    req(B >= 1, "B >= 1")
    req(src.is_contiguous(), "src.is_contiguous")
    _icp_check_counts(req, B, n_src=n_src, status=status)
    req(depth.dtype == torch.float32, "depth.dtype == float32", str(depth.dtype))
    req(depth.dim() == 3 and depth.shape[0] == B, "depth.shape == [B,H,W]", str(tuple(depth.shape)))
    H, W = depth.shape[1], depth.shape[2]
    req(H >= 1 and W >= 1 and H * W < 2 ** 31, "H, W >= 1 and H W < 2^31", f"{H} x {W}")
    req(depth.is_contiguous(), "depth.is_contiguous")
    req(mask.dtype == torch.int32, "mask.dtype == int32", str(mask.dtype))
    req(tuple(mask.shape) == (B, H, W), "mask.shape == depth.shape", str(tuple(mask.shape)))
    req(mask.is_contiguous(), "mask.is_contiguous")
    req(cam9.dtype == torch.float64, "cam9.dtype == float64", str(cam9.dtype))
    req(tuple(cam9.shape) == (B, 9), "cam9.shape == [B,9]", str(tuple(cam9.shape)))
    req(cam9.is_contiguous(), "cam9.is_contiguous")
    req(poses.dtype == torch.float32, "poses.dtype == float32", str(poses.dtype))
    req(poses.dim() in (3, 4) and poses.shape[0] == B and tuple(poses.shape[-2:]) == (4, 4) and (poses.dim() == 3 or poses.shape[1] >= 1),
        "poses.shape == [B,K,4,4] or [B,4,4]", str(tuple(poses.shape)))
    req(poses.is_contiguous(), "poses.is_contiguous")
    K = 1 if poses.dim() == 3 else poses.shape[1]
    req(K <= POSE_VERIFY_MAX_POSES, f"K <= {POSE_VERIFY_MAX_POSES}", str(K))
    req(all(t.device == src.device for t in (n_src, depth, mask, cam9, poses, status) if t is not None), "one device")
    req(float(tol) >= 0.0, "tol >= 0", str(tol))
    req(cap_src <= ICP_MAX_ROWS, f"cap_src <= {ICP_MAX_ROWS}", str(cap_src))
    dev = _lib.require_gpu(src.device)
    with torch.cuda.device(dev):
        ws = _lib.workspace(dev, lib().oryon_pose_verify_workspace_bytes(B, cap_src, K),
                            f"oryon_pose_verify_workspace_bytes({B}, {cap_src}, {K})", workspace)
        counts = torch.empty((B, K, POSE_VERIFY_CLASSES), dtype=torch.int32, device=dev)
        best = torch.empty((B,), dtype=torch.int32, device=dev)
        cls = torch.empty((B, K, cap_src), dtype=torch.int32, device=dev) if want_cls else None
        check(lib().oryon_pose_verify(ptr(src), ptr(n_src), cap_src, ptr(depth), ptr(mask), H, W, ptr(cam9), B, ptr(poses), K, float(tol),
                                      ptr(status), ptr(ws), ws.numel(), ptr(counts), ptr(best), ptr(cls), stream_ptr(dev)), "oryon_pose_verify")
        score = counts[:, :, POSE_VERIFY_HIT].to(torch.float64) / torch.clamp(n_src, min=1, max=cap_src).to(torch.float64)[:, None]
    out = dict(counts=counts, best=best, score=score)
    if want_cls:
        out["cls"] = cls
    return out


MASK_CLEAN_MODES = ("all", "largest", "area")          # oryon_mask_clean's mode 0, 1, 2
MASK_CLEAN_ROUTES = ("auto", "lds", "global")           # its route 0, 1, 2
MASK_CLEAN_STATS = ("components", "a_max", "kept_components", "kept_pixels", "removed_pixels", "filled_pixels")      # stats[..., i]
MASK_CLEAN_LDS_PIXELS = 65536                           # ORYON_MASK_CLEAN_LDS_PIXELS (include/oryon_hip.h): what the LDS route holds


def mask_clean_frac_q16(frac: float) -> int:
    """The one rounding of the area fraction, on the host: the device compares integers only."""
    return int(min(max(round(float(frac) * 65536.0), 0), 65536))


@_on_tensor_device
def mask_clean(mask: torch.Tensor, mode: str = "largest", frac: float = 0.25, fill_holes: bool = False, route: str = "auto",
               want_labels: bool = False, want_stats: bool = False):
    """Mask clean-up by connected components (h1, csrc/mask_clean.hip; definition: include/oryon_hip.h, oryon_mask_clean).
    mask [n,H,W] or [H,W], foreground = (mask == 1) -> out of the same shape, int32 0 / 1: with fill_holes the enclosed holes
    (4-connected background that does not reach the border) filled, then of the 8-connected components every one (mode 'all'), the
    largest (ties: the one that starts first in raster order) or those of at least frac x the largest area ('area').  route: 'auto'
    (one workgroup per map in LDS up to MASK_CLEAN_LDS_PIXELS pixels, else the global route), 'lds' or 'global'.  Runs on the current
    stream with no host round trip.  -> out, or (out[, labels][, stats]): labels int32, the smallest linear index of every foreground
    pixel's component before the selection and -1 on the background; stats [n, 6] ([6] for one map) int32, MASK_CLEAN_STATS."""
    if mode not in MASK_CLEAN_MODES:
        raise ValueError(f"mask_clean: mode {mode!r} is none of {MASK_CLEAN_MODES}")
    if route not in MASK_CLEAN_ROUTES:
        raise ValueError(f"mask_clean: route {route!r} is none of {MASK_CLEAN_ROUTES}")
    if not 0.0 <= float(frac) <= 1.0:
        raise ValueError(f"mask_clean: frac must lie in [0, 1], not {frac}")
    if not (isinstance(mask, torch.Tensor) and mask.dim() in (2, 3)):
        raise ValueError("mask_clean: mask is a tensor [n,H,W] or [H,W]")
    single = mask.dim() == 2
    dev = _lib.require_gpu(mask.device)
    m = (mask[None] if single else mask).to(torch.int32).contiguous()
    n, H, W = m.shape
    if H < 1 or W < 1:
        raise ValueError(f"mask_clean: an empty map ({H} x {W})")
    out = torch.empty_like(m)
    labels = torch.empty_like(m) if want_labels else None
    stats = torch.empty((n, len(MASK_CLEAN_STATS)), dtype=torch.int32, device=dev) if want_stats else None
    if n > 0:
        r = MASK_CLEAN_ROUTES.index(route)
        ws = _lib.workspace(dev, lib().oryon_mask_clean_workspace_bytes(n, H, W, r), f"oryon_mask_clean_workspace_bytes({n}, {H}, {W}, {r})")
        check(lib().oryon_mask_clean(ptr(m), n, H, W, MASK_CLEAN_MODES.index(mode), mask_clean_frac_q16(frac), int(bool(fill_holes)), r,
                                     ptr(out), ptr(labels), ptr(stats), ptr(ws), ws.numel(), stream_ptr(dev)), "oryon_mask_clean")
    res = tuple(t[0] if single else t for t in (out, labels, stats) if t is not None)
    return res[0] if len(res) == 1 else res


_x3_weights = {}
# Validation mode of the fp16x3 path (backbone.enable_fp16x3(True, guard=True)): every call first checks max|activation| against the
# float16 range (one reduction + a host sync per linear - for a first run with a real checkpoint, not for throughput) and evaluates
# that layer with torch's fp32 linear when the split would overflow; weights are checked once, when they are split.
X3_GUARD = False
X3_LIMIT = 60000.0            # below float16's 65504 with room for the rounding of `hi`
X3_EXACT_WEIGHTS = True       # use the two-product kernel for weights whose fp16 split has no low half (results are bit-identical)
x3_guard_fallbacks = 0        # layers evaluated by torch because an operand left the float16 range (guard mode)


def x3_range_flag(device=None, reset: bool = True) -> bool:
    """oryon_x3_range_flag: True when an fp16x3 kernel launched on `device`'s CURRENT stream saw an out-of-range / non-finite output since
    that stream's flag was last cleared.  Synchronises that stream: call once per forward.  The flag word belongs to the (device, stream)
    pair: other streams' launches neither raise nor clear it."""
    dev = _lib.require_gpu(torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))
    v = ctypes.c_int(0)
    with torch.cuda.device(dev):
        check(lib().oryon_x3_range_flag(ctypes.byref(v), int(bool(reset)), stream_ptr(dev)), "oryon_x3_range_flag")
    return v.value != 0


def x3_range_reset(device=None) -> None:
    """Queue a clear of the current stream's fp16x3 range flag (no synchronisation, no read-back): the start of a forward.  The first
    call on a device allocates its flag table, so that no kernel launch does."""
    dev = _lib.require_gpu(torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))
    with torch.cuda.device(dev):
        check(lib().oryon_x3_range_flag(None, 1, stream_ptr(dev)), "oryon_x3_range_flag")


def _split_weight_f16x3(weight: torch.Tensor):
    """(hi, lo) fp16 halves of an fp32 weight, made once per live tensor and in-place version and cached.  The entry holds a weak
    reference to the tensor it was made from: an address re-used by another tensor after a free can not hit a stale split."""
    key = id(weight)
    hit = _x3_weights.get(key)
    if hit is not None and (hit[0]() is not weight or hit[1] != (weight._version, weight.data_ptr(), tuple(weight.shape))):
        hit = None
    if hit is None:
        w = weight.detach().to(torch.float32).contiguous()
        if X3_GUARD and float(w.abs().amax()) >= X3_LIMIT:
            raise _lib.OryonError(f"fp16x3 linear: a weight of magnitude {float(w.abs().amax()):.3g} does not fit the float16 split "
                                  "(|w| must stay below 65504): evaluate this model with backbone.enable_fp16x3(False)")
        hi = torch.empty(w.shape, dtype=torch.float16, device=w.device)
        lo = torch.empty(w.shape, dtype=torch.float16, device=w.device)
        check(lib().oryon_split_f16x3(ptr(w), w.numel(), ptr(hi), ptr(lo), stream_ptr(w.device)), "oryon_split_f16x3")
        # A weight that IS an fp16 value in every element (what `clip.load` leaves in the reference's CLIPEncoder - an fp16 checkpoint
        # widened with `.to(torch.float32)`, models/vlm.py:19-22 - and what every frozen layer of a checkpoint fine-tuned from it still
        # holds) has an all-zero low half: the kernel then leaves out the a_hi * w_lo products (W_lo = NULL; 16 instead of 24 MFMAs per
        # k-step, bit-identical results).  One device read-back per weight and version, here, never per call.
        if X3_EXACT_WEIGHTS and w.shape[1] >= 64 and not bool(lo.any()):
            lo = None
        if len(_x3_weights) > 4096:
            _x3_weights.clear()
        ref = weakref.ref(weight, lambda _r, k=key: _x3_weights.pop(k, None))
        hit = _x3_weights[key] = (ref, (weight._version, weight.data_ptr(), tuple(weight.shape)), hi, lo)
    return hit[2], hit[3]


def linear_f16x3_supported(x: torch.Tensor, weight: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and not torch.is_grad_enabled()
            and weight.dim() == 2 and weight.shape[1] % 32 == 0 and x.shape[-1] == weight.shape[1] and weight.numel() < 2 ** 30
            and (weight.shape[0] % 256 == 0 or (weight.shape[0] % 128 == 0 and weight.shape[1] >= 64)))


@_on_tensor_device
def linear_f16x3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, quick_gelu: bool = False,
                 gelu: bool = False) -> torch.Tensor:
    """act(x @ weight.T + bias) for fp32 x [..., K], weight [N, K] on the fp16 matrix pipe with error-compensated operands (B4):
    fp32-grade results (~1e-6 relative) at ~3x the fp32-MFMA rate.  act: QuickGELU (CLIP) or erf-GELU (Swin) or none.  Inference only.
    Range: |x|, |w| < 65504 or the split overflows silently to inf (X3_GUARD checks it, see above); an operand below 2^-3 in magnitude
    has its low half in float16's subnormal range, i.e. an ABSOLUTE split error of up to 2^-25 instead of the relative 2^-22."""
    dev = _lib.require_gpu(x.device)
    assert not (quick_gelu and gelu)
    K, N = weight.shape[1], weight.shape[0]
    x2 = x.reshape(-1, K).contiguous()
    if X3_GUARD and not bool(torch.isfinite(x2).all() & (x2.abs().amax() < X3_LIMIT)):
        global x3_guard_fallbacks
        x3_guard_fallbacks += 1
        y = torch.nn.functional.linear(x2, weight, bias)
        y = y * torch.sigmoid(1.702 * y) if quick_gelu else (torch.nn.functional.gelu(y) if gelu else y)
        return y.view(*x.shape[:-1], N)
    hi, lo = _split_weight_f16x3(weight)
    out = torch.empty((x2.shape[0], N), dtype=torch.float32, device=dev)
    b = None if bias is None else bias.detach().to(torch.float32).contiguous()
    check(lib().oryon_linear_f16x3(ptr(x2), x2.shape[0], K, ptr(hi), ptr(lo) if lo is not None else None, ptr(b), N, 2 if gelu else (1 if quick_gelu else 0), ptr(out),
                                   stream_ptr(dev)), "oryon_linear_f16x3")
    return out.view(*x.shape[:-1], N)


def linear_f16x3_acc_supported(weight: torch.Tensor, out: torch.Tensor) -> bool:
    """Can `out += x @ weight.T + bias` run in place (oryon_linear_f16x3_acc)?  x is any fp32 CUDA tensor [..., K] with out's row count."""
    return (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and weight.dtype == torch.float32 and weight.dim() == 2
            and not torch.is_grad_enabled() and not X3_GUARD and weight.shape[1] % 32 == 0 and weight.shape[1] >= 64
            and weight.shape[0] % 128 == 0 and weight.numel() < 2 ** 30 and out.shape[-1] == weight.shape[0])


@_on_tensor_device
def linear_f16x3_acc(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor) -> torch.Tensor:
    """out += x @ weight.T + bias, in place (oryon_linear_f16x3_acc): the residual update of a transformer block done by its last linear.
    Same value per element as `out + linear_f16x3(x, weight, bias)` (one fp32 addition of the finished sum)."""
    dev = _lib.require_gpu(x.device)
    K, N = weight.shape[1], weight.shape[0]
    x2 = x.reshape(-1, K).contiguous()
    assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == x2.shape[0] * N and out.data_ptr() != x2.data_ptr()
    hi, lo = _split_weight_f16x3(weight)
    b = None if bias is None else bias.detach().to(torch.float32).contiguous()
    check(lib().oryon_linear_f16x3_acc(ptr(x2), x2.shape[0], K, ptr(hi), ptr(lo) if lo is not None else None, ptr(b), N, ptr(out),
                                       stream_ptr(dev)), "oryon_linear_f16x3_acc")
    return out


@_on_tensor_device
def mha_f16x3(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """Self-attention on the packed in_proj output qkv [N, L, 3*D] fp32 (head dim 64, no mask) -> [N, L, D] fp32 (B5)."""
    dev = _lib.require_gpu(qkv.device)
    N, L, D3 = qkv.shape
    D = D3 // 3
    assert qkv.dtype == torch.float32 and D == heads * 64 and D3 == 3 * D
    qkv = qkv.contiguous()
    out = torch.empty((N, L, D), dtype=torch.float32, device=dev)
    check(lib().oryon_mha_f16x3(ptr(qkv), N, L, heads, 64, ptr(out), stream_ptr(dev)), "oryon_mha_f16x3")
    return out


@_on_tensor_device
def sample_first_gate(n_valid1: torch.Tensor, n_a1: torch.Tensor, n_a: torch.Tensor, max_corrs: int) -> torch.Tensor:
    """Per-pair anchor counts of the second matcher stage: n_a where the first stage came up short although anchors were left out, else 0."""
    dev = _lib.require_gpu(n_a.device)
    out = torch.empty_like(n_a)
    check(lib().oryon_sample_first_gate(ptr(n_valid1), ptr(n_a1), ptr(n_a), n_a.shape[0], int(max_corrs), ptr(out), stream_ptr(dev)),
          "oryon_sample_first_gate")
    return out


@_on_tensor_device
def sample_first_merge_(n_a2, corrs2, n_valid2, n_sel2, status2, corrs1, n_valid1, n_sel1, status1) -> None:
    """In place: the second stage's correspondences / counts / status replace the first stage's for the pairs that were redone."""
    dev = _lib.require_gpu(corrs1.device)
    assert corrs1.shape == corrs2.shape
    check(lib().oryon_sample_first_merge(ptr(n_a2), ptr(corrs2), ptr(n_valid2), ptr(n_sel2), ptr(status2), corrs1.shape[0], corrs1.shape[1],
                                         ptr(corrs1), ptr(n_valid1), ptr(n_sel1), ptr(status1), stream_ptr(dev)), "oryon_sample_first_merge")
