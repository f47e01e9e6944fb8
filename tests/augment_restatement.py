"""A numpy statement of the training augmentations (include/oryon_hip.h, K-1a), written from the definition - torchvision's
tensor path for ColorJitter, utils/augmentations.py:51-127 for the flips, preproc.hip's header for the resize - and not from the device
code.  Images are float64 [3,H,W] in [0,1] (the reference's numpy `/255.`); the hue stage alone runs in `hue_dtype` (float32 as
defined; float64 = the same formulas in exact-enough arithmetic, the yardstick of what the float32 stage costs).

    colour_jitter(x, fn_idx, factors)            one ColorJitter application
    apply_colour(x, applications)                jitter, then bright
    flip_image / flip_box / flip_coords          the flips
    resize_bilinear(x, out_hw)                   float64 bilinear, align_corners=False
    augment_resize(rgb_u8, applications, hflip, vflip, out_hw)   the whole of oryon_rgb_augment_resize for one image, float64 out
"""
import numpy as np


def gray(x):
    return (0.2989 * x[0] + 0.587 * x[1]) + 0.114 * x[2]


def blend(a, b, f):
    return np.clip(f * a + (1.0 - f) * b, 0.0, 1.0)


def rgb_to_hsv(x):
    r, g, b = x[0], x[1], x[2]
    one = x.dtype.type(1)
    maxc, minc = np.max(x, axis=0), np.min(x, axis=0)
    eqc = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eqc, one, maxc)
    d = np.where(eqc, one, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (x.dtype.type(2) + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (x.dtype.type(4) + gc - rc)
    h = np.fmod((hr + hg + hb) / x.dtype.type(6) + one, one)
    return h.astype(x.dtype), s.astype(x.dtype), maxc


def hsv_to_rgb(h, s, v):
    T = h.dtype.type
    h6 = h * T(6)
    i = np.floor(h6)
    fr = h6 - i
    i = i.astype(np.int32) % 6
    p = np.clip(v * (T(1) - s), T(0), T(1))
    q = np.clip(v * (T(1) - s * fr), T(0), T(1))
    t = np.clip(v * (T(1) - s * (T(1) - fr)), T(0), T(1))
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    return np.stack([r, g, b]).astype(h.dtype)


def adjust_hue(x, f, hue_dtype=np.float32):
    T = np.dtype(hue_dtype).type
    h, s, v = rgb_to_hsv(x.astype(hue_dtype))
    h = h + T(f)
    h = np.fmod(h, T(1))                       # remainder with the divisor's sign: a negative fmod gets the divisor added
    h = np.where(h < 0, h + T(1), h).astype(hue_dtype)
    return hsv_to_rgb(h, s, v).astype(np.float64)


def colour_jitter(x, fn_idx, factors, hue_dtype=np.float32):
    """x float64 [3,H,W]; fn_idx a permutation of (0 brightness, 1 contrast, 2 saturation, 3 hue); factors[id] None = skipped."""
    x = np.asarray(x, dtype=np.float64)
    for op in fn_idx:
        f = factors[op]
        if f is None:
            continue
        if op == 0:
            x = blend(x, 0.0, f)
        elif op == 1:
            x = blend(x, np.mean(gray(x)), f)
        elif op == 2:
            x = blend(x, gray(x)[None], f)
        else:
            x = adjust_hue(x, f, hue_dtype)
    return x


def apply_colour(x, applications, hue_dtype=np.float32):
    for fn_idx, factors in applications:
        x = colour_jitter(x, fn_idx, factors, hue_dtype)
    return x


def flip_image(x, hflip, vflip):
    """Mirrors the last axis (hflip) / the one before it (vflip) of [..,H,W]."""
    if hflip:
        x = x[..., ::-1]
    if vflip:
        x = x[..., ::-1, :]
    return np.ascontiguousarray(x)


def flip_box(box, H, W, hflip, vflip):
    y, x, h, w = box
    if hflip:
        x = W - w - x
    if vflip:
        y = H - y - h
    return [y, x, h, w]


def flip_coords(coords, H, W, hflip, vflip):
    out = np.array(coords, copy=True)
    if hflip:
        out[:, 1] = W - out[:, 1] - 1
    if vflip:
        out[:, 0] = H - out[:, 0] - 1
    return out


def _taps(out_size, in_size):
    src = (in_size / out_size) * (np.arange(out_size, dtype=np.float64) + 0.5) - 0.5
    src = np.maximum(src, 0.0)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = src - i0
    return i0, i1, 1.0 - l1, l1


def resize_bilinear(x, out_hw):
    """float64 [C,H,W] -> [C,HO,WO]: out = l0h*(l0w*a + l1w*b) + l1h*(l0w*c + l1w*d)."""
    y0, y1, ly0, ly1 = _taps(out_hw[0], x.shape[-2])
    x0, x1, lx0, lx1 = _taps(out_hw[1], x.shape[-1])
    a, b = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    c, d = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    return ly0[None, :, None] * (lx0 * a + lx1 * b) + ly1[None, :, None] * (lx0 * c + lx1 * d)


def augment_resize(rgb_u8, applications, hflip, vflip, out_hw, hue_dtype=np.float32):
    """uint8 [H,W,3] -> float64 [3,HO,WO]: /255., CHW, colour applications, flips, resize.  (The colour ops are pointwise apart from the
    image mean, which a flip does not change: colour-then-flip equals the reference's flip-after-colour order and any other.)"""
    x = np.asarray(rgb_u8).transpose(2, 0, 1) / 255.0
    x = apply_colour(x, applications, hue_dtype)
    return resize_bilinear(flip_image(x, hflip, vflip), out_hw)
