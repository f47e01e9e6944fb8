"""Plain numpy statements of the kernels in front of and behind the matcher: the three K-1 resizes (csrc/preproc.hip, csrc/roi.hip, the tap
of csrc/resample.h), the ROI compaction (csrc/roi.hip), the K2 lifts (csrc/post.hip) and the pose metrics (csrc/evaluate.hip).  Written from
the definitions in those files' headers and in include/oryon_hip.h, not from the device code.

    taps(out, in, dtype)                      the bilinear tap of one axis
    bilinear64(x, out_hw)                     float64 [n,HI,WI] -> [n,HO,WO]
    rgb64(u8, out_hw)                         uint8 [n,HI,WI,3] -> /255. -> CHW -> bilinear, float64 [n,3,HO,WO]
    depth_bar(x, out_hw)                      the per-pixel error bar of the fp32 depth resize (derivation below)
    nearest(mask, out_hw)                     torch's legacy 'nearest' index rule in float32, values passed through as int32
    compact(mask)                             per map, the ordered list of the pixels equal to 1
    lift_pairs(...), lift_points(...)         float32, one operation per rounding
    transform_f16(pts, R, t)                  the float16 model transform
    pose_stats(pts, pred, gt)                 float64 ADD / ADD-S of the half-transformed clouds
"""
import numpy as np

U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ resizes
def taps(out_size, in_size, dtype=np.float64):
    """scale = in/out, src = max(scale*(dst+0.5)-0.5, 0), i0 = min(int(src), in-1), i1 = i0 + (i0 < in-1), l1 = src-i0, l0 = 1-l1."""
    T = np.dtype(dtype).type
    scale = T(in_size) / T(out_size)
    src = np.maximum(scale * (np.arange(out_size).astype(dtype) + T(0.5)) - T(0.5), T(0))
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (src - i0.astype(dtype)).astype(dtype)
    return i0, i1, (T(1) - l1).astype(dtype), l1


def bilinear64(x, out_hw):
    """float64 [n,HI,WI] -> [n,HO,WO]: l0y*(l0x*a + l1x*b) + l1y*(l0x*c + l1x*d)."""
    x = np.asarray(x, dtype=np.float64)
    y0, y1, ly0, ly1 = taps(out_hw[0], x.shape[-2])
    x0, x1, lx0, lx1 = taps(out_hw[1], x.shape[-1])
    a, b = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    c, d = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    return ly0[None, :, None] * (lx0 * a + lx1 * b) + ly1[None, :, None] * (lx0 * c + lx1 * d)


def rgb64(u8, out_hw):
    """uint8 [n,HI,WI,3] -> float64 [n,3,HO,WO]."""
    x = np.asarray(u8).transpose(0, 3, 1, 2) / 255.0
    n = x.shape[0]
    return bilinear64(x.reshape(n * 3, x.shape[2], x.shape[3]), out_hw).reshape(n, 3, out_hw[0], out_hw[1])


def depth_bar(x, out_hw):
    """Per output pixel, 4e (WI S_x + HI S_y + M), e = 2^-24: what the float32 resize of `x` [n,HI,WI] may differ by from bilinear64.
    S_x (S_y) = the largest |difference of horizontal (vertical) neighbours| of the input over rows y0-1..y1+1 and columns x0-1..x1+1
    clipped to the image, M = the largest |tap value|.  The float32 src is within 3e*in_size of the exact one (scale rounding, product,
    subtraction; fused or not), the bilinear surface is continuous, so a src that crosses an integer only moves the pixel into the
    neighbouring cell - hence the one-cell margin of S - and the lerp itself adds at most 4eM."""
    x = np.asarray(x, dtype=np.float64)
    n, HI, WI = x.shape
    y0, y1, _, _ = taps(out_hw[0], HI)
    x0, x1, _, _ = taps(out_hw[1], WI)
    dx = np.abs(np.diff(x, axis=2)) if WI > 1 else np.zeros((n, HI, 1))
    dy = np.abs(np.diff(x, axis=1)) if HI > 1 else np.zeros((n, 1, WI))
    sx = np.zeros((n, out_hw[0], out_hw[1]))
    sy = np.zeros_like(sx)
    # clipping the offsets names exactly the rows/columns of the clipped window: y0+2 is y1+1 except on the last row, where it clips to it
    for r in (-1, 0, 1, 2):
        for c in (-1, 0, 1):
            rows, cols = np.clip(y0 + r, 0, HI - 1), np.clip(x0 + c, 0, dx.shape[2] - 1)
            sx = np.maximum(sx, dx[:, rows][:, :, cols])
            rows, cols = np.clip(y0 + c, 0, dy.shape[1] - 1), np.clip(x0 + r, 0, WI - 1)
            sy = np.maximum(sy, dy[:, rows][:, :, cols])
    ax = np.abs(x)
    m = np.maximum(np.maximum(ax[:, y0][:, :, x0], ax[:, y0][:, :, x1]), np.maximum(ax[:, y1][:, :, x0], ax[:, y1][:, :, x1]))
    return 4.0 * U24 * (WI * sx + HI * sy + m)


def nearest(mask, out_hw):
    """[n,HI,WI] -> int32 [n,HO,WO]: ys = min(floor(float32(y) * (float32(HI)/float32(HO))), HI-1) in float32, x likewise."""
    mask = np.asarray(mask)
    HI, WI = mask.shape[-2:]
    f = np.float32
    ys = np.minimum(np.floor(np.arange(out_hw[0]).astype(f) * (f(HI) / f(out_hw[0]))).astype(np.int64), HI - 1)
    xs = np.minimum(np.floor(np.arange(out_hw[1]).astype(f) * (f(WI) / f(out_hw[1]))).astype(np.int64), WI - 1)
    return mask[:, ys][:, :, xs].astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ compaction
def compact(mask):
    """[n,H,W] -> per map the ascending linear indices of the pixels whose value is 1 (no other value counts)."""
    return [np.flatnonzero(m.reshape(-1) == 1).astype(np.int32) for m in np.asarray(mask)]


# ------------------------------------------------------------------------------------------------------------------ lifts
def _lift(depth, cam9, ix, iy):
    f = np.float32
    fx, cx, fy, cy = f(cam9[0]), f(cam9[2]), f(cam9[4]), f(cam9[5])
    z = depth[iy, ix].astype(f)
    X = ((ix.astype(f) - cx) * z).astype(f) / fx
    Y = ((iy.astype(f) - cy) * z).astype(f) / fy
    return X.astype(f), Y.astype(f), z


def lift_pairs(corrs, feat_hw, depth_a, depth_q, cam_a, cam_q):
    """corrs [n,4] int (ya, xa, yq, xq on the FH x FW grid), depth_* [H,W] float32 millimetres, cam_* [9] float32 -> (pcd_a, pcd_q [m,3]
    float32 metres, keep [n] bool).  y' = f32(y) * (f32(H)/f32(FH)); a row is kept when 0 <= y' < H and 0 <= x' < W on both sides; the
    pixel is trunc(y'), trunc(x'); X = (((x-cx)*z)/fx)/1000, Y likewise, Z = z/1000; kept rows stay in order."""
    f = np.float32
    corrs = np.asarray(corrs).reshape(-1, 4)
    FH, FW = feat_hw
    pix, keep = [], np.ones(corrs.shape[0], dtype=bool)
    for d, cy_, cx_ in ((depth_a, 0, 1), (depth_q, 2, 3)):
        H, W = d.shape
        yp = (corrs[:, cy_].astype(f) * (f(H) / f(FH))).astype(f)
        xp = (corrs[:, cx_].astype(f) * (f(W) / f(FW))).astype(f)
        keep &= (yp >= 0) & (yp < f(H)) & (xp >= 0) & (xp < f(W))
        pix.append((yp, xp))
    out = []
    for (yp, xp), d, cam in zip(pix, (depth_a, depth_q), (cam_a, cam_q)):
        iy, ix = np.trunc(yp[keep]).astype(np.int64), np.trunc(xp[keep]).astype(np.int64)
        X, Y, z = _lift(np.asarray(d, dtype=f), cam, ix, iy)
        out.append(np.stack([(X / f(1000)).astype(f), (Y / f(1000)).astype(f), (z / f(1000)).astype(f)], axis=1))
    return out[0], out[1], keep


def lift_points(depth, cam9, x_idx, y_idx):
    """Selected pixels of one depth map -> [n,3] float32 in the depth's unit: lift_pairs without the scale, the validity test, the /1000."""
    ix, iy = np.asarray(x_idx).astype(np.int64), np.asarray(y_idx).astype(np.int64)
    X, Y, z = _lift(np.asarray(depth, dtype=np.float32), cam9, ix, iy)
    return np.stack([X, Y, z], axis=1).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------------ pose metrics
def transform_f16(pts, R, t):
    """Points, R and t rounded to float16; the products accumulated in float32 in k order; one rounding to float16, + t16, one more."""
    f = np.float32
    p = np.asarray(pts).astype(np.float16).astype(f)
    R16 = np.asarray(R).astype(np.float16).astype(f)
    t16 = np.asarray(t).astype(np.float16)
    out = np.empty(p.shape, dtype=np.float16)
    for r in range(3):
        acc = (p[:, 0] * R16[r, 0]).astype(f)
        acc = (acc + (p[:, 1] * R16[r, 1]).astype(f)).astype(f)
        acc = (acc + (p[:, 2] * R16[r, 2]).astype(f)).astype(f)
        out[:, r] = (acc.astype(np.float16).astype(f) + t16[r].astype(f)).astype(np.float16)
    return out


def nearest_distance(a, b, chunk=256):
    """float64 brute force: for every row of a the distance to its nearest row of b."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty(a.shape[0])
    for i in range(0, a.shape[0], chunk):
        d = a[i:i + chunk, None, :] - b[None]
        out[i:i + chunk] = np.sqrt((d * d).sum(-1).min(1))
    return out


def pose_stats(pts, pred, gt):
    """(ADD, ADD-S) as float64 statistics of the half-transformed clouds: ADD = mean |half(a - b)|, ADD-S = mean nearest distance; an
    empty model gives 0, 0."""
    if np.asarray(pts).shape[0] == 0:
        return 0.0, 0.0
    a = transform_f16(pts, pred[:3, :3], pred[:3, 3])
    b = transform_f16(pts, gt[:3, :3], gt[:3, 3])
    diff = (a - b).astype(np.float64)                       # float16 - float16 = one rounding to float16
    return float(np.mean(np.sqrt((diff * diff).sum(1)))), float(np.mean(nearest_distance(a, b)))
