"""The float64 numpy statement of the ground-truth correspondence routine, written from its definition (include/oryon_hip.h,
oryon_gt_corrs) and from nothing else: every step is one correctly rounded IEEE operation per element, in the order the definition
gives, so the device kernels (csrc/gt_corrs.hip, compiled without contraction) must agree with it bit for bit.  Shared by
tests/test_gt_corrs_restatement.py (CPU, against the reference's recorded results) and tests/test_gpu_gt_corrs.py."""
import numpy as np
import torch

SAMPLE = 20000


def pixel_list(mask, mask_idx):
    """Row-major linear pixels where mask == mask_idx."""
    return np.nonzero(np.asarray(mask).reshape(-1) == mask_idx)[0].astype(np.int32)


def lift(depth, pix, K, pose=None):
    """depth [H,W] fp32 millimetres, pix [n] linear pixels, K [3,3] float64, pose [3|4,4] float64 or None -> xyz [n,3] float64, yx [n,2]."""
    depth = np.asarray(depth)
    assert depth.dtype == np.float32
    H, W = depth.shape
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    pix = np.asarray(pix, dtype=np.int64)
    y, x = pix // W, pix % W
    z = depth.reshape(-1)[pix].astype(np.float64)
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    dx = (x.astype(np.float32) - np.float32(cx)).astype(np.float64)            # the fp32 difference of the definition
    dy = (y.astype(np.float32) - np.float32(cy)).astype(np.float64)
    X = ((dx * z) / fx) / 1000.0
    Y = ((dy * z) / fy) / 1000.0
    Z = z / 1000.0
    if pose is not None:
        T = np.asarray(pose, dtype=np.float64)
        X, Y, Z = (((T[r, 0] * X + T[r, 1] * Y) + T[r, 2] * Z) + T[r, 3] for r in range(3))
    return np.stack([X, Y, Z], axis=1), np.stack([y, x], axis=1).astype(np.int32)


def nearest(src, dst, chunk=256, second=False):
    """src [n,3], dst [m,3] float64 -> (idx [n] int32 first minimiser, d2 [n] float64); idx -1 / d2 inf when m == 0.
    second=True adds the smallest squared distance among the OTHER columns (inf when m < 2): the margin the fixtures assert."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    n, m = src.shape[0], dst.shape[0]
    idx, d2, d2b = np.full(n, -1, dtype=np.int32), np.full(n, np.inf), np.full(n, np.inf)
    if m > 0:
        for r0 in range(0, n, chunk):
            s = src[r0:r0 + chunk]
            dx, dy, dz = (s[:, None, c] - dst[None, :, c] for c in range(3))
            d = ((dx * dx + dy * dy) + dz * dz)
            j = np.argmin(d, axis=1)
            rows = np.arange(s.shape[0])
            idx[r0:r0 + chunk], d2[r0:r0 + chunk] = j, d[rows, j]
            if second and m > 1:
                d[rows, j] = np.inf
                d2b[r0:r0 + chunk] = d.min(axis=1)
    return (idx, d2, d2b) if second else (idx, d2)


def keep(d2, threshold):
    return np.sqrt(d2) <= threshold


def threshold_margin(d2, threshold):
    """Smallest relative distance of a row's minimum from the threshold (inf for no rows): the cases assert it is >= 1e-9, so that a
    last-bit difference of a distance cannot move a row across the threshold."""
    d = np.sqrt(np.asarray(d2, dtype=np.float64))
    d = d[np.isfinite(d)]
    return float(np.min(np.abs(d - threshold) / max(threshold, 1e-300))) if d.size else float("inf")


def gt_corrs(depth_a, depth_q, pix_a, pix_q, K_a, K_q, pose_aq, threshold):
    """One pair -> dict(corrs [n,4] int32 (y_a,x_a,y_q,x_q) in anchor order, idx, d2, xyz_a, xyz_q)."""
    xyz_a, yx_a = lift(depth_a, pix_a, K_a, pose_aq)
    xyz_q, yx_q = lift(depth_q, pix_q, K_q)
    idx, d2 = nearest(xyz_a, xyz_q)
    k = keep(d2, threshold) & (idx >= 0)
    corrs = np.concatenate([yx_a[k], yx_q[idx[k]]], axis=1).astype(np.int32) if k.any() else np.zeros((0, 4), dtype=np.int32)
    return dict(corrs=corrs, idx=idx, d2=d2, xyz_a=xyz_a, xyz_q=xyz_q)


def _draw(n, k):
    return torch.multinomial(torch.ones(n, dtype=float), k, replacement=False)


def pcd_correspondences(feats1, feats2, threshold, max_corrs):
    """The reference's routine of that name on the restatement: the draws are its calls in its order (global CPU generator)."""
    f1, f2 = np.asarray(feats1, dtype=np.float64), np.asarray(feats2, dtype=np.float64)
    i1, i2 = np.arange(f1.shape[0]), np.arange(f2.shape[0])
    if f1.shape[0] >= SAMPLE:
        i1 = i1[_draw(f1.shape[0], SAMPLE).numpy()]
        f1 = f1[i1]
    if f2.shape[0] >= SAMPLE:
        i2 = i2[_draw(f2.shape[0], SAMPLE).numpy()]
        f2 = f2[i2]
    idx, d2 = nearest(f1, f2)
    valid = np.nonzero(keep(d2, threshold))[0]
    i1, i2 = i1[valid], i2[idx[valid]]
    if valid.shape[0] > max_corrs:
        ch = _draw(valid.shape[0], max_corrs).numpy()
        i1, i2 = i1[ch], i2[ch]
    return torch.as_tensor(i1, dtype=torch.int64), torch.as_tensor(i2, dtype=torch.int64)


# ------------------------------------------------------------------------------------------------------------------ golden fixtures
# name -> (numpy seed, n1, n2, threshold, max_corrs, torch seed).  tools/gen_goldens.py `gt_corrs` runs the reference on golden_clouds()
# and records its results; the tests regenerate the same clouds from the seed, so a 20 000-point fixture stores no points.
GOLDEN_CASES = {
    "small": (11, 3000, 2500, 0.002, 10000, 101),             # both sides below 20 000, no draw at all
    "exact20000": (12, 20000, 700, 0.002, 10000, 102),        # n1 == 20000 exactly: the >= draw, against a small n2
    "overmax": (13, 4000, 3500, 0.004, 600, 103),             # more kept rows than max_corrs: the final draw
    "nokeep": (14, 500, 400, 0.0005, 10000, 104),             # no kept row
    "single": (15, 1, 1, 0.002, 10000, 105),                  # a single point on each side
}


def golden_clouds(name):
    """(feats1 [n1,3], feats2 [n2,3]) float64 metres: points on a bumpy sheet 0.8 m from the camera about 1 mm apart, the second cloud
    the first one's surface sampled elsewhere and moved by a fraction of a millimetre - so that some rows fall inside the threshold
    and some outside, as on a real pair.  Only numpy's seeded generator and +, -, *, / are used besides sin / cos on the grid."""
    seed, n1, n2 = GOLDEN_CASES[name][:3]
    rng = np.random.default_rng(seed)

    def sheet(n, shift):
        u, v = rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n)
        z = 0.8 + 0.01 * np.sin(u * 40.0) + 0.008 * np.cos(v * 55.0)
        return np.stack([u + shift[0], v + shift[1], z + shift[2]], axis=1)
    if name == "nokeep":
        return sheet(n1, (0.0, 0.0, 0.0)), sheet(n2, (0.0, 0.0, 0.05))
    if name == "single":
        p = sheet(1, (0.0, 0.0, 0.0))
        return p, p + np.array([[0.0005, 0.0, 0.0]])
    return sheet(n1, (0.0, 0.0, 0.0)), sheet(n2, (0.0002, -0.0001, 0.0001))
