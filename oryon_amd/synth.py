"""Synthetic rigid RGB-D pair generator (descriptors given), used by bench.py, the tests and the
golden generator.  It follows the recipe the reference uses to build ground-truth correspondences
for its fixed test splits (scripts/data/make_nocs_test.py:223-234: lift anchor depth, transform,
re-project into the query view), but on closed-form inputs so nothing has to be shipped:

  anchor depth   D_a(y,x) = 800 + 60 sin(x/9) + 40 cos(y/7)            [mm]
  intrinsics     fx = fy = 1.25 W, cx = W/2, cy = H/2
  motion         rotation about the anchor cloud's centroid, axis uniform on S^2, angle U(0,20 deg),
                 translation U(-50,50)^3 mm
  descriptors    F_a ~ N(0,1);  F_q ~ N(0,1) then F_q[:, v, u] = F_a[:, y, x] + 0.05 N(0,1) at the
                 re-projected pixel (u,v) of every anchor pixel (last writer in row-major order wins)
  query depth    D_q[v,u] = z_q of the winning anchor pixel, 0 elsewhere
  masks          mask_a = centred square of side H/2 ; mask_q = D_q > 0

Everything is deterministic given (index, H, W, C) on a given device type.
"""
from __future__ import annotations

import math
from typing import Dict

import torch


def intrinsics(H: int, W: int) -> torch.Tensor:
    K = torch.zeros(3, 3, dtype=torch.float64)
    K[0, 0] = K[1, 1] = 1.25 * W
    K[0, 2] = W / 2.0
    K[1, 2] = H / 2.0
    K[2, 2] = 1.0
    return K


def _rotation(axis: torch.Tensor, angle: float) -> torch.Tensor:
    a = axis / axis.norm()
    Kx = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def smooth_field(index: int, H: int, W: int, C: int, dev: torch.device, salt: int = 0) -> torch.Tensor:
    """[C, H*W] rank-8 descriptor field (constant, x, y, xy and four slow sinusoids with random per-channel coefficients): neighbouring
    pixels are nearly parallel, so every pixel has many near-ties in cosine - what a decoder's smooth output looks like and what no
    6- or 8-bit screen can separate (the `hard_descriptors` workload of bench.py uses the same basis)."""
    g = torch.Generator(device=dev)
    g.manual_seed(9000 + 2 * index + salt)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
    coef = torch.stack([torch.ones_like(xx), xx, yy, xx * yy, torch.sin(3 * xx), torch.cos(3 * yy), torch.sin(7 * yy), torch.cos(5 * xx)])
    basis = torch.randn((C, coef.shape[0]), generator=g, device=dev)
    return (basis @ coef.reshape(coef.shape[0], H * W)).contiguous()


def _pair_geometry(index: int, H: int, W: int):
    """The closed-form geometry of pair `index`: (R, t, c, D_a [H,W], K, winner [HW] = the anchor pixel whose re-projection owns each
    query pixel or -1, hit = winner >= 0, D_q [HW])."""
    g = torch.Generator(device="cpu")
    g.manual_seed(1000 + index)
    axis = torch.randn(3, generator=g, dtype=torch.float64)
    angle = float(torch.rand(1, generator=g, dtype=torch.float64)) * math.radians(20.0)
    t = (torch.rand(3, generator=g, dtype=torch.float64) * 100.0 - 50.0)
    R = _rotation(axis, angle)

    ys = torch.arange(H, dtype=torch.float64)
    xs = torch.arange(W, dtype=torch.float64)
    D_a = 800.0 + 60.0 * torch.sin(xs / 9.0)[None, :] + 40.0 * torch.cos(ys / 7.0)[:, None]
    K = intrinsics(H, W)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    X = (xs[None, :] - cx) * D_a / fx
    Y = (ys[:, None] - cy) * D_a / fy
    P_a = torch.stack((X, Y, D_a), dim=-1).reshape(-1, 3)
    c = P_a.mean(0)
    P_q = (P_a - c) @ R.T + c + t
    u = torch.round(P_q[:, 0] * fx / P_q[:, 2] + cx).long()
    v = torch.round(P_q[:, 1] * fy / P_q[:, 2] + cy).long()
    inside = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (P_q[:, 2] > 0)
    src = torch.arange(H * W)[inside]
    tgt = (v * W + u)[inside]
    # last writer (largest row-major source index) wins, deterministically
    winner = torch.full((H * W,), -1, dtype=torch.long)
    winner.scatter_reduce_(0, tgt, src, reduce="amax", include_self=True)
    hit = winner >= 0
    D_q = torch.zeros(H * W, dtype=torch.float64)
    D_q[hit] = P_q[winner[hit], 2]

    return R, t, c, D_a, K, winner, hit, D_q


def make_pair(index: int, H: int, W: int, C: int, device: str = "cpu", noise: float = 0.05,
              feat_dtype: torch.dtype = torch.float32, smooth: float = 0.0) -> Dict[str, torch.Tensor]:
    """One synthetic pair.  Returns feat_a/feat_q [C,H,W], mask_a/mask_q [H,W] int32,
    depth_a/depth_q [H,W] fp32 (mm), camera [3,3] fp64, sizes (H,W), pose [4,4] fp64 (metres,
    maps anchor-camera points to query-camera points).
    smooth > 0: the Gaussian descriptors become `smooth` x N(0,1) noise on top of rank-8 smooth fields (one for the anchor map, another
    for the query background); the re-projected query pixels still carry their anchor pixel's descriptor + `noise` x N(0,1), so the
    geometry (and the ground-truth pose) is unchanged while every anchor now has a crowd of near-ties around its true match."""
    dev = torch.device(device)
    R, t, c, D_a, K, winner, hit, D_q = _pair_geometry(index, H, W)

    gd = torch.Generator(device=dev)
    gd.manual_seed(7000 + index)
    feat_a = torch.randn(C, H * W, generator=gd, device=dev, dtype=torch.float32)
    feat_q = torch.randn(C, H * W, generator=gd, device=dev, dtype=torch.float32)
    pert = torch.randn(C, int(hit.sum()), generator=gd, device=dev, dtype=torch.float32) * noise
    if smooth > 0.0:
        feat_a = smooth_field(index, H, W, C, dev, 0) + smooth * feat_a
        feat_q = smooth_field(index, H, W, C, dev, 1) + smooth * feat_q
    hit_d = hit.to(dev)
    win_d = winner[hit].to(dev)
    feat_q[:, hit_d] = feat_a[:, win_d] + pert

    mask_a = torch.zeros(H, W, dtype=torch.int32)
    h0, w0 = H // 4, W // 4
    mask_a[h0:h0 + H // 2, w0:w0 + W // 2] = 1
    mask_q = (D_q > 0).reshape(H, W).to(torch.int32)

    pose = torch.eye(4, dtype=torch.float64)
    pose[:3, :3] = R
    pose[:3, 3] = (c - R @ c + t) / 1000.0
    return dict(
        feat_a=feat_a.reshape(C, H, W).to(feat_dtype), feat_q=feat_q.reshape(C, H, W).to(feat_dtype),
        mask_a=mask_a.to(dev), mask_q=mask_q.to(dev),
        depth_a=D_a.to(torch.float32).to(dev), depth_q=D_q.reshape(H, W).to(torch.float32).to(dev),
        camera=K, sizes=(H, W), pose=pose,
    )


def make_batch(first_index: int, B: int, H: int, W: int, C: int, device: str = "cpu") -> Dict[str, object]:
    """B pairs stacked: feat_* [B,C,H,W], mask_* [B,H,W], depth_* [B,H,W], camera [B,3,3], pose [B,4,4]."""
    items = [make_pair(first_index + i, H, W, C, device) for i in range(B)]
    out: Dict[str, object] = {}
    for k in ("feat_a", "feat_q", "mask_a", "mask_q", "depth_a", "depth_q", "camera", "pose"):
        out[k] = torch.stack([it[k] for it in items])
    out["sizes"] = (H, W)
    return out


def pair_rgb(index: int, H: int, W: int):
    """Images for pair `index` (what a network that is being TRAINED on synthetic pairs sees): (rgb_a, rgb_q) [3,H,W] fp32 in [0,1].
    The anchor is a smooth 3-channel texture (smooth_field, squashed by a sigmoid); every query pixel that `_pair_geometry`'s `winner`
    assigns an anchor pixel shows that pixel's colour, the rest another smooth field as background - so corresponding pixels look
    alike, which is what the contrastive loss can learn from."""
    _, _, _, _, _, winner, hit, _ = _pair_geometry(index, H, W)
    cpu = torch.device("cpu")
    rgb_a = torch.sigmoid(smooth_field(index, H, W, 3, cpu, 0))
    rgb_q = torch.sigmoid(smooth_field(index, H, W, 3, cpu, 1))
    rgb_q[:, hit] = rgb_a[:, winner[hit]]
    return rgb_a.reshape(3, H, W).contiguous(), rgb_q.reshape(3, H, W).contiguous()


def pair_gt_corrs(index: int, H: int, W: int, max_corrs: int) -> torch.Tensor:
    """Ground-truth correspondences of pair `index` as the generator itself made them: [n,4] int64 rows (y_a, x_a, y_q, x_q), one per
    query pixel (y_q, x_q) that carries the descriptor of its winning anchor pixel (y_a, x_a) with the anchor pixel inside mask_a, in
    H x W pixels.  More than max_corrs candidates are thinned to max_corrs by a permutation seeded with the index (sorted back into
    row-major order), as the reference's loaders sample `dataset.max_corrs` of a pair's correspondences; n can be smaller."""
    _, _, _, _, _, winner, hit, _ = _pair_geometry(index, H, W)
    tgt = torch.nonzero(hit).flatten()
    src = winner[tgt]
    ya, xa = src // W, src % W
    h0, w0 = H // 4, W // 4
    inside = (ya >= h0) & (ya < h0 + H // 2) & (xa >= w0) & (xa < w0 + W // 2)
    tgt, ya, xa = tgt[inside], ya[inside], xa[inside]
    corrs = torch.stack([ya, xa, tgt // W, tgt % W], dim=1)
    if corrs.shape[0] > max_corrs:
        g = torch.Generator(device="cpu")
        g.manual_seed(5000 + index)
        keep = torch.randperm(corrs.shape[0], generator=g)[:max_corrs].sort().values
        corrs = corrs[keep]
    return corrs


# ------------------------------------------------------------------------------------------------ VSD fixtures (closed form, no RNG)
# Meshes in millimetres, poses in metres, a 640 x 480 camera: what tools/gen_goldens.py `vsd` feeds to the reference's evaluator and
# what tests/test_vsd.py / tests/test_gpu_vsd.py rebuild.  Only +, -, *, / and sqrt are used for the meshes (correctly rounded
# everywhere); the poses use sin / cos, so the golden file stores them and the tests read them from there.
def icosphere(level: int, radius: float = 60.0):
    """(verts [V,3] float64, faces [F,3] int32): an icosahedron subdivided `level` times, vertices pushed onto the sphere; 20 * 4^level
    faces, outward winding."""
    import numpy as np
    phi = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, phi, 0), (1, phi, 0), (-1, -phi, 0), (1, -phi, 0), (0, -1, phi), (0, 1, phi), (0, -1, -phi), (0, 1, -phi),
         (phi, 0, -1), (phi, 0, 1), (-phi, 0, -1), (-phi, 0, 1)]
    verts = [np.asarray(p, dtype=np.float64) / np.sqrt(1.0 + phi * phi) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nxt = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[key[0]] + verts[key[1]]
                verts.append(m / np.sqrt(np.dot(m, m)))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    return np.stack(verts) * radius, np.asarray(faces, dtype=np.int32)


def box_mesh(sx: float, sy: float, sz: float, centre=(0.0, 0.0, 0.0)):
    """(verts [8,3] float64, faces [12,3] int32) of an axis-aligned box, outward winding."""
    import numpy as np
    h = np.array([sx, sy, sz]) / 2.0
    verts = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * h + np.asarray(centre, dtype=np.float64)
    faces = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                      [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    return verts, faces


def two_part_mesh():
    """A plate with a post standing on it (two closed boxes, 24 faces): seen from the side the post hides part of the plate."""
    import numpy as np
    v0, f0 = box_mesh(110.0, 110.0, 24.0)
    v1, f1 = box_mesh(28.0, 28.0, 90.0, centre=(20.0, -15.0, 57.0))
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + 8]).astype(np.int32)


def vsd_objects():
    """name -> {'pts' [V,3] float64 mm (the mesh vertices), 'faces' [F,3] int32, 'diameter' mm}."""
    import numpy as np
    out = {}
    for name, (v, f) in (("ico2", icosphere(2)), ("ico3", icosphere(3)), ("box", box_mesh(120.0, 90.0, 60.0)), ("twopart", two_part_mesh())):
        d = v[:, None, :] - v[None, :, :]
        out[name] = {"pts": v, "faces": f, "diameter": float(np.sqrt((d * d).sum(-1).max()))}
    return out


VSD_H, VSD_W = 480, 640
VSD_K = ((591.0125, 0.0, 322.525), (0.0, 590.16775, 244.11084), (0.0, 0.0, 1.0))
VSD_CLS = ("ico2", "ico3", "box", "twopart", "box", "ico3", "twopart", "box")
VSD_FAILURES = (6,)


def vsd_poses():
    """(gt [8,4,4], pred [8,4,4]) float64, metres: exact, a few mm / degrees off, grossly wrong, behind the camera (pair 5)."""
    import numpy as np

    def pose(axis, deg, t):
        a = np.asarray(axis, dtype=np.float64)
        a = a / np.sqrt(np.dot(a, a))
        Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        th = np.deg2rad(deg)
        P = np.eye(4)
        P[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)
        P[:3, 3] = t
        return P
    gt = [pose((1, 2, 3), 20.0, (0.010, -0.020, 0.800)), pose((0, 1, 0), 35.0, (-0.030, 0.015, 0.900)),
          pose((1, 1, 0), 40.0, (0.020, 0.010, 0.750)), pose((1, 0.2, 0), 115.0, (0.000, 0.000, 0.850)),
          pose((0, 1, 1), 25.0, (-0.040, -0.030, 0.950)), pose((1, 0, 0), 10.0, (0.030, 0.020, 0.700)),
          pose((1, 0.2, 0), 100.0, (0.010, 0.010, 0.900)), pose((2, 1, 0), 50.0, (0.000, -0.010, 0.800))]
    err = [np.eye(4), pose((0, 0, 1), 2.0, (0.003, -0.002, 0.004)), pose((1, 0, 0), 3.0, (0.002, 0.003, -0.005)),
           pose((0, 1, 0), 2.0, (-0.004, 0.001, 0.006)), pose((1, 1, 1), 60.0, (0.100, -0.050, 0.080)), np.eye(4),
           pose((0, 0, 1), 1.0, (0.001, 0.001, 0.001)), pose((0, 1, 0), 4.0, (0.001, -0.002, 0.012))]
    pred = []
    for g_, e_ in zip(gt, err):
        p = g_.copy()
        p[:3, :3] = e_[:3, :3] @ g_[:3, :3]
        p[:3, 3] = g_[:3, 3] + e_[:3, 3]
        pred.append(p)
    pred[5][2, 3] = -0.700                                  # behind the camera: nothing is rendered
    return np.stack(gt), np.stack(pred)


def vsd_test_depth(depth_gt):
    """The test depth image [H,W] float32 (mm) of a pair from the rasterised ground-truth depth: the object's surface moved by a
    sin-shaped offset of up to +-20 mm (quantised to 1/8 mm; both sides of delta = 15 occur), a smooth background plane elsewhere,
    an occluder patch in front and a hole of zeros."""
    import numpy as np
    H, W = depth_gt.shape
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    off = np.round(20.0 * np.sin(c / 7.0 + r / 11.0) * 8.0) / 8.0
    d = np.where(depth_gt > 0, depth_gt.astype(np.float64) + off, 1500.0 + 0.25 * c + 0.125 * r)
    d[H * 5 // 12:H * 13 // 24, W * 15 // 32:W * 33 // 64] = 300.0
    d[H * 23 // 48:H * 7 // 12, W * 33 // 64:W * 35 // 64] = 0.0
    return d.astype(np.float32)
