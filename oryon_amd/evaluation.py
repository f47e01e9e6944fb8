"""Pose-accuracy metrics and the prediction CSV of the reference's test loop, restated (CPU / numpy; off the throughput
path - SURVEY.md §8f-3):

    compute_add / compute_adds     utils/metrics.py:194-220 (+ np_transform_pcd utils/pcd.py:127-133: the reference transforms
                                   the model points in FLOAT16, which must be replicated for 0.1-point parity)
    compute_RT_distances           utils/metrics.py:222-259 (degrees, centimetres)
    mask_iou                       utils/metrics.py:18-40
    compute_fmr / fmr_from_distances   utils/metrics.py:59-77 (feature-matching recall of ground-truth correspondence sets)
    format_pred_line / read_pred_csv   pipeline.py:490-497 and scripts/evaluation/compute_metrics.py:14-47
    get_symmetry_transformations / format_sym_set   bop_toolkit_lib/misc.py:43-90, :402-411 (the symmetry set of a BOP model)
    mssd_error / mspd_error        bop_toolkit_lib/pose_error.py:370-427 (my_mssd / my_mspd) behind the float16 pose rounding of
                                   utils/evaluator.py:258-265
    Evaluator                      utils/evaluator.py:82-128 (thresholds), :206-288 (register_eval / register_test), :290-338
                                   (register_test_failure), :340-440 (means, LaTeX row, JSON): the accumulator of the test loop;
                                   per-pair errors come from the device (ops.pose_metrics, ops.pose_bop_errors) or from the numpy
                                   restatements in this file.
    rasterize_depth                bop_toolkit_lib/renderer_vispy.py:512-617 (render_object(..)['depth']) replaced by a DEFINED
                                   rasteriser (DESIGN.md "VSD"); the numpy restatement of csrc/vsd.hip, equal to it bit for bit
    vsd_counts_np / vsd_errors     bop_toolkit_lib/pose_error.py:17-93 (vsd, 'step' cost), misc.py:143-163
                                   (depth_im_to_dist_im_fast), visibility.py (bop19)
"""
from __future__ import annotations

import json
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
from scipy.spatial import cKDTree


def transform_points_f16(pcd: np.ndarray, R: np.ndarray, t: np.ndarray) -> np.ndarray:
    """Rigidly move model points with every operand rounded to float16 first (utils/pcd.py:127-133)."""
    return np.dot(np.asarray(pcd.astype(np.float16)), R.astype(np.float16).T) + t.astype(np.float16)


def compute_add(pcd: np.ndarray, pred_pose: np.ndarray, gt_pose: np.ndarray) -> float:
    """ADD: mean distance between corresponding model points under the two poses."""
    a = transform_points_f16(pcd, pred_pose[:3, :3], pred_pose[:3, 3])
    b = transform_points_f16(pcd, gt_pose[:3, :3], gt_pose[:3, 3])
    return np.mean(np.linalg.norm(a - b, axis=1))


def compute_adds(pcd: np.ndarray, pred_pose: np.ndarray, gt_pose: np.ndarray) -> float:
    """ADD-S: mean distance from every predicted model point to its nearest ground-truth model point."""
    a = transform_points_f16(pcd, pred_pose[:3, :3], pred_pose[:3, 3])
    b = transform_points_f16(pcd, gt_pose[:3, :3], gt_pose[:3, 3])
    d, _ = cKDTree(b.astype(np.float64)).query(a.astype(np.float64), k=1)
    return np.mean(d)


def compute_RT_distances(pose1: np.ndarray, pose2: np.ndarray):
    """Rotation angle (degrees) and translation distance (centimetres, poses in metres); batched or not."""
    if pose1 is None or pose2 is None:
        return -1
    if pose1.ndim == 2:
        pose1, pose2 = pose1[None], pose2[None]
    def unit_det(P):
        R = P[:, :3, :3]
        return R / np.cbrt(np.linalg.det(R))[:, None, None]
    R = np.matmul(unit_det(pose1), unit_det(pose2).transpose(0, 2, 1))
    c = np.clip((np.trace(R, axis1=1, axis2=2) - 1) / 2, -1 + 1e-12, 1 - 1e-12)
    theta = np.arccos(c) * 180 / np.pi
    theta[np.isnan(theta)] = 180.0
    shift = np.linalg.norm(pose1[:, :3, 3] - pose2[:, :3, 3], axis=-1) * 100
    return theta, shift


def mask_iou(mask1: np.ndarray, mask2: np.ndarray) -> np.ndarray:
    """IoU of binary masks [B,H,W] = |and| / |or| per sample; like the reference an empty union gives NaN (0/0)
    (utils/metrics.py:18-40)."""
    a, b = mask1.reshape(mask1.shape[0], -1) != 0, mask2.reshape(mask2.shape[0], -1) != 0
    inter, union = (a & b).sum(1).astype(np.float32), (a | b).sum(1).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / union


def fmr_from_distances(dist_pos, dist_th: float, inlier_th: float) -> np.ndarray:
    """utils/metrics.py:72-77 from the distances 0.5 (1 - cos) of the correspondences themselves ([B,N] or [N], numpy or torch - e.g. the
    `d_pos` of losses.FeatureLoss.forward): 1.0 for every set whose share of distances below dist_th exceeds inlier_th."""
    d = np.asarray(dist_pos.detach().cpu().numpy() if hasattr(dist_pos, "detach") else dist_pos)
    if d.ndim == 1:
        d = d[None]
    inlier_ratio = (d < dist_th).astype(float).mean(1)
    return (inlier_ratio > inlier_th).astype(float)


def compute_fmr(feats1, feats2, dist_th: float, inlier_th: float) -> np.ndarray:
    """FMR between two correspondence sets [B,N,D] (or [N,D]) of descriptors (utils/metrics.py:59-77): cosine distance per
    correspondence (torch's cosine_similarity: each norm clamped at 1e-8), then fmr_from_distances."""
    import torch
    import torch.nn.functional as F
    f1, f2 = torch.as_tensor(feats1), torch.as_tensor(feats2)
    assert f1.shape == f2.shape
    if f1.dim() == 2:
        f1, f2 = f1.unsqueeze(0), f2.unsqueeze(0)
    dist_pos = 0.5 * (-1 * F.cosine_similarity(f1, f2, dim=2) + 1)
    return fmr_from_distances(dist_pos, dist_th, inlier_th)


def format_pred_line(id_a: str, id_q: str, iou_a, iou_q, pred_pose: np.ndarray) -> str:
    """`id_a,id_q,<12 floats of pose[:3,:] row-major, space separated>,iou_a,iou_q` (pipeline.py:490-497)."""
    return ",".join([id_a, id_q, " ".join(str(n) for n in pred_pose[:3, :].flatten()), str(iou_a), str(iou_q)]) + "\n"


def read_pred_csv(path: str) -> List[Dict]:
    out = []
    with open(path) as fh:
        for line in fh:
            if not line.strip():
                continue
            id_a, id_q, pose_txt, iou_a, iou_q = line.strip().split(",")
            P = np.eye(4)
            P[:3, :] = np.array([float(x) for x in pose_txt.split(" ")]).reshape(3, 4)
            out.append(dict(id_a=id_a, id_q=id_q, pose=P, iou_a=float(iou_a), iou_q=float(iou_q)))
    return out


def add_accuracy(adds: np.ndarray, diameters: np.ndarray, frac: float = 0.1) -> float:
    """ADD(-S)-0.1d: share of instances whose error is below `frac` of the object diameter."""
    return float(np.mean(np.asarray(adds) < frac * np.asarray(diameters)))


# ------------------------------------------------------------------------------------------------ BOP symmetry sets, MSSD, MSPD
def rotation_matrix3(angle: float, direction) -> np.ndarray:
    """3x3 rotation by `angle` about `direction` (bop_toolkit_lib/transform.py:302-345 without the homogeneous row / point)."""
    sina, cosa = math.sin(angle), math.cos(angle)
    d = np.array(direction[:3], dtype=np.float64)
    d = d / math.sqrt(np.dot(d, d))
    R = np.diag([cosa, cosa, cosa])
    R += np.outer(d, d) * (1.0 - cosa)
    d = d * sina
    R += np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    return R


def get_symmetry_transformations(model_info: Dict, max_sym_disc_step: float = 0.05) -> List[Dict]:
    """The symmetry set of a BOP `models_info.json` entry (bop_toolkit_lib/misc.py:43-90): identity + discrete symmetries, each
    combined with the discretised continuous ones.  The reference's datasets call it with max_sym_disc_step=0.05
    (utils/data/nocs.py:139, utils/data/toyl.py:233)."""
    trans_disc = [{"R": np.eye(3), "t": np.array([[0, 0, 0]]).T}]
    for sym in model_info.get("symmetries_discrete", []):
        m = np.reshape(sym, (4, 4))
        trans_disc.append({"R": m[:3, :3], "t": m[:3, 3].reshape((3, 1))})
    trans_cont = []
    for sym in model_info.get("symmetries_continuous", []):
        axis = np.array(sym["axis"])
        offset = np.array(sym["offset"]).reshape((3, 1))
        steps = int(np.ceil(np.pi / max_sym_disc_step))
        step = 2.0 * np.pi / steps
        for i in range(steps):
            R = rotation_matrix3(i * step, axis)
            trans_cont.append({"R": R, "t": -R.dot(offset) + offset})
    trans = []
    for td in trans_disc:
        if trans_cont:
            for tc in trans_cont:
                trans.append({"R": tc["R"].dot(td["R"]), "t": tc["R"].dot(td["t"]) + tc["t"]})
        else:
            trans.append(td)
    return trans


def format_sym_set(syms: Sequence[Dict]) -> np.ndarray:
    """[N,3,4] array [R|t] of a symmetry set (bop_toolkit_lib/misc.py:402-411)."""
    return np.concatenate([np.stack([np.asarray(s_["R"]) for s_ in syms]), np.stack([np.asarray(s_["t"]) for s_ in syms])], axis=2)


def _pose_f16_mm(pose: np.ndarray):
    """utils/evaluator.py:258-262: the pose rounded to float16, translation times 1000 in float16 arithmetic."""
    p16 = np.asarray(pose).astype(np.float16)
    return p16[:3, :3], np.expand_dims(p16[:3, 3], axis=1) * 1000


def _sym_poses(R_gt, t_gt, syms):
    R = R_gt[None] @ syms[:, :3, :3]
    t = (R_gt[None] @ syms[:, :3, 3, None]) + t_gt[None]
    return R, t


REFERENCE_BOP_POINTS = 3     # bop_toolkit_lib/pose_error.py:345: np_transform slices `pts[:, :3]` on the POINT axis of its [1,N,3]
                             # input, so the reference's my_mssd / my_mspd run over the first three model points; None = all points


def mssd_error(pred_pose: np.ndarray, gt_pose: np.ndarray, pts_mm: np.ndarray, syms: np.ndarray, max_points=REFERENCE_BOP_POINTS) -> float:
    """MSSD of one pair in millimetres (my_mssd on the float16-rounded poses)."""
    pts_mm = pts_mm[:max_points] if max_points else pts_mm
    Re, te = _pose_f16_mm(pred_pose)
    Rg, tg = _pose_f16_mm(gt_pose)
    est = pts_mm @ Re.T + te.T
    Rs, ts = _sym_poses(Rg, tg, syms)
    gts = pts_mm[None] @ np.swapaxes(Rs, -1, -2) + np.swapaxes(ts, -1, -2)
    return float(np.linalg.norm(est[None] - gts, axis=2).max(axis=1).min())


def mspd_error(pred_pose: np.ndarray, gt_pose: np.ndarray, K: np.ndarray, pts_mm: np.ndarray, syms: np.ndarray,
               max_points=REFERENCE_BOP_POINTS) -> float:
    """MSPD of one pair in pixels (my_mspd on the float16-rounded poses)."""
    pts_mm = pts_mm[:max_points] if max_points else pts_mm
    Re, te = _pose_f16_mm(pred_pose)
    Rg, tg = _pose_f16_mm(gt_pose)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)

    def project(R, t):
        x = (pts_mm[None] @ np.swapaxes(R, -1, -2) + np.swapaxes(t, -1, -2)) @ K.T
        return x[:, :, :2] / x[:, :, 2, None]
    Rs, ts = _sym_poses(Rg, tg, syms)
    return float(np.linalg.norm(project(Re[None], te[None]) - project(Rs, ts), axis=2).max(axis=1).min())


# ------------------------------------------------------------------------------------------------ VSD: depth rasteriser, counts, errors
VSD_DELTA = 15.0
VSD_TAUS = np.arange(0.05, 0.51, 0.05)


def rasterize_depth(pose: np.ndarray, K: np.ndarray, verts_mm: np.ndarray, faces: np.ndarray, H: int, W: int) -> np.ndarray:
    """Depth image [H,W] float32 (millimetres, 0 = background) of one mesh at one pose: the numpy restatement of the rasteriser in
    csrc/vsd.hip, operation for operation (DESIGN.md "VSD: the rasterisation definition"), so the two agree bit for bit.
    pose [4,4] (rotation, translation in millimetres), K [3,3] (fx, fy, cx, cy are read), verts_mm [V,3], faces [F,3] zero-based.
    Vertex stage in float32 with left-to-right sums; coordinates snapped to 1/256 pixel (round half to even); int64 edge functions
    with the top-left fill rule at the samples (c + 0.5, r + 0.5); depth = 1 / ((iz0 + l1 (iz1 - iz0)) + l2 (iz2 - iz0)) in float32;
    the nearest surface wins.  Triangles with a vertex at Z <= 0 or further than 2^15 pixels out, or with zero area, are dropped whole."""
    f32 = np.float32
    P = np.asarray(pose, dtype=f32).reshape(4, 4)
    Kc = np.asarray(K, dtype=f32).reshape(3, 3)
    fx, cx, fy, cy = Kc[0, 0], Kc[0, 2], Kc[1, 1], Kc[1, 2]
    v = np.asarray(verts_mm, dtype=f32).reshape(-1, 3)
    F = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    zbuf = np.full((H, W), 0xFFFFFFFF, dtype=np.uint32)
    F = F[((F >= 0) & (F < v.shape[0])).all(axis=1)]
    if F.shape[0] == 0 or v.shape[0] == 0:
        return np.zeros((H, W), dtype=f32)
    with np.errstate(all="ignore"):
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        X = ((P[0, 0] * x + P[0, 1] * y) + P[0, 2] * z) + P[0, 3]
        Y = ((P[1, 0] * x + P[1, 1] * y) + P[1, 2] * z) + P[1, 3]
        Z = ((P[2, 0] * x + P[2, 1] * y) + P[2, 2] * z) + P[2, 3]
        ok = (Z > 0) & (Z <= np.finfo(f32).max)
        su = (fx * (X / Z) + cx) * f32(256.0)
        sv = (fy * (Y / Z) + cy) * f32(256.0)
        ok &= (np.abs(su) <= f32(8388608.0)) & (np.abs(sv) <= f32(8388608.0))
        sx = np.where(ok, np.rint(su), 0).astype(np.int64)
        sy = np.where(ok, np.rint(sv), 0).astype(np.int64)
        iz = f32(1.0) / Z
    assert X.dtype == f32 and su.dtype == f32 and iz.dtype == f32
    F = F[ok[F].all(axis=1)]
    x0, y0, x1, y1, x2, y2 = sx[F[:, 0]], sy[F[:, 0]], sx[F[:, 1]], sy[F[:, 1]], sx[F[:, 2]], sy[F[:, 2]]
    area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    flip = area < 0                                        # orient to positive area: exchange the second and third vertex
    i1, i2 = np.where(flip, F[:, 2], F[:, 1]), np.where(flip, F[:, 1], F[:, 2])
    T = np.stack([F[:, 0], i1, i2], axis=1)[area != 0]
    area = np.abs(area)[area != 0]
    for (a, b, c), A in zip(T, area):
        xs, ys, izs = (sx[a], sx[b], sx[c]), (sy[a], sy[b], sy[c]), (iz[a], iz[b], iz[c])
        cmin, cmax = max((min(xs) + 127) >> 8, 0), min((max(xs) - 128) >> 8, W - 1)
        rmin, rmax = max((min(ys) + 127) >> 8, 0), min((max(ys) - 128) >> 8, H - 1)
        if cmin > cmax or rmin > rmax:
            continue
        px = (np.arange(cmin, cmax + 1, dtype=np.int64) * 256 + 128)[None, :]
        py = (np.arange(rmin, rmax + 1, dtype=np.int64) * 256 + 128)[:, None]
        w, inside = [], True
        for j, k in ((1, 2), (2, 0), (0, 1)):              # w0 faces vertex 0, ...
            dx, dy = xs[k] - xs[j], ys[k] - ys[j]
            e = dx * (py - ys[j]) - dy * (px - xs[j])
            inside = inside & ((e > 0) | ((e == 0) & bool(dy < 0 or (dy == 0 and dx > 0))))
            w.append(e)
        if not inside.any():
            continue
        Af = f32(A)
        l1, l2 = w[1][inside].astype(f32) / Af, w[2][inside].astype(f32) / Af
        inv = (izs[0] + l1 * (izs[1] - izs[0])) + l2 * (izs[2] - izs[0])
        assert inv.dtype == f32
        inside[inside] = inv > 0                           # the rounded sum of a sliver spanning ~2^23 in depth can leave (0, inf): not drawn
        depth = f32(1.0) / inv[inv > 0]
        sub = zbuf[rmin:rmax + 1, cmin:cmax + 1]
        sub[inside] = np.minimum(sub[inside], depth.view(np.uint32))
    zbuf[zbuf == 0xFFFFFFFF] = 0
    return zbuf.view(f32)


def _dist_image(depth: np.ndarray, K: np.ndarray) -> np.ndarray:
    """depth_im_to_dist_im_fast (bop_toolkit_lib/misc.py:129-163): float64, no half-pixel offset."""
    xs, ys = np.meshgrid(np.arange(depth.shape[1]), np.arange(depth.shape[0]))
    pre_x, pre_y = (xs - K[0, 2]) / np.float64(K[0, 0]), (ys - K[1, 2]) / np.float64(K[1, 1])
    return np.sqrt(np.multiply(pre_x, depth) ** 2 + np.multiply(pre_y, depth) ** 2 + depth.astype(np.float64) ** 2)


def vsd_counts_from_depths(depth_est: np.ndarray, depth_gt: np.ndarray, depth_test: np.ndarray, K: np.ndarray, diameter_mm: float,
                           delta: float = VSD_DELTA, taus=VSD_TAUS) -> np.ndarray:
    """(n_union, n_inter, n_cost[tau]...) int32 of one pair from its three depth images: bop19 visibility with the difference taken
    in float32 (visibility.py:35-37, :73-74), 'step' cost on the distances normalised by the diameter (pose_error.py:60-83)."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    d_test, d_est, d_gt = (_dist_image(np.asarray(d, dtype=np.float32), K) for d in (depth_test, depth_est, depth_gt))

    def visible(d_model):
        diff = d_model.astype(np.float32) - d_test.astype(np.float32)
        return np.logical_and(np.logical_or(diff <= np.float32(delta), d_test == 0), d_model > 0)
    vis_gt = visible(d_gt)
    vis_est = np.logical_or(visible(d_est), np.logical_and(vis_gt, d_est > 0))
    inter = np.logical_and(vis_gt, vis_est)
    dists = np.abs(d_gt[inter] - d_est[inter]) / diameter_mm
    return np.array([np.logical_or(vis_gt, vis_est).sum(), inter.sum()] + [(dists >= tau).sum() for tau in taus], dtype=np.int32)


def vsd_counts_np(pred_pose: np.ndarray, gt_pose: np.ndarray, K: np.ndarray, depth_test: np.ndarray, verts_mm: np.ndarray,
                  faces: np.ndarray, diameter_mm: float, delta: float = VSD_DELTA, taus=VSD_TAUS) -> np.ndarray:
    """The counts of one pair (poses [4,4] in metres): float16 pose rounding (utils/evaluator.py:263-266), the two renders, the
    counting - what oryon_vsd_counts does on the device."""
    H, W = depth_test.shape
    renders = []
    for pose in (pred_pose, gt_pose):
        R, t = _pose_f16_mm(pose)
        P = np.eye(4, dtype=np.float32)
        P[:3, :3], P[:3, 3] = R.astype(np.float32), t[:, 0].astype(np.float32)
        renders.append(rasterize_depth(P, K, verts_mm, faces, H, W))
    return vsd_counts_from_depths(renders[0], renders[1], depth_test, K, diameter_mm, delta, taus)


def vsd_errors(counts: np.ndarray) -> np.ndarray:
    """[..., 2 + n_tau] counts -> [..., n_tau] VSD errors (pose_error.py:75-91): (n_cost + n_union - n_inter) / n_union, or 1.0 for
    an empty union."""
    c = np.asarray(counts, dtype=np.int64)
    union, inter, cost = c[..., 0:1], c[..., 1:2], c[..., 2:]
    with np.errstate(invalid="ignore", divide="ignore"):
        e = (cost + (union - inter)) / union.astype(np.float64)
    return np.where(union == 0, 1.0, e)


class Evaluator:
    """The reference's test-time accumulator (utils/evaluator.py): one list per metric, one entry per pair.  compute_vsd=False (the
    default) leaves VSD / AR out, like the reference's own compute_vsd=False; True adds the two lists and the table columns.
    `register_test` takes the per-pair ERRORS of a batch (from the device kernels or the numpy functions above) and applies the
    reference's bookkeeping: zero-pose rule, failed-pose count, ADD(S)-0.1d against the ADD diameter, MSSD / MSPD recall means,
    rotation / translation recalls; `register_test_failure` is the automatic failure of an invalid detection or a matcher that
    returned nothing (pipeline.py:335-350: every score 0).  The validation loop (pipeline.py:196-247) keeps the same lists without the
    `instance_id` / `cls_id` columns: `init_validation`, `register_eval`, `register_valid_failure`; the test methods add the two columns."""

    def __init__(self, exp_tag: str = "", compute_iou: bool = True, compute_vsd: bool = False):
        self.exp_tag = exp_tag
        self.compute_iou = compute_iou
        self.compute_vsd = compute_vsd
        self.vsd_taus = np.arange(0.05, 0.51, 0.05)
        self.vsd_rec = np.arange(0.05, 0.51, 0.05)
        self.vsd_delta = VSD_DELTA
        self.mssd_rec = np.arange(0.05, 0.51, 0.05)
        self.mspd_rec = np.arange(5, 51, 5)
        self.pose_recall_th = [(5, 10), (10, 20), (15, 30)]
        self.metrics: Dict[str, list] = {}
        self.counts: Dict[str, list] = {}
        self.init_test()

    def init_test(self) -> None:
        self.init_validation()
        self.metrics["instance_id"], self.metrics["cls_id"] = [], []

    def init_training(self) -> None:
        """utils/evaluator.py:130-141: training keeps the IoU lists only."""
        self.metrics, self.counts = {}, {}
        if self.compute_iou:
            for k in ("Anchor IoU", "Query IoU", "Mean IoU", "IoU > .25", "IoU > .5", "IoU > .75"):
                self.metrics[k] = []

    def register_train(self, results: Dict, clear: bool = False) -> None:
        """utils/evaluator.py:178-204: the IoUs of one training batch (`results` of FeatureLoss.forward: 'iou_a', 'iou_q' [B])."""
        if clear:
            self.init_training()
        if self.compute_iou:
            import torch
            iou_a, iou_q = (np.asarray(torch.as_tensor(results[k]).detach().cpu().numpy()) for k in ("iou_a", "iou_q"))
            mean = (iou_a + iou_q) / 2.0
            self.metrics["Anchor IoU"].extend(iou_a.tolist())
            self.metrics["Query IoU"].extend(iou_q.tolist())
            self.metrics["Mean IoU"].extend(mean.tolist())
            for k, th in (("IoU > .25", 0.25), ("IoU > .5", 0.5), ("IoU > .75", 0.75)):
                self.metrics[k].extend((mean > th).astype(int).tolist())

    def init_validation(self) -> None:
        """utils/evaluator.py:143-167: the lists of the test run without the `instance_id` / `cls_id` columns."""
        self.init_training()
        for k in ("R error", "T error", "ADD(S)-0.1d") + (("AR", "VSD") if self.compute_vsd else ()) + ("MSSD", "MSPD"):
            self.metrics[k] = []
        for k in ("Missing segm", "Failed pose", "Zero pose"):
            self.counts[k] = []
        for r_th, t_th in self.pose_recall_th:
            self.metrics[f"Recall ({r_th}deg, {t_th}cm)"] = []

    @staticmethod
    def effective_pose(pred_pose: np.ndarray, pred_pose_rel: np.ndarray) -> np.ndarray:
        """utils/evaluator.py:229-231: a relative pose with at most one non-zero entry scores as the identity."""
        return np.eye(4, dtype=pred_pose.dtype) if np.count_nonzero(pred_pose_rel) <= 1 else pred_pose

    def register_test(self, *, pred_pose_rel: np.ndarray, rot_deg: float, trans_cm: float, add_s: float, add_diam: float, mssd_mm: float,
                      mspd_px: float, bop_diam_mm: float, cls_id, instance_id, iou_a: Optional[float] = None,
                      iou_q: Optional[float] = None, vsd_errs: Optional[Sequence[float]] = None) -> None:
        """One pair that went through the registration.  The errors must have been computed on `effective_pose`.  vsd_errs: the
        pair's VSD error per tau (vsd_errors), required with compute_vsd."""
        self.register_eval(pred_pose_rel=pred_pose_rel, rot_deg=rot_deg, trans_cm=trans_cm, add_s=add_s, add_diam=add_diam, mssd_mm=mssd_mm,
                           mspd_px=mspd_px, bop_diam_mm=bop_diam_mm, iou_a=iou_a, iou_q=iou_q, vsd_errs=vsd_errs)
        self.metrics["cls_id"].append(cls_id)
        self.metrics["instance_id"].append(instance_id)

    def register_eval(self, *, pred_pose_rel: np.ndarray, rot_deg: float, trans_cm: float, add_s: float, add_diam: float, mssd_mm: float,
                      mspd_px: float, bop_diam_mm: float, iou_a: Optional[float] = None, iou_q: Optional[float] = None,
                      vsd_errs: Optional[Sequence[float]] = None) -> None:
        """The validation-time registration of one pair (utils/evaluator.py:206-288): register_test without the two id columns."""
        if self.compute_iou:
            mean = (iou_a + iou_q) / 2.0
            self.metrics["Anchor IoU"].append(float(iou_a)); self.metrics["Query IoU"].append(float(iou_q))
            self.metrics["Mean IoU"].append(float(mean))
            for k, th in (("IoU > .25", 0.25), ("IoU > .5", 0.5), ("IoU > .75", 0.75)):
                self.metrics[k].append(int(mean > th))
        self.counts["Missing segm"].append(0)
        self.counts["Failed pose"].append(int((np.asarray(pred_pose_rel) == np.eye(4)).all()))
        self.counts["Zero pose"].append(int(np.count_nonzero(pred_pose_rel) <= 1))
        self.metrics["R error"].append(float(rot_deg))
        self.metrics["T error"].append(float(trans_cm))
        for r_th, t_th in self.pose_recall_th:
            self.metrics[f"Recall ({r_th}deg, {t_th}cm)"].append(float(rot_deg <= r_th and trans_cm <= t_th))
        self.metrics["ADD(S)-0.1d"].append(float(add_s <= add_diam * 0.1))
        mean_mssd, mean_mspd = (mssd_mm < self.mssd_rec * bop_diam_mm).mean(), (mspd_px < self.mspd_rec).mean()
        self.metrics["MSSD"].append(float(mean_mssd))
        self.metrics["MSPD"].append(float(mean_mspd))
        if self.compute_vsd:                               # utils/evaluator.py:283-288: the mean over the tau x recall table
            if vsd_errs is None:
                raise ValueError("Evaluator(compute_vsd=True).register_test needs vsd_errs")
            e = np.asarray(vsd_errs, dtype=np.float64)
            mean_vsd = np.stack([e < rec for rec in self.vsd_rec], axis=1).mean()
            self.metrics["VSD"].append(float(mean_vsd))
            self.metrics["AR"].append(float((mean_mssd + mean_mspd + mean_vsd) / 3.0))

    def register_test_failure(self, *, cls_id, instance_id, iou_a: Optional[float] = None, iou_q: Optional[float] = None) -> None:
        self.register_valid_failure(iou_a=iou_a, iou_q=iou_q)
        self.metrics["cls_id"].append(cls_id)
        self.metrics["instance_id"].append(instance_id)

    def register_valid_failure(self, *, iou_a: Optional[float] = None, iou_q: Optional[float] = None) -> None:
        """utils/evaluator.py:296-328: the automatic failure of a wrong detection, every score 0."""
        for k in ("R error", "T error", "ADD(S)-0.1d", "MSSD", "MSPD") + (("VSD", "AR") if self.compute_vsd else ()):
            self.metrics[k].append(0.0)
        if self.compute_iou:
            self.metrics["Anchor IoU"].append(float(iou_a)); self.metrics["Query IoU"].append(float(iou_q))
            for k in ("Mean IoU", "IoU > .25", "IoU > .5", "IoU > .75"):
                self.metrics[k].append(0.0)
        self.counts["Missing segm"].append(1)
        self.counts["Failed pose"].append(0)
        self.counts["Zero pose"].append(0)
        for r_th, t_th in self.pose_recall_th:
            self.metrics[f"Recall ({r_th}deg, {t_th}cm)"].append(0)

    def get_means(self, cls_id=None) -> Dict[str, float]:
        sel = None if cls_id is None else np.asarray(self.metrics["cls_id"]) == cls_id
        out = {}
        for name, value in self.metrics.items():
            if name not in ("cls_id", "instance_id") and len(value) > 0:
                v = np.asarray(value)
                out[name] = float((v if sel is None else v[sel]).mean())
        return out

    def get_latex_str(self, cls_id=None) -> str:
        """The reference's table row (utils/evaluator.py:404-420; per class :345-355): AR and VSD with compute_vsd, `- & -` without."""
        m = self.get_means(cls_id)
        tag = self.exp_tag if cls_id is None else cls_id
        head = f"{m['AR'] * 100:.1f} & {m['VSD'] * 100:.1f}" if self.compute_vsd else "- & -"
        s_ = f"{tag} & {head} & {m['MSSD'] * 100:.1f} & {m['MSPD'] * 100:.1f} & {m['ADD(S)-0.1d'] * 100:.1f} &"
        s_ += f" {m['Mean IoU'] * 100:.1f} \\\\" if self.compute_iou else " - \\\\"
        return s_ + (" \n" if cls_id is None else "")

    def test_summary(self) -> List[str]:
        return [self.get_latex_str(c) for c in np.unique(self.metrics["cls_id"]).tolist()]

    def save(self, fh) -> None:
        d = dict(self.metrics)
        d.update(self.counts)
        json.dump(d, fh)


def evaluate_batch(evaluator: Evaluator, *, pred_pose_rel: np.ndarray, anchor_pose: np.ndarray, gt_pose: np.ndarray, K: np.ndarray,
                   status: Sequence[int], cls_ids: Sequence, instance_ids: Sequence[str], objects: Dict, iou_a=None, iou_q=None,
                   device: Optional[str] = None, depth: Optional[Sequence[np.ndarray]] = None, validation: bool = False) -> None:
    """What the per-sample loop of FPM_Pipeline.test_step registers for a batch (pipeline.py:313-350): pairs whose status is not
    PAIR_OK are automatic failures (`register_test_failure`), the others are scored on pred_q = pred_pose_rel @ anchor_pose (fp32,
    pipeline.py:320) after the zero-pose rule.  objects[cls_id] = {'pts' [N,3] mm (float64), 'diameter' (BOP, mm), 'syms' [S,3,4]}.
    device: a torch device string -> per-pair errors from the HIP kernels (oryon_pose_metrics, oryon_pose_bop_errors); None -> the
    numpy restatements in this file.
    With evaluator.compute_vsd: depth = one [H,W] test depth image (millimetres) per pair, all of one size, and objects[cls_id] also
    holds 'faces' [F,3] (zero-based indices into 'pts'); VSD comes from oryon_vsd_counts on the device, else from vsd_counts_np.
    validation: register through register_eval / register_valid_failure (the validation loop, pipeline.py:206-243: the same scores without
    the id columns; the evaluator must have been reset with init_validation)."""
    n = len(status)
    vsd = evaluator.compute_vsd
    if vsd and depth is None:
        raise ValueError("evaluate_batch: Evaluator(compute_vsd=True) needs the test depth images (depth=...)")
    rel = np.asarray(pred_pose_rel, dtype=np.float32)
    pred_q = np.matmul(rel, np.asarray(anchor_pose, dtype=np.float32))
    for i in range(n):
        pred_q[i] = Evaluator.effective_pose(pred_q[i], rel[i])
    ok = [i for i in range(n) if int(status[i]) == 0]
    errs = {}
    if ok and device is not None:
        import torch
        from . import ops
        keys = list(dict.fromkeys(cls_ids[i] for i in ok))
        pts_mm = [np.asarray(objects[k]["pts"], dtype=np.float64) for k in keys]
        syms = [np.asarray(objects[k]["syms"], dtype=np.float64) for k in keys]
        po = torch.tensor(np.concatenate(([0], np.cumsum([p_.shape[0] for p_ in pts_mm]))), dtype=torch.int32)
        so = torch.tensor(np.concatenate(([0], np.cumsum([s_.shape[0] for s_ in syms]))), dtype=torch.int32)
        which = torch.tensor([keys.index(cls_ids[i]) for i in ok], dtype=torch.int32)
        pq, gq = torch.from_numpy(pred_q[ok]), torch.from_numpy(np.asarray(gt_pose)[ok])
        met = ops.pose_metrics(pq.to(device), gq.to(device, torch.float32), torch.from_numpy(np.concatenate(pts_mm) / 1000.0).float().to(device),
                               po, which).cpu().numpy()
        bop = ops.pose_bop_errors(pq.to(device), gq.to(device), torch.from_numpy(np.asarray(K, dtype=np.float64)[ok]).to(device),
                                  torch.from_numpy(np.concatenate(pts_mm)).to(device), po, torch.from_numpy(np.concatenate(syms)).to(device),
                                  so, which).cpu().numpy()
        if vsd:
            faces = [np.asarray(objects[k]["faces"]) for k in keys]
            fo = torch.tensor(np.concatenate(([0], np.cumsum([f_.shape[0] for f_ in faces]))), dtype=torch.int32)
            cnt = ops.vsd_counts(pq.to(device), gq.to(device), torch.from_numpy(np.asarray(K, dtype=np.float64)[ok]).to(device),
                                 torch.from_numpy(np.stack([np.asarray(depth[i], dtype=np.float32) for i in ok])).to(device),
                                 torch.from_numpy(np.concatenate(pts_mm)).to(device), torch.from_numpy(np.concatenate(faces)).to(device),
                                 torch.tensor([float(objects[cls_ids[i]]["diameter"]) for i in ok], dtype=torch.float64), po, fo, which,
                                 delta=evaluator.vsd_delta, taus=evaluator.vsd_taus).cpu().numpy()
            vsd_e = vsd_errors(cnt)
        for j, i in enumerate(ok):
            sym = objects[cls_ids[i]]["syms"].shape[0] > 1
            errs[i] = (float(met[j, 2]), float(met[j, 3]), float(met[j, 1] if sym else met[j, 0]), float(bop[j, 0]), float(bop[j, 1]),
                       vsd_e[j] if vsd else None)
    elif ok:
        for i in ok:
            o = objects[cls_ids[i]]
            pts_m = np.asarray(o["pts"]) / 1000.0
            th, sh = compute_RT_distances(pred_q[i], np.asarray(gt_pose[i]))
            add = compute_adds(pts_m, pred_q[i], gt_pose[i]) if o["syms"].shape[0] > 1 else compute_add(pts_m, pred_q[i], gt_pose[i])
            ve = vsd_errors(vsd_counts_np(pred_q[i], gt_pose[i], K[i], np.asarray(depth[i], dtype=np.float32), o["pts"], o["faces"],
                                          float(o["diameter"]), evaluator.vsd_delta, evaluator.vsd_taus)) if vsd else None
            errs[i] = (float(th[0]), float(sh[0]), float(add), mssd_error(pred_q[i], gt_pose[i], o["pts"], o["syms"]),
                       mspd_error(pred_q[i], gt_pose[i], K[i], o["pts"], o["syms"]), ve)
    for i in range(n):
        ia = None if iou_a is None else float(iou_a[i])
        iq = None if iou_q is None else float(iou_q[i])
        ids = {} if validation else dict(cls_id=cls_ids[i], instance_id=instance_ids[i])
        if i not in errs:
            (evaluator.register_valid_failure if validation else evaluator.register_test_failure)(iou_a=ia, iou_q=iq, **ids)
            continue
        o = objects[cls_ids[i]]
        rot, tr, add, ms, mp, ve = errs[i]
        (evaluator.register_eval if validation else evaluator.register_test)(
            pred_pose_rel=rel[i], rot_deg=rot, trans_cm=tr, add_s=add, add_diam=extent_diameter(o["pts"]) / 1000.0, mssd_mm=ms, mspd_px=mp,
            bop_diam_mm=float(o["diameter"]), iou_a=ia, iou_q=iq, vsd_errs=ve, **ids)


def extent_diameter(pts: np.ndarray) -> float:
    """The "ADD diameter" of the reference: the largest side of the model's axis-aligned bounding box (utils/pcd.py:16-20), not the
    BOP diameter; same unit as pts."""
    xyz = np.asarray(pts)[:, :3]
    return float(np.max(xyz.max(axis=0) - xyz.min(axis=0)))
