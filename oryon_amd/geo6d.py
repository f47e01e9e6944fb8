"""Drop-in counterpart of the reference's utils/geo6d.py: `best_fit_transform` and `best_fit_transform_with_RANSAC` (lines 40-120),
`best_fit_transform_icp` and `icp` (lines 122-208), same names, argument order and defaults, numpy in / numpy out.

    from oryon_amd.geo6d import best_fit_transform_with_RANSAC      # instead of: from utils.geo6d import ...

The arithmetic runs in liboryon_hip.so (csrc/ransac.hip: every hypothesis of a call is scored in ONE launch); this module only
moves the arrays and keeps numpy's global generator where the reference leaves it.  `icp` and `best_fit_transform_icp` run in
csrc/icp.hip (ops.icp_refine: float64 throughout, the clouds need not be of equal length); `icp_point_to_plane`, which the reference
does not have, runs point-to-plane ICP of a cloud onto a depth map (csrc/icp_plane.hip, ops.icp_plane_refine); `spectral_pose`, which
the reference does not have either, is the per-sample facade of the spectral solver (csrc/spectral.hip).  The points are handed to the kernel as
float32 (what pipeline.py:459-463 passes); fits and the inlier test are float64, as numpy computes them for float64 input.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops

MAX_ROWS = 2048          # oryon_ransac_register: rows per pair


def _as_points(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    assert x.ndim == 2 and x.shape[1] == 3, "points are [n, 3]"
    return x


def _device_rows(A: np.ndarray, B: np.ndarray, device):
    n = A.shape[0]
    if n > MAX_ROWS:
        raise ValueError(f"at most {MAX_ROWS} correspondences per call ({n} given)")
    n_cap = max(4, n)
    src = torch.zeros((1, n_cap, 3), dtype=torch.float32, device=device)
    tgt = torch.zeros((1, n_cap, 3), dtype=torch.float32, device=device)
    src[0, :n] = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32))
    tgt[0, :n] = torch.from_numpy(np.ascontiguousarray(B, dtype=np.float32))
    return src, tgt, torch.tensor([n], dtype=torch.int32, device=device)


def best_fit_transform(A, B, *, device="cuda") -> np.ndarray:
    """utils/geo6d.py:40-73: least-squares rigid transform of A onto B, [3,4] float64 (hypothesis 0 of the RANSAC kernel)."""
    A, B = _as_points(A), _as_points(B)
    assert A.shape == B.shape and A.shape[0] >= 1
    if A.shape[0] < 4:                           # the kernel wants four rows; repeating every row changes neither means nor rotation
        A, B = np.tile(A, (4, 1)), np.tile(B, (4, 1))
    src, tgt, n = _device_rows(A, B, device)
    # one iteration = the fit over all rows; a threshold nothing exceeds and a fraction nothing reaches: no refit, the fit as it is
    out = ops.ransac_register(src, tgt, n, max_iter=1, match_err=1e30, fix_percent=2.0,
                              sample_idx=torch.zeros((1, 1, 4), dtype=torch.int32, device=src.device))
    return out["T"][0, :3, :].double().cpu().numpy()


def best_fit_transform_with_RANSAC(A, B, max_iter=20, match_err=0.015, fix_percent=0.7, *, sample_idx: Optional[np.ndarray] = None,
                                   device="cuda") -> np.ndarray:
    """utils/geo6d.py:75-120.  Without `sample_idx` ([max_iter, 4] row indices) the draws come from numpy's global generator exactly
    as the reference makes them - one bulk randint gives the rows of its per-iteration calls - and the generator is left in the
    state the reference leaves it in: after an exit at iteration k only k draws have been consumed."""
    A, B = _as_points(A), _as_points(B)
    assert A.shape == B.shape
    n = A.shape[0]
    max_iter = int(max_iter)
    if n < 4 or max_iter <= 0:                   # geo6d.py:79-80 (and a loop that never runs): zeros, no draw
        return np.zeros((3, 4), dtype=np.float32)
    state = None
    if sample_idx is None:
        state = np.random.get_state()
        sample_idx = np.random.randint(0, n, (max_iter, 4))
    idx = torch.from_numpy(np.ascontiguousarray(np.asarray(sample_idx).reshape(1, max_iter, 4), dtype=np.int32))
    src, tgt, nn = _device_rows(A, B, device)
    out = ops.ransac_register(src, tgt, nn, max_iter=max_iter, match_err=float(match_err), fix_percent=float(fix_percent),
                              sample_idx=idx.to(src.device))
    if state is not None and int(out["exited"][0]) == 1:
        k = int(out["winner"][0])
        np.random.set_state(state)
        if k > 0:
            np.random.randint(0, n, (k, 4))
    return out["T"][0, :3, :].double().cpu().numpy()


def spectral_pose(pcd_a, pcd_q, device="cuda", **cfg) -> torch.Tensor:
    """The per-sample facade of the spectral solver (test.solver = spectral), shaped like pointdsc.get_pointdsc_pose: pcd_a, pcd_q
    [N,3] corresponding points (metres) -> [4,4] fp32 on the CPU.  No weights, no random numbers (csrc/spectral.hip); cfg: the fields of
    oryon_spectral_config_t, whose defaults (ops.SPECTRAL_DEFAULTS) are object-scale and come from a synthetic experiment only.  Fewer
    than int(1 / ratio) points give no seed: the identity, as the batched route reports with ORYON_PAIR_NO_CORR."""
    A, B = _as_points(pcd_a), _as_points(pcd_q)
    assert A.shape == B.shape
    n = A.shape[0]
    if n > MAX_ROWS:
        raise ValueError(f"at most {MAX_ROWS} correspondences per call ({n} given)")
    n_cap = ops.round_up(max(n, 1), 128)
    src = torch.zeros((1, n_cap, 3), dtype=torch.float32, device=device)
    tgt = torch.zeros((1, n_cap, 3), dtype=torch.float32, device=device)
    src[0, :n] = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32))
    tgt[0, :n] = torch.from_numpy(np.ascontiguousarray(B, dtype=np.float32))
    out = ops.spectral_register(src, tgt, torch.tensor([n], dtype=torch.int32, device=device), **cfg)
    return out["T"][0].cpu()


def _cloud(x: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))[None].to(device)


def best_fit_transform_icp(A, B, *, device="cuda") -> np.ndarray:
    """utils/geo6d.py:122-155: least-squares rigid transform of A onto B (row i of A corresponds to row i of B), [4,4] float64."""
    A, B = _as_points(A), _as_points(B)
    assert A.shape == B.shape and A.shape[0] >= 3, "two [n,3] arrays of one length, n >= 3"
    dev = torch.device(device)
    out = ops.icp_best_fit(_cloud(A, dev), _cloud(B, dev), torch.tensor([A.shape[0]], dtype=torch.int32, device=dev))
    T = np.identity(4)
    T[:3, :] = out["T64"][0].cpu().numpy()
    return T


def icp(A, B, init_pose=None, max_iterations=20, tolerance=0.001, *, max_dist=float("inf"), device="cuda") -> np.ndarray:
    """utils/geo6d.py:157-208: iterative closest point of A [n,3] onto B [m,3] from init_pose ([4,4], None = identity) -> [3,4] float64.
    The clouds need not be of equal length; max_dist drops source rows further than that from the target (inf: none, the reference).
    init_pose reaches the kernel as float32, as the solvers' poses do; the result is the composed T_K of the definition
    (include/oryon_hip.h, oryon_icp_refine), which the reference's closing fit of A onto the moved cloud equals to rounding."""
    A, B = _as_points(A), _as_points(B)
    dev = torch.device(device)
    T0 = np.eye(4, dtype=np.float32) if init_pose is None else np.asarray(init_pose, dtype=np.float32).reshape(4, 4)
    if A.shape[0] < 3 or B.shape[0] == 0:                  # the definition: such a pair returns T_0
        return T0[:3, :].astype(np.float64)
    out = ops.icp_refine(_cloud(A, dev), _cloud(B, dev), torch.tensor([A.shape[0]], dtype=torch.int32, device=dev),
                         torch.tensor([B.shape[0]], dtype=torch.int32, device=dev), torch.from_numpy(np.ascontiguousarray(T0))[None].to(dev),
                         max_iter=int(max_iterations), tolerance=float(tolerance), max_dist=float(max_dist))
    return out["T64"][0].cpu().numpy()


def icp_point_to_plane(A, depth_mm, mask, K, init_pose=None, max_iterations=20, tolerance=1e-5, *, max_dist=0.02, normal_jump=0.02,
                       device="cuda") -> np.ndarray:
    """Point-to-plane ICP of the cloud A [n,3] (metres) onto a depth map: depth_mm [H,W] millimetres, mask [H,W] (1 = object), K the
    [3,3] intrinsics; from init_pose ([4,4], None = identity) -> [3,4] float64.  Projective association against the map's own normals
    (include/oryon_hip.h, oryon_icp_plane_refine; csrc/icp_plane.hip); max_dist and normal_jump in metres.  init_pose and K reach the
    kernel as float32 values, as the solvers' poses and the pipeline's intrinsics do.  The reference has no counterpart."""
    A = _as_points(A)
    dev = torch.device(device)
    T0 = np.eye(4, dtype=np.float32) if init_pose is None else np.asarray(init_pose, dtype=np.float32).reshape(4, 4)
    depth_mm, mask = np.asarray(depth_mm), np.asarray(mask)
    assert depth_mm.ndim == 2 and mask.shape == depth_mm.shape, "depth_mm and mask are [H, W]"
    if A.shape[0] < 6:                                      # the definition: such a pair returns T_0
        return T0[:3, :].astype(np.float64)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt))[None].to(dev)
    cam9 = np.asarray(K, dtype=np.float32).reshape(9).astype(np.float64)
    out = ops.icp_plane_refine(_cloud(A, dev), torch.tensor([A.shape[0]], dtype=torch.int32, device=dev), t(depth_mm, np.float32),
                               t(mask == 1, np.int32), t(cam9, np.float64), t(T0, np.float32), max_iter=int(max_iterations),
                               tolerance=float(tolerance), max_dist=float(max_dist), normal_jump=float(normal_jump))
    return out["T64"][0].cpu().numpy()


def pose_depth_score(A, depth_mm, mask, K, poses, tol=0.01, *, device="cuda") -> dict:
    """How well the depth map agrees with each candidate pose of the cloud A [n,3] (metres): depth_mm [H,W] millimetres, mask [H,W]
    (1 = object), K the [3,3] intrinsics, poses [k,4,4] (or one [4,4]), tol in metres -> dict(counts [k,7] int32 - rows BEHIND the
    camera, OUTSIDE the map, on a pixel of UNKNOWN depth, OCCLUDED, in VIOLATION of free space, on the surface but OFF the object, and
    HITs - score [k] float64 = counts[:, 6] / max(n, 1), best = the candidate with the most hits (ties: the fewest BEHIND + VIOLATION +
    OFF, then the first)).  The definition is include/oryon_hip.h's, oryon_pose_verify (csrc/pose_verify.hip); it needs no ground truth
    and no mesh.  poses and K reach the kernel as float32 values, as the solvers' poses and the pipeline's intrinsics do.  The
    reference has no counterpart."""
    A = _as_points(A)
    dev = torch.device(device)
    P = np.asarray(poses, dtype=np.float32)
    P = P.reshape(1, 4, 4) if P.ndim == 2 else P
    assert P.ndim == 3 and P.shape[1:] == (4, 4) and P.shape[0] >= 1, "poses are [k, 4, 4]"
    depth_mm, mask = np.asarray(depth_mm), np.asarray(mask)
    assert depth_mm.ndim == 2 and mask.shape == depth_mm.shape, "depth_mm and mask are [H, W]"
    n = A.shape[0]
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt))[None].to(dev)
    cam9 = np.asarray(K, dtype=np.float32).reshape(9).astype(np.float64)
    src = _cloud(A, dev) if n > 0 else torch.zeros((1, 1, 3), dtype=torch.float64, device=dev)      # a capacity of one row, none in use
    out = ops.pose_verify(src, torch.tensor([n], dtype=torch.int32, device=dev), t(depth_mm, np.float32), t(mask == 1, np.int32),
                          t(cam9, np.float64), t(P, np.float32), tol=float(tol))
    return dict(counts=out["counts"][0].cpu().numpy(), score=out["score"][0].cpu().numpy(), best=int(out["best"][0]))
