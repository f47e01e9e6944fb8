"""Test-time counterpart of the reference's FPM_Pipeline (pipeline.py:306-355, 372-472, 490-497).

`Pipeline` offers the same four callables the reference's test loop uses, with the same argument dicts:

    is_detection_valid(results, batch, idx) -> bool
    get_featmap_corrs(batch, net_output, results, idx) -> (corrs | None, pos_a, pos_q)
    get_pose(batch, corrs, idx) -> Tensor[4,4] fp32
    test_step(batch, batch_idx)                       # per-sample loop, host RNG: reference semantics
    test_step_batched(batch, first_pair_index=0)      # same work for the whole batch with no host sync

`test.refine = icp` (absent or `none`: nothing changes) refines every solved pose by ICP of the anchor's object cloud onto the query's
(utils/geo6d.py:157-208 `icp`, csrc/icp.hip) in both routes; flags test.refine_points / refine_max_iter / refine_tolerance /
refine_max_dist.  `test.refine = icp_plane` refines it by point-to-plane ICP of the anchor's object cloud onto the query's DEPTH MAP
(projective association, csrc/icp_plane.hip; no counterpart in the reference): the same flags with defaults of their own
(REFINE_DEFAULTS) and test.refine_normal_jump.

`test.verify = score` (absent or `none`: nothing changes) rates the final pose of every solved pair against the query's depth map
(csrc/pose_verify.hip; no counterpart in the reference): the share of the anchor's object cloud that lands on the object within
test.verify_tol of the measured depth, with no ground truth and no mesh.  `test.verify = guard` (needs a refinement) rates the solver's
pose and the refined one and keeps the refinement only when more of the cloud agrees with it.

`test.mask_clean = largest | area` and / or `test.mask_fill_holes` (absent, `none` and False: nothing changes, no launch, no new key)
cleans every binary mask - predicted or external - before the matcher, a refiner or the verifier uses it (csrc/mask_clean.hip; no
counterpart in the reference): enclosed holes filled, then the largest 8-connected component kept, or every one of at least
test.mask_clean_frac of the largest area.  The thresholded masks stay in the results as `mask_a_raw` / `mask_q_raw`.

and the validation step (pipeline.py:196-247, 579-590):

    on_validation_start(objects=None) / validation_step(batch, batch_idx) -> (loss, log) / on_validation_end() -> dict
    reduce_losses(losses) -> (loss, weighted losses)

and the training step (pipeline.py:100-152, 170-181):

    configure_optimizers() -> ([optimizer], [scheduler]) / training_step(batch, batch_idx) -> (loss, log)

The loss of a training step is differentiable: losses.FeatureLoss carries its own backward pass (csrc/feature_loss_grad.hip), fusion
and decoder - the only trainable modules, net.py:148 - are torch modules under torch autograd.  run_train.py is the loop around it.
Logging (wandb), the dataloaders' augmentations and DDP of the reference are out of scope.  Config flags keep the
names of configs/config.yaml.
"""
from __future__ import annotations

import ctypes
import math
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib, ops
from .engine import MatchPoseConfig, MatchPoseEngine, PAIR_NO_CORR, PAIR_NO_MASK, PAIR_OK, SOLVERS, default_mutual, default_ratio, default_solver, default_subpixel, default_topk
from .geo6d import best_fit_transform_with_RANSAC, spectral_pose
from .pcd import nn_correspondences, nn_correspondences_filtered, nn_correspondences_topk, subpixel_offsets
from .pointdsc import PointDSC, get_pointdsc_pose


REFINEMENTS = ("none", "icp", "icp_plane")
# test.refine_tolerance / refine_max_dist / refine_normal_jump (metres) where the args do not name them.  icp: the reference's.
# icp_plane: design choices, not tuned on data - the 1 mm tolerance of icp stops point-to-plane too early (its mean |r| is a distance
# along the normal, far smaller than a point-to-point distance: fixture 4 of tests/icp_plane_restatement.py stops after two iterations,
# 8.2 degrees off, where 1e-5 takes seven to 0.05 degrees), and the gates are the scale of a solver's error (2 cm) and of a depth step
# between neighbouring pixels that is an edge rather than a slope (2 cm).
REFINE_DEFAULTS = {"icp": dict(tolerance=1e-3, max_dist=float("inf")), "icp_plane": dict(tolerance=1e-5, max_dist=0.02, normal_jump=0.02)}
_default_refine = "none"


def set_default_refine(name: str) -> None:
    """The process-wide default of test.refine: what a Pipeline does when its args name no refinement ('none' unless set).  A driver
    sets it once, before it builds pipelines (run_pose.py --refine does, as --solver does through engine.set_default_solver)."""
    global _default_refine
    if name not in REFINEMENTS:
        raise ValueError(f"Refinement {name} not implemented")
    _default_refine = name


def default_refine() -> str:
    return _default_refine


# test.verify (csrc/pose_verify.hip; no counterpart in the reference): 'score' rates the final pose of every solved pair by how much
# of the anchor's object cloud the query's depth map confirms on the object; 'guard' rates the solver's pose and the refined one and
# keeps the one the measurements agree with more.  A property of the pipeline like test.refine - not a refinement, not a field of
# MatchPoseConfig.  test.verify_tol (metres): how far a moved point may lie from the measured surface and still agree with it.  The
# default is a design choice at the scale of the refiners' gates (REFINE_DEFAULTS: 2 cm), not tuned on data.
VERIFY_MODES = ("none", "score", "guard")
VERIFY_TOL = 0.01
_default_verify = ("none", VERIFY_TOL)


def _check_verify(mode: str, tol: float) -> Tuple[str, float]:
    if mode not in VERIFY_MODES:
        raise ValueError(f"Verification {mode} not implemented")
    tol = float(tol)
    if not tol >= 0.0:
        raise ValueError(f"test.verify_tol must be >= 0 (metres), not {tol}")
    return mode, tol


def set_default_verify(mode: str, tol: float = VERIFY_TOL) -> None:
    """The process-wide default of test.verify / test.verify_tol: what default_args() carries and what a Pipeline does when its args
    name neither (('none', 0.01) unless set).  A driver sets it once, before it builds pipelines (run_pose.py --verify does)."""
    global _default_verify, _latest_verify
    _default_verify = _check_verify(mode, tol)
    _latest_verify = None


def default_verify() -> Tuple[str, float]:
    return _default_verify


# (mode, tol, log) of the latest Pipeline built with test.verify != 'none' since the last set_default_verify.  A driver that cannot
# reach the pipeline another module builds (run_pose.py around run_test.py) reads its summary from here.
_latest_verify: Optional[Tuple[str, float, List[Tuple]]] = None


def _reduce_verify(mode: str, tol: float, log: List[Tuple]) -> Dict:
    """log: per step (status, chosen score, best), each [B] -> the mode, the tolerance, the mean score of the chosen poses over the
    solved pairs and, for 'guard', how many of them kept their refinement.  Reads the device once per step."""
    scores = [float(s) for st, sc, _ in log for s in sc[st == PAIR_OK].cpu().tolist()]
    out = {"verify": mode, "verify_tol": tol, "verify_pairs": len(scores), "verify_score_mean": float(np.mean(scores)) if scores else None}
    if mode == "guard":
        out["verify_refinements_kept"] = int(sum(int((b[st == PAIR_OK] == 1).sum()) for st, _, b in log))
    return out


def verify_summary() -> Dict:
    """Pipeline.verify_summary() of the latest verifying pipeline of this process; {} when there is none."""
    return {} if _latest_verify is None else _reduce_verify(*_latest_verify)


# test.mask_clean / test.mask_clean_frac / test.mask_fill_holes (csrc/mask_clean.hip; no counterpart in the reference): clean every
# binary mask before the matcher, a refiner or the verifier sees it - fill the enclosed holes, then keep the 'largest' 8-connected
# component or every one of at least mask_clean_frac x the largest 'area'.  A property of the pipeline like test.verify - not a field of
# MatchPoseConfig: the engine gets cleaned masks.  The fraction's default is a design choice, not tuned on data.
MASK_CLEAN_MODES = ("none", "largest", "area")
MASK_CLEAN_FRAC = 0.25
_default_mask_clean = ("none", MASK_CLEAN_FRAC, False)


def _check_mask_clean(mode: str, frac: float, fill_holes: bool) -> Tuple[str, float, bool]:
    if mode not in MASK_CLEAN_MODES:
        raise ValueError(f"Mask clean-up {mode} not implemented")
    frac = float(frac)
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f"test.mask_clean_frac must lie in [0, 1], not {frac}")
    return mode, frac, bool(fill_holes)


def set_default_mask_clean(mode: str, frac: float = MASK_CLEAN_FRAC, fill_holes: bool = False) -> None:
    """The process-wide default of test.mask_clean / test.mask_clean_frac / test.mask_fill_holes: what default_args() carries and what
    a Pipeline does when its args name none of them (('none', 0.25, False) unless set).  A driver sets it once, before it builds
    pipelines (run_pose.py --mask-clean does)."""
    global _default_mask_clean, _latest_mask_clean
    _default_mask_clean = _check_mask_clean(mode, frac, fill_holes)
    _latest_mask_clean = None


def default_mask_clean() -> Tuple[str, float, bool]:
    return _default_mask_clean


# (mode, frac, fill_holes, log) of the latest Pipeline built with clean-up active since the last set_default_mask_clean: what a driver
# that cannot reach the pipeline another module builds (run_pose.py around run_test.py) reads its summary from.
_latest_mask_clean: Optional[Tuple[str, float, bool, List[Tensor]]] = None


def _reduce_mask_clean(mode: str, frac: float, fill_holes: bool, log: List[Tensor]) -> Dict:
    """log: the stats [n, 6] (ops.MASK_CLEAN_STATS) of every cleaned batch of masks, on the device -> the flags, how many masks were
    cleaned and the means of their statistics.  The only place that reads them back."""
    out = {"mask_clean": mode, "mask_clean_frac": frac, "mask_fill_holes": fill_holes, "mask_clean_masks": 0}
    rows = torch.cat([s.reshape(-1, len(ops.MASK_CLEAN_STATS)) for s in log]).cpu().numpy().astype(np.int64) if log else np.zeros((0, 6), np.int64)
    out["mask_clean_masks"] = int(rows.shape[0])
    for i, name in enumerate(ops.MASK_CLEAN_STATS):
        if name != "a_max":
            out[f"mask_clean_{name}_mean"] = float(rows[:, i].mean()) if rows.shape[0] else None
    return out


def mask_clean_summary() -> Dict:
    """Pipeline.mask_clean_summary() of the latest cleaning pipeline of this process; {} when there is none."""
    return {} if _latest_mask_clean is None else _reduce_mask_clean(*_latest_mask_clean)


# The log of the latest Pipeline built with test.subpixel (csrc/match_subpix.hip): what a driver that cannot reach the pipeline
# another module builds (run_pose.py around run_test.py) reads its summary from.
_latest_subpixel: Optional[List[Tuple[Tensor, Tensor]]] = None


def _reduce_subpixel(log: List[Tuple[Tensor, Tensor]]) -> Dict:
    """log: per step (flags [n] uint8, offsets [n, 2] fp32) of the rows handed to the lift, on the device -> the rows per flag value
    and the mean |offset| (pixels of the feature map) of the refined rows.  The only place that reads them back."""
    flags = torch.cat([f.reshape(-1) for f, _ in log]).cpu().numpy() if log else np.zeros((0,), np.uint8)
    offs = torch.cat([o.reshape(-1, 2) for _, o in log]).cpu().numpy().astype(np.float64) if log else np.zeros((0, 2))
    out = {"subpixel_rows": int(flags.shape[0])}
    for i, name in enumerate(ops.SUBPIX_FLAGS):
        out[f"subpixel_{name}"] = int((flags == i).sum())
    ref = offs[flags == 0]
    out["subpixel_offset_mean"] = float(np.hypot(ref[:, 0], ref[:, 1]).mean()) if ref.shape[0] else None
    return out


def subpixel_summary() -> Dict:
    """Pipeline.subpixel_summary() of the latest refining pipeline of this process; {} when there is none."""
    return {} if _latest_subpixel is None else _reduce_subpixel(_latest_subpixel)


def default_args(**overrides) -> SimpleNamespace:
    """The hot-path subset of configs/config.yaml (same names, same defaults)."""
    args = SimpleNamespace(
        device="cuda", corrs_device="cpu", seed=1, debug_valid=False,
        dataset=SimpleNamespace(img_size=[224, 224], max_corrs=500),
        model=SimpleNamespace(image_encoder=SimpleNamespace(img_size=[192, 192], out_channels=32)),
        test=SimpleNamespace(mask="predicted", src_sampling=5000, solver=default_solver(), n_corrs=500, dist_th=0.25,
                             mask_threshold=0.5,
                             # test.solver = spectral (csrc/spectral.hip; the reference has no counterpart): the fields of
                             # oryon_spectral_config_t.  Object-scale lengths chosen from one synthetic experiment, not from real data
                             spectral_num_iterations=10, spectral_ratio=0.1, spectral_inlier_threshold=0.01, spectral_sigma_d=0.01,
                             spectral_k=40, spectral_nms_radius=0.02,
                             # test.mutual (csrc/match_mutual.hip; the reference matches in one direction only): keep only the
                             # mutual nearest neighbours (False unless a driver called engine.set_default_mutual).  Read with
                             # getattr(..., False): arg objects without it keep working
                             mutual=default_mutual(),
                             # test.ratio / test.ratio_radius (csrc/match_second.hip; no counterpart in the reference): the ratio
                             # test with an exclusion disc, 0 = off ((0.0, 5) unless a driver called engine.set_default_ratio).  Read
                             # with getattr(..., 0.0 / 5)
                             ratio=default_ratio()[0], ratio_radius=default_ratio()[1],
                             # test.topk / test.topk_radius / test.topk_margin (csrc/match_next.hip; no counterpart in the reference):
                             # up to topk rows per drawn anchor, 1 = off ((1, 5, 0.1) unless a driver called
                             # engine.set_default_topk).  Read with getattr(..., 1 / 5 / 0.1)
                             topk=default_topk()[0], topk_radius=default_topk()[1], topk_margin=default_topk()[2],
                             # test.subpixel / test.subpixel_curv_min / test.subpixel_depth_jump (csrc/match_subpix.hip; no
                             # counterpart in the reference): sub-pixel refinement of the selected rows, off ((False, 1e-4, 0.02)
                             # unless a driver called engine.set_default_subpixel).  Read with getattr(..., False / 1e-4 / 0.02)
                             subpixel=default_subpixel()[0], subpixel_curv_min=default_subpixel()[1],
                             subpixel_depth_jump=default_subpixel()[2],
                             # test.verify / test.verify_tol (csrc/pose_verify.hip; no counterpart in the reference): rate, or
                             # choose between, the poses of a pair against the query's depth map (('none', 0.01) unless a driver
                             # called set_default_verify).  Read with getattr: arg objects without them keep working
                             verify=default_verify()[0], verify_tol=default_verify()[1],
                             # test.mask_clean / test.mask_clean_frac / test.mask_fill_holes (csrc/mask_clean.hip; no counterpart in
                             # the reference): connected-component clean-up of every mask the path uses (('none', 0.25, False) unless
                             # a driver called set_default_mask_clean).  Read with getattr: arg objects without them keep working
                             mask_clean=default_mask_clean()[0], mask_clean_frac=default_mask_clean()[1],
                             mask_fill_holes=default_mask_clean()[2]),
        loss=SimpleNamespace(hard_negatives=True, pos_margin=0.2, neg_margin=0.9, neg_kernel_size=5, mask_type="dice",
                             w={"mask": 1.0, "pos": 0.5, "neg": 0.5}),
        optimization=SimpleNamespace(optim_type="Adam", scheduler_type="cosine", lr=0.001, momentum=0.0, w_decay=0.0005, gamma=0.1),
        training=SimpleNamespace(n_epochs=20, freq_save=5, freq_valid=5),
        # the training augmentations (datasets.py:98-114); read by nothing unless handed to data.DeviceCollate(augs=...)
        augs=SimpleNamespace(rgb=SimpleNamespace(jitter=True, bright=True, hflip=True, vflip=True)),
    )
    for k, v in overrides.items():
        node = args
        parts = k.split(".")
        for p in parts[:-1]:
            node = getattr(node, p)
        setattr(node, parts[-1], v)
    return args


class PrecomputedFeatures:
    """Stand-in for Oryon.forward when descriptors are given: returns the batch's own feature maps / mask logits
    under the output keys of net.py:162-167."""

    def forward(self, batch: Dict) -> Dict[str, Tensor]:
        return {k: batch[k] for k in ("featmap_a", "featmap_q", "mask_a", "mask_q") if k in batch}

    __call__ = forward


def mask_iou(gt: Tensor, pred: Tensor) -> Tensor:
    """Per-sample IoU of binary masks [B,H,W]: |and| / |or|; an empty union gives NaN, as in utils/metrics.py:18-40."""
    g, p = gt != 0, pred != 0
    inter = (g & p).flatten(1).sum(1).float()
    union = (g | p).flatten(1).sum(1).float()
    return inter / union


class Pipeline:
    def __init__(self, args: SimpleNamespace, model=None, pointdsc_solver: Optional[PointDSC] = None):
        """pointdsc_solver may be None with test.solver = 'ransac' or 'spectral' (the solvers that need no pretrained weights).
        The solver is a property of the pipeline, read from args.test.solver HERE: `pointdsc_solver` is handed in for it, and the
        batched engine bakes it into its arena and registration stream.  The reference reads the flag at every call; this class has
        always refused `args.test.solver = "ransac"` set on a pipeline that was built for PointDSC (the suite pins that), and still
        does now that the solver exists: `get_pose` raises when the flag no longer names the solver the pipeline was built with, so
        the per-sample and the batched route of one pipeline can never use different solvers.  Build a new Pipeline to switch."""
        self.args = args
        self.solver = args.test.solver
        self.device = args.device
        self.corrs_device = args.corrs_device
        self.model = model if model is not None else PrecomputedFeatures()
        self.pointdsc_solver = pointdsc_solver
        self.pred_lines: List[str] = []
        self.failures: List[str] = []
        self._engine: Optional[MatchPoseEngine] = None
        self._feature_loss = None
        self.evaluator = None
        self.train_evaluator = None                      # the reference shares one evaluator; here a validation pass inside an epoch
        self.optimizer = self.scheduler = None           # keeps its lists while training registers its own
        self.last_training: Optional[Dict] = None        # the latest training_step's {'losses', 'results'} (detached)
        self._valid_objects: Optional[Dict] = None
        self._valid_log: List[Dict[str, float]] = []
        self._valid_fmr: List[float] = []
        self.last_validation: Optional[Dict] = None      # the latest validation_step's {'poses', 'status', 'results', 'losses'}
        self.last_refine: Optional[Dict] = None          # the latest ops.icp_refine / ops.icp_plane_refine result (test.refine)
        self.last_verify: Optional[Dict] = None          # the latest ops.pose_verify result (test.verify)
        self._verify_log: List[Tuple] = []               # per step (status, chosen score, best), each [B]: what verify_summary reduces
        self.refine_mode()                               # an unknown test.refine raises here, not at the first pose
        if self.verify_mode() != "none":                 # and so does an unknown test.verify, or a guard with nothing to choose from
            global _latest_verify
            _latest_verify = (self.verify_mode(), self.verify_tol(), self._verify_log)
        self.last_mask_clean: Optional[Dict[str, Tensor]] = None      # the latest step's ops.mask_clean stats per side, on the device
        self._mask_clean_log: List[Tensor] = []          # every cleaned batch's stats [n, 6], on the device: what mask_clean_summary reduces
        if self.mask_clean_active():                     # an unknown test.mask_clean or a fraction outside [0, 1] raises here
            global _latest_mask_clean
            _latest_mask_clean = (*self.mask_clean_cfg(), self._mask_clean_log)
        self.last_subpixel: Optional[Tuple[Tensor, Tensor]] = None    # the latest (offsets [n,2], flags [n]) of the per-sample route
        self._subpixel_log: List[Tuple[Tensor, Tensor]] = []          # per step (flags, offsets) of the rows handed to the lift
        if self.subpixel_cfg()[0]:                       # a negative curvature floor or depth jump raises here
            global _latest_subpixel
            _latest_subpixel = self._subpixel_log

    # ------------------------------------------------------------------ sub-pixel refinement (test.subpixel; csrc/match_subpix.hip)
    def subpixel_cfg(self) -> Tuple[bool, float, float]:
        """(test.subpixel, test.subpixel_curv_min, test.subpixel_depth_jump); absent = (False, 1e-4, 0.02).  Checked as
        MatchPoseConfig checks them."""
        on = bool(getattr(self.args.test, "subpixel", False))
        curv, jump = float(getattr(self.args.test, "subpixel_curv_min", 1e-4)), float(getattr(self.args.test, "subpixel_depth_jump", 0.02))
        if on:
            MatchPoseConfig(solver="ransac", subpixel=True, subpixel_curv_min=curv, subpixel_depth_jump=jump)
        return on, curv, jump

    def subpixel_summary(self) -> Dict:
        """What a driver adds to its summary: {} when test.subpixel is off; else, over the steps of this pipeline so far, the rows handed
        to the lift, how many of them carry each flag (refined, border, flat, outside) and the mean |offset| of the refined ones in
        feature-map pixels."""
        return _reduce_subpixel(self._subpixel_log) if self.subpixel_cfg()[0] else {}

    # ------------------------------------------------------------------ mask clean-up (test.mask_clean; csrc/mask_clean.hip)
    def mask_clean_cfg(self) -> Tuple[str, float, bool]:
        """(test.mask_clean, test.mask_clean_frac, test.mask_fill_holes); absent = the process-wide default, ('none', 0.25, False)
        unless a driver set it."""
        d = default_mask_clean()
        t = self.args.test
        return _check_mask_clean(getattr(t, "mask_clean", d[0]), getattr(t, "mask_clean_frac", d[1]), getattr(t, "mask_fill_holes", d[2]))

    def mask_clean_active(self) -> bool:
        mode, _, fill = self.mask_clean_cfg()
        return mode != "none" or fill

    def clean_masks(self, mask: Tensor, side: Optional[str] = None) -> Tensor:
        """The one place a mask is cleaned: mask [n,H,W] or [H,W] on the device -> int32 of that shape (ops.mask_clean; 'none' with
        test.mask_fill_holes runs the kernel in mode 'all'); the mask itself when clean-up is inactive.  side ('a' / 'q'): the stats
        go under last_mask_clean[side] and into the summary's log, on the device; None: they are not kept."""
        mode, frac, fill = self.mask_clean_cfg()
        if mode == "none" and not fill:
            return mask
        out, stats = ops.mask_clean(mask, mode="all" if mode == "none" else mode, frac=frac, fill_holes=fill, want_stats=True)
        if side is not None:
            self.last_mask_clean = dict(self.last_mask_clean or {}, **{side: stats})
            self._mask_clean_log.append(stats)
        return out

    def mask_clean_summary(self) -> Dict:
        """What a driver adds to its summary: {} when clean-up is inactive; else the flags, the number of masks cleaned so far and the
        means of their statistics (components, kept components, kept / removed / filled pixels).  Reads the device."""
        return _reduce_mask_clean(*self.mask_clean_cfg(), self._mask_clean_log) if self.mask_clean_active() else {}

    # ------------------------------------------------------------------ mask post-processing (losses.py:56-60)
    def mask_results(self, batch: Dict, outputs: Dict) -> Dict[str, Tensor]:
        th = self.args.test.mask_threshold
        res = {"mask_a": ops.mask_from_logits(outputs["mask_a"].squeeze(1), th),
               "mask_q": ops.mask_from_logits(outputs["mask_q"].squeeze(1), th)}
        if self.mask_clean_active():                     # the IoUs below rate the mask the path uses; the thresholded one stays beside it
            for key in ("a", "q"):
                res["mask_" + key + "_raw"] = res["mask_" + key]
                res["mask_" + key] = self.clean_masks(res["mask_" + key], key if self.args.test.mask == "predicted" else None)
        for side, key in (("anchor", "a"), ("query", "q")):
            gt = batch.get(side, {}).get("mask") if isinstance(batch.get(side), dict) else None
            pred = res["mask_" + key]
            if gt is not None:
                gt_r = ops.mask_resize_nearest(gt.to(pred.device), pred.shape[-2:]) if gt.shape[-2:] != pred.shape[-2:] else gt.to(pred.device)
                res["iou_" + key] = mask_iou(gt_r, pred)
            else:
                res["iou_" + key] = torch.zeros(pred.shape[0], device=pred.device)
        return res

    def _external_masks(self, batch: Dict, idx: int, size: Tuple[int, int], log: bool = True) -> Tuple[Tensor, Tensor]:
        """log=False: the cleaned masks' stats are not kept (is_detection_valid looks at masks get_featmap_corrs builds again)."""
        dev = _lib.require_gpu(self.device)
        ma = ops.mask_resize_nearest(batch["anchor"]["mask"][idx].to(dev), size)[0]
        mq = ops.mask_resize_nearest(batch["query"]["mask"][idx].to(dev), size)[0]
        return self.clean_masks(ma, "a" if log else None), self.clean_masks(mq, "q" if log else None)

    # ------------------------------------------------------------------ pipeline.py:372-395
    def is_detection_valid(self, results: Dict, batch: Dict, idx: int) -> bool:
        if self.args.test.mask != "predicted":
            mask_a, mask_q = self._external_masks(batch, idx, tuple(self.args.model.image_encoder.img_size), log=False)
        else:
            mask_a, mask_q = results["mask_a"][idx], results["mask_q"][idx]
        valid_a = torch.count_nonzero(mask_a == 1)
        valid_q = torch.count_nonzero(mask_q == 1)
        return (valid_a.item() > 0) and (valid_q.item() > 0)

    # ------------------------------------------------------------------ pipeline.py:397-427
    def get_featmap_corrs(self, batch: Dict, net_output: Dict, results: Dict, idx: int):
        NH, NW = net_output["featmap_a"].shape[2:]
        if self.args.test.mask != "predicted":
            mask_ai, mask_qi = self._external_masks(batch, idx, (NH, NW))
        else:
            mask_ai, mask_qi = results["mask_a"][idx], results["mask_q"][idx]
        featmap_ai, featmap_qi = net_output["featmap_a"][idx], net_output["featmap_q"][idx]
        ratio = float(getattr(self.args.test, "ratio", 0.0))
        topk = int(getattr(self.args.test, "topk", 1))
        if topk > 1:
            # the checks of the batched route (K, the solvers' row cap, no mutual / ratio) before anything runs
            MatchPoseConfig(n_corrs=self.args.test.n_corrs, solver=self.solver, mutual=bool(getattr(self.args.test, "mutual", False)),
                            ratio=ratio, topk=topk, topk_radius=int(getattr(self.args.test, "topk_radius", 5)),
                            topk_margin=float(getattr(self.args.test, "topk_margin", 0.1)))
            pred_corrs = nn_correspondences_topk(featmap_ai, featmap_qi, mask_ai, mask_qi, self.args.test.dist_th, self.args.test.n_corrs,
                                                 self.args.test.src_sampling, self.corrs_device, topk=topk,
                                                 topk_radius=int(getattr(self.args.test, "topk_radius", 5)),
                                                 topk_margin=float(getattr(self.args.test, "topk_margin", 0.1)))
        elif ratio > 0:
            pred_corrs = nn_correspondences_filtered(featmap_ai, featmap_qi, mask_ai, mask_qi, self.args.test.dist_th, self.args.test.n_corrs,
                                                     self.args.test.src_sampling, self.corrs_device,
                                                     mutual=bool(getattr(self.args.test, "mutual", False)), ratio=ratio,
                                                     ratio_radius=int(getattr(self.args.test, "ratio_radius", 5)))
        else:
            pred_corrs = nn_correspondences(featmap_ai, featmap_qi, mask_ai, mask_qi, self.args.test.dist_th, self.args.test.n_corrs,
                                            self.args.test.src_sampling, self.corrs_device, mutual=bool(getattr(self.args.test, "mutual", False)))
        self.last_subpixel = None
        if pred_corrs is not None and self.subpixel_cfg()[0]:    # the refinement of the rows just drawn; get_pose takes it as offsets=
            self.last_subpixel = subpixel_offsets(featmap_ai, featmap_qi, pred_corrs, self.subpixel_cfg()[1])
        if pred_corrs is not None:
            corr_ai, corr_qi = pred_corrs[:, :2], pred_corrs[:, 2:]
            pos_a = featmap_ai[:, corr_ai[:, 0], corr_ai[:, 1]].transpose(1, 0)
            pos_q = featmap_qi[:, corr_qi[:, 0], corr_qi[:, 1]].transpose(1, 0)
        else:
            pos_a, pos_q = None, None
        return pred_corrs, pos_a, pos_q

    # ------------------------------------------------------------------ ICP refinement (test.refine = icp; utils/geo6d.py:157-208)
    REFINE_SEED_A, REFINE_SEED_Q = 0x1C9A0A, 0x1C9A0B       # the two sides' subsamples draw from streams of their own

    def refine_mode(self) -> str:
        """test.refine: 'none' (absent = the process-wide default, 'none' unless a driver set it), 'icp' - ICP of the anchor's object
        cloud onto the query's - or 'icp_plane' - point-to-plane ICP of that cloud onto the query's depth map - started at the solver's pose."""
        mode = getattr(self.args.test, "refine", default_refine())
        if mode not in REFINEMENTS:
            raise RuntimeError(f"Refinement {mode} not implemented")
        return mode

    def refine_clouds(self, mask_a: Tensor, mask_q: Tensor, depth_a: Tensor, depth_q: Tensor, cam_a: Tensor, cam_q: Tensor,
                      pair_key: Tensor) -> Dict[str, Tensor]:
        """The object clouds ICP runs on, per side: the mask ([B,h,w], the masks the matcher saw - test.mask) resized to the depth map's
        size (nearest), AND depth > 0, compacted to a pixel list, thinned to test.refine_points pixels by the device RNG keyed by
        (seed, pair key) - so a pair's cloud does not depend on the batch it arrives in - and lifted in float64 (ops.gtc_lift).
        depth_* [B,H,W] fp32 millimetres, cam_* [B,9] or [B,3,3], pair_key [B] int64 -> src, dst [B,cap,3] float64 metres (anchor,
        query) and n_src, n_dst [B] int32, all on the device, nothing read back."""
        out = {}
        for side, mask, depth, cam, salt in (("src", mask_a, depth_a, cam_a, self.REFINE_SEED_A), ("dst", mask_q, depth_q, cam_q, self.REFINE_SEED_Q)):
            out[side], out["n_" + side] = self._refine_cloud(mask, depth, cam, salt, pair_key)
        return out

    @staticmethod
    def _object_mask(mask: Tensor, depth: Tensor) -> Tensor:
        """The object's pixels of one side: the mask resized (nearest) to the depth map's size, AND depth > 0 -> [B,H,W] int32."""
        H, W = depth.shape[-2:]
        m = ops.mask_resize_nearest(mask, (H, W)) if tuple(mask.shape[-2:]) != (H, W) else mask.to(torch.int32)
        return ((m == 1) & (depth > 0)).to(torch.int32)

    def _refine_cloud(self, mask: Tensor, depth: Tensor, cam: Tensor, salt: int, pair_key: Tensor) -> Tuple[Tensor, Tensor]:
        """One side of refine_clouds -> (xyz [B,cap,3] float64 metres, count [B] int32)."""
        points = int(getattr(self.args.test, "refine_points", 2048))
        seed = self.args.seed if self.args.seed is not None else 1
        B, H, W = depth.shape
        roi, count = ops.roi_compact(self._object_mask(mask, depth))
        ops.roi_subsample_(roi, count, points, seed ^ salt, pair_key)
        cap = min(points, H * W)
        pix = roi[:, :cap].contiguous()
        count = torch.clamp(count, max=cap)
        # the intrinsics as both solver routes see them: fp32 values, widened
        xyz, _ = ops.gtc_lift(depth, pix, count, cam.to(depth.device, torch.float32).to(torch.float64).reshape(B, 9))
        return xyz, count

    def refine_target(self, mask_q: Tensor, depth_q: Tensor, cam_q: Tensor) -> Dict[str, Tensor]:
        """The target of test.refine = icp_plane: the query's depth map as it is ([B,H,W] fp32 millimetres), its object mask (resized
        with nearest to the depth map's size, AND depth > 0; int32) and the intrinsics as fp32 values, widened ([B,9] float64)."""
        B = depth_q.shape[0]
        return dict(depth=depth_q.contiguous(), mask=self._object_mask(mask_q, depth_q).contiguous(),
                    cam9=cam_q.to(depth_q.device, torch.float32).to(torch.float64).reshape(B, 9).contiguous())

    def refine_inputs(self, mask_a: Tensor, mask_q: Tensor, depth_a: Tensor, depth_q: Tensor, cam_a: Tensor, cam_q: Tensor,
                      pair_key: Tensor) -> Dict[str, Tensor]:
        """What refine_poses runs on in the pipeline's mode: refine_clouds (icp), or the anchor's cloud - the very cloud refine_clouds
        builds for it - and refine_target (icp_plane)."""
        if self.refine_mode() == "icp_plane":
            src, n_src = self._refine_cloud(mask_a, depth_a, cam_a, self.REFINE_SEED_A, pair_key)
            return dict(self.refine_target(mask_q, depth_q, cam_q), src=src, n_src=n_src)
        return self.refine_clouds(mask_a, mask_q, depth_a, depth_q, cam_a, cam_q, pair_key)

    def refine_poses(self, pose: Tensor, status: Optional[Tensor], clouds: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """ops.icp_refine (clouds of refine_clouds) or ops.icp_plane_refine (clouds of refine_inputs in mode icp_plane: they hold a depth
        map) with the flags test.refine_max_iter / refine_tolerance / refine_max_dist / refine_normal_jump (defaults: REFINE_DEFAULTS of
        the mode): pose [B,4,4] fp32 (the solver's) -> the refined poses and the iteration counts; a pair with a failure status keeps
        its pose."""
        t = self.args.test
        plane = "depth" in clouds
        d = REFINE_DEFAULTS["icp_plane" if plane else "icp"]
        max_iter, tolerance = int(getattr(t, "refine_max_iter", 20)), float(getattr(t, "refine_tolerance", d["tolerance"]))
        max_dist = float(getattr(t, "refine_max_dist", d["max_dist"]))
        if plane:
            return ops.icp_plane_refine(clouds["src"], clouds["n_src"], clouds["depth"], clouds["mask"], clouds["cam9"],
                                        pose.to(torch.float32).contiguous(), max_iter=max_iter, tolerance=tolerance, max_dist=max_dist,
                                        normal_jump=float(getattr(t, "refine_normal_jump", d["normal_jump"])), status=status)
        return ops.icp_refine(clouds["src"], clouds["dst"], clouds["n_src"], clouds["n_dst"], pose.to(torch.float32).contiguous(),
                              max_iter=max_iter, tolerance=tolerance, max_dist=max_dist, status=status)

    def _refine_masks(self, batch: Dict, results: Optional[Dict], dev, pairs: slice = slice(None)) -> Tuple[Tensor, Tensor]:
        """The masks of the batch's `pairs` the refiners and the verifier build their clouds from."""
        if self.args.test.mask != "predicted":                   # the external masks at their own size, cleaned like the matcher's
            return self.clean_masks(batch["anchor"]["mask"][pairs].to(dev)), self.clean_masks(batch["query"]["mask"][pairs].to(dev))
        if results is None or "mask_a" not in results:
            raise KeyError(f"test.refine='{self.refine_mode()}' / test.verify='{self.verify_mode()}' with test.mask='predicted' needs the "
                           "predicted masks (results['mask_a'], results['mask_q'])")
        return results["mask_a"][pairs], results["mask_q"][pairs]

    # ------------------------------------------------------------------ depth-consistency verification (test.verify; csrc/pose_verify.hip)
    def verify_mode(self) -> str:
        """test.verify: 'none' (absent = the process-wide default, 'none' unless a driver set it), 'score' - rate the final pose - or
        'guard' - rate the solver's pose and the refined one, keep the better (needs test.refine != 'none')."""
        mode, _ = _check_verify(getattr(self.args.test, "verify", default_verify()[0]), self.verify_tol())
        if mode == "guard" and self.refine_mode() == "none":
            raise ValueError("test.verify='guard' needs a refinement (test.refine='icp' or 'icp_plane'): nothing to choose from")
        return mode

    def verify_tol(self) -> float:
        return float(getattr(self.args.test, "verify_tol", default_verify()[1]))

    def verify_inputs(self, mask_a: Tensor, mask_q: Tensor, depth_a: Tensor, depth_q: Tensor, cam_a: Tensor, cam_q: Tensor,
                      pair_key: Tensor, clouds: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
        """What verify_poses runs on: the anchor's object cloud exactly as _refine_cloud builds it for the refiners (REFINE_SEED_A,
        test.refine_points) and refine_target - the query's depth map, its object mask, the intrinsics.  clouds: what refine_inputs
        returned for the same pair(s), if a refinement ran - its cloud (and, in mode icp_plane, its target) is taken, not rebuilt."""
        if clouds is not None and "depth" in clouds:
            return clouds
        if clouds is not None:
            src, n_src = clouds["src"], clouds["n_src"]
        else:
            src, n_src = self._refine_cloud(mask_a, depth_a, cam_a, self.REFINE_SEED_A, pair_key)
        return dict(self.refine_target(mask_q, depth_q, cam_q), src=src, n_src=n_src)

    def verify_poses(self, poses: Tensor, status: Optional[Tensor], inputs: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """ops.pose_verify on the inputs of verify_inputs with test.verify_tol: poses [B,K,4,4] fp32 -> dict(counts [B,K,7], best [B],
        score [B,K]); a pair with a failure status gets zero counts and best 0."""
        return ops.pose_verify(inputs["src"], inputs["n_src"], inputs["depth"], inputs["mask"], inputs["cam9"],
                               poses.to(torch.float32).contiguous(), tol=self.verify_tol(), status=status)

    def verify_summary(self) -> Dict:
        """What a driver adds to its summary: {} in mode 'none'; else the mode, the tolerance, the mean score of the chosen poses over
        the solved pairs of every step of this pipeline so far and, for 'guard', how many of them kept their refinement."""
        mode = self.verify_mode()
        return {} if mode == "none" else _reduce_verify(mode, self.verify_tol(), self._verify_log)

    def _subpixel_offsets_of_step(self) -> Optional[Tensor]:
        """The offsets get_featmap_corrs just computed (None when test.subpixel is off), logged for subpixel_summary."""
        if self.last_subpixel is None:
            return None
        offsets, flags = self.last_subpixel
        self._subpixel_log.append((flags, offsets))
        return offsets

    # ------------------------------------------------------------------ pipeline.py:429-472
    def get_pose(self, batch: Dict, corrs: Tensor, idx: int, results: Optional[Dict] = None, pair_key: Optional[int] = None,
                 offsets: Optional[Tensor] = None) -> Tensor:
        """results: the masks' post-processing (mask_results), needed by test.refine = icp with predicted masks only; pair_key: the
        pair's global index (default idx), which keys the refinement's subsample; offsets: [n,2] fp32 sub-pixel (dy, dx) of the rows'
        query pixels (pcd.subpixel_offsets) - given, the lift is ops.lift_pairs_subpix with test.subpixel_depth_jump."""
        dev = _lib.require_gpu(self.device)
        depth_a = batch["anchor"]["orig_depth"][idx].squeeze().to(dev, torch.float32)
        depth_q = batch["query"]["orig_depth"][idx].squeeze().to(dev, torch.float32)
        camera_a = batch["anchor"]["camera"][idx].reshape(1, 9).to(torch.float32).to(dev)
        camera_q = batch["query"]["camera"][idx].reshape(1, 9).to(torch.float32).to(dev)
        HO, WO = self.args.model.image_encoder.img_size
        if self.args.test.solver not in SOLVERS:
            raise RuntimeError(f"Solver {self.args.test.solver} not implemented")
        if self.args.test.solver != self.solver:
            raise RuntimeError(f"test.solver was changed from '{self.solver}' to '{self.args.test.solver}' after this Pipeline was built: "
                               "the solver is fixed at construction, build a new Pipeline")
        c = corrs.to(dev).to(torch.int32).contiguous()[None]
        if offsets is not None:
            pcd_a, pcd_q, n = ops.lift_pairs_subpix(c, None, (HO, WO), depth_a[None].contiguous(), depth_q[None].contiguous(), camera_a,
                                                    camera_q, offsets=offsets.to(dev, torch.float32).contiguous()[None],
                                                    depth_jump=self.subpixel_cfg()[2])
        else:
            pcd_a, pcd_q, n = ops.lift_pairs(c, None, (HO, WO), depth_a[None].contiguous(), depth_q[None].contiguous(),
                                             camera_a, camera_q)
        m = int(n.item())
        if self.args.test.solver == "ransac":                  # pipeline.py:462-466
            pose = best_fit_transform_with_RANSAC(pcd_a[0, :m], pcd_q[0, :m], max_iter=10000, fix_percent=0.9999, match_err=0.001,
                                                  device=dev)
            pose4 = np.eye(4)
            pose4[:3, :] = pose
            pose4 = torch.tensor(pose4)
        elif self.args.test.solver == "spectral":
            pose4 = spectral_pose(pcd_a[0, :m], pcd_q[0, :m], dev, **self._spectral_cfg())
        else:
            pose4 = get_pointdsc_pose(self.pointdsc_solver, pcd_a[0, :m], pcd_q[0, :m], self.device)
        refine, verify = self.refine_mode(), self.verify_mode()
        if refine == "none" and verify == "none":
            return pose4.to(torch.float32)
        mask_a, mask_q = self._refine_masks(batch, results, dev, slice(idx, idx + 1))
        key = torch.tensor([idx if pair_key is None else pair_key], dtype=torch.int64, device=dev)
        sides = (mask_a, mask_q, depth_a[None].contiguous(), depth_q[None].contiguous(), camera_a, camera_q, key)
        start = pose4.to(torch.float32)[None].to(dev)
        final, clouds = start, None
        if refine != "none":
            clouds = self.refine_inputs(*sides)
            self.last_refine = self.refine_poses(start, None, clouds)
            final = self.last_refine["T"]
        if verify != "none":                                   # guard: [solver's, refined] - the solver's pose wins an exact tie
            cand = torch.stack([start, final], dim=1) if verify == "guard" else final[:, None]
            self.last_verify = self.verify_poses(cand, None, self.verify_inputs(*sides, clouds=clouds))
            if verify == "guard":
                final = cand[:, int(self.last_verify["best"][0])]
        return final[0].cpu() if refine != "none" else pose4.to(torch.float32)

    _SPECTRAL_FIELDS = ("num_iterations", "ratio", "inlier_threshold", "sigma_d", "k", "nms_radius")

    def _spectral_cfg(self) -> Dict[str, float]:
        """test.spectral_* (absent = the defaults of MatchPoseConfig) under the names of oryon_spectral_config_t, the floats rounded
        through float32 as the engine carries them: both routes hand the kernels the same numbers."""
        d = MatchPoseConfig(solver="spectral")
        vals = {f: getattr(self.args.test, "spectral_" + f, getattr(d, "spectral_" + f)) for f in self._SPECTRAL_FIELDS}
        return {f: (int(v) if f in ("num_iterations", "k") else ctypes.c_float(float(v)).value) for f, v in vals.items()}

    # ------------------------------------------------------------------ pipeline.py:490-497
    def add_pred_pose(self, id_a: str, id_q: str, mask_a_iou, mask_q_iou, pred_pose: np.ndarray) -> str:
        pose_txt = " ".join([str(n) for n in pred_pose[:3, :].flatten()])
        line = ",".join([id_a, id_q, pose_txt, str(mask_a_iou), str(mask_q_iou)]) + "\n"
        self.pred_lines.append(line)
        return line

    # ------------------------------------------------------------------ pipeline.py:311 -> losses.py:64-88,196-199,250
    def feature_loss_rng_draws(self, batch: Dict, outputs: Dict) -> int:
        """The reference's test_step calls `self.feature_loss.forward(batch, outputs)` before the per-sample loop (pipeline.py:311) - for
        its mask post-processing, but the call also samples contrastive negatives and thereby CONSUMES random numbers ahead of the
        matcher's two draws.  The loss values are not part of the path; the generator state is: with `seed: 1` the matcher's samples
        depend on it.  This replays exactly those draws (same generator, same order, same arguments) and returns how many were made:
          loss.hard_negatives (config.yaml:43, default True): per side (anchor, then query) and per pair with batch['valid'] == 1,
              `torch_sample_select(featmap_i, 2000)` when FH*FW > 2000 (losses.py:196-199) = multinomial(ones(HW, float64), 2000, False)
              on the FEATURE MAP's device - the CUDA generator in a GPU run, i.e. it only interacts with the matcher's draws
              (CPU generator, `corrs_device: cpu`) when everything runs on one device;
          otherwise `torch.randint(0, HW, (n_gt_corrs,))` on the CPU generator (losses.py:250).
        Batches without the loader's 'valid' / 'corrs' entries (synthetic drivers) draw nothing."""
        if "valid" not in batch or "corrs" not in batch:
            return 0
        fm = outputs["featmap_a"]
        HW = fm.shape[2] * fm.shape[3]
        hard = bool(getattr(getattr(self.args, "loss", None), "hard_negatives", True))
        valid = batch["valid"]
        n = 0
        for _side in ("a", "q"):
            for i_b in range(fm.shape[0]):
                if valid[i_b] == 1:
                    if hard:
                        if HW > 2000:
                            torch.multinomial(torch.ones(HW, dtype=float).to(fm.device), 2000, replacement=False)
                            n += 1
                    else:
                        torch.randint(0, HW, (batch["corrs"].shape[1],))
                        n += 1
        return n

    # ------------------------------------------------------------------ pipeline.py:306-355
    def test_step(self, batch: Dict, batch_idx: int = 0, first_pair_index: int = 0) -> List[Dict]:
        outputs = self.model.forward(batch)
        BS = outputs["featmap_a"].shape[0]
        self.feature_loss_rng_draws(batch, outputs)          # generator state as after pipeline.py:311
        # the reference evaluates the predicted masks (and logs their IoU) whatever test.mask says (pipeline.py:311,352-354);
        # only the masks fed to the matcher switch to the external ones
        if "mask_a" in outputs and "mask_q" in outputs:
            results = self.mask_results(batch, outputs)
        elif self.args.test.mask == "predicted":
            raise KeyError("test.mask='predicted' needs the model's mask logits (outputs['mask_a'], outputs['mask_q'])")
        else:
            results = {"iou_a": torch.ones(BS), "iou_q": torch.ones(BS)}
        records = []
        for i_b in range(BS):
            id_a, id_q = batch["anchor"]["instance_id"][i_b], batch["query"]["instance_id"][i_b]
            status, pred_q = PAIR_OK, None
            if self.is_detection_valid(results, batch, i_b):
                pred_corrs, _, _ = self.get_featmap_corrs(batch, outputs, results, idx=i_b)
                if pred_corrs is not None:
                    pred_pose = self.get_pose(batch, pred_corrs, idx=i_b, results=results, pair_key=first_pair_index + i_b,
                                              offsets=self._subpixel_offsets_of_step())
                    pred_q = pred_pose @ batch["anchor"]["pose"][i_b].cpu().detach().to(torch.float32)
                else:
                    status, pred_pose = PAIR_NO_CORR, torch.eye(4)
            else:
                status, pred_pose = PAIR_NO_MASK, torch.eye(4)
            if status != PAIR_OK:
                self.failures.append(batch["instance_id"][i_b] if "instance_id" in batch else id_q)
            iou_a = results["iou_a"][i_b].cpu().numpy()
            iou_q = results["iou_q"][i_b].cpu().numpy()
            self.add_pred_pose(id_a, id_q, iou_a, iou_q, pred_pose.cpu().numpy())
            records.append(dict(status=status, pred_pose_rel=pred_pose, pred_pose=pred_q))
            if status == PAIR_OK and self.refine_mode() != "none":
                records[-1]["refine_iters"] = int(self.last_refine["iters"][0])
            if status == PAIR_OK and self.verify_mode() != "none":         # the chosen candidate's counts and score
                v = self.last_verify
                best = int(v["best"][0])
                records[-1]["verify_counts"] = [int(c) for c in v["counts"][0, best].cpu().tolist()]
                records[-1]["verify_score"] = float(v["score"][0, best])
                if self.verify_mode() == "guard":
                    records[-1]["verify_best"] = best
                self._verify_log.append((torch.tensor([PAIR_OK]), torch.tensor([records[-1]["verify_score"]], dtype=torch.float64),
                                         torch.tensor([best])))
        return records

    # ------------------------------------------------------------------ batched device path
    def test_step_batched(self, batch: Dict, first_pair_index: int = 0) -> Dict[str, Tensor]:
        """Same stages for the whole batch in ~25 launches and no host round trip.  orig_depth entries must share
        one size per side (NOCS / TOYL: 480x640).  Returns pose_rel [B,4,4], pred_q [B,4,4], status [B]."""
        dev = _lib.require_gpu(self.device)
        outputs = self.model.forward(batch)
        BS = outputs["featmap_a"].shape[0]
        FH, FW = outputs["featmap_a"].shape[2:]
        res = None
        if "mask_a" in outputs and "mask_q" in outputs:          # the predicted masks are evaluated (IoU) whatever test.mask says
            res = self.mask_results(batch, outputs)
        if self.args.test.mask == "predicted":
            if res is None:
                raise KeyError("test.mask='predicted' needs the model's mask logits (outputs['mask_a'], outputs['mask_q'])")
            mask_a, mask_q = res["mask_a"], res["mask_q"]
        else:
            mask_a = self.clean_masks(ops.mask_resize_nearest(batch["anchor"]["mask"].to(dev), (FH, FW)), "a")
            mask_q = self.clean_masks(ops.mask_resize_nearest(batch["query"]["mask"].to(dev), (FH, FW)), "q")
        if self._engine is None:
            self._engine = MatchPoseEngine(self.pointdsc_solver, MatchPoseConfig(
                dist_th=self.args.test.dist_th, n_corrs=self.args.test.n_corrs, src_sampling=self.args.test.src_sampling,
                seed=self.args.seed if self.args.seed is not None else 1, solver=self.solver,
                mutual=bool(getattr(self.args.test, "mutual", False)),
                ratio=float(getattr(self.args.test, "ratio", 0.0)), ratio_radius=int(getattr(self.args.test, "ratio_radius", 5)),
                topk=int(getattr(self.args.test, "topk", 1)), topk_radius=int(getattr(self.args.test, "topk_radius", 5)),
                topk_margin=float(getattr(self.args.test, "topk_margin", 0.1)),
                subpixel=self.subpixel_cfg()[0], subpixel_curv_min=self.subpixel_cfg()[1], subpixel_depth_jump=self.subpixel_cfg()[2],
                **{"spectral_" + f: v for f, v in self._spectral_cfg().items()}))

        def stack(x):
            return (torch.stack([d.squeeze() for d in x]) if isinstance(x, (list, tuple)) else x).to(dev, torch.float32).contiguous()
        depth_a, depth_q = stack(batch["anchor"]["orig_depth"]), stack(batch["query"]["orig_depth"])
        key = torch.arange(first_pair_index, first_pair_index + BS, dtype=torch.int64, device=dev)
        out = self._engine.run(outputs["featmap_a"].float().contiguous(), outputs["featmap_q"].float().contiguous(), mask_a,
                               mask_q, depth_a, depth_q, batch["anchor"]["camera"].to(dev), batch["query"]["camera"].to(dev), key)
        if "subpix_flags" in out:                                # the rows handed to the lift: [0, n_rows) of every solved pair
            n_rows = out["n_rows"] if "n_rows" in out else torch.where(out["status"] == PAIR_OK, self.args.test.n_corrs, 0)
            live = torch.arange(out["subpix_flags"].shape[1], device=dev)[None] < n_rows[:, None]
            self._subpixel_log.append((out["subpix_flags"][live], out["subpix_offsets"][live]))
        refine, verify = self.refine_mode(), self.verify_mode()
        clouds = None
        if refine != "none" or verify != "none":
            rmask_a, rmask_q = self._refine_masks(batch, res, dev)
            sides = (rmask_a, rmask_q, depth_a, depth_q, batch["anchor"]["camera"].to(dev), batch["query"]["camera"].to(dev), key)
        if refine != "none":                                     # same stream, no host round trip; failed pairs keep their identity
            clouds = self.refine_inputs(*sides)
            self.last_refine = self.refine_poses(out["pose"], out["status"], clouds)
            out["pose_unrefined"], out["pose"], out["refine_iters"] = out["pose"], self.last_refine["T"], self.last_refine["iters"]
        if verify != "none":                                     # same stream again, nothing read back; failed pairs: zero counts, best 0
            guard = verify == "guard"
            cand = torch.stack([out["pose_unrefined"].to(torch.float32), out["pose"]], dim=1) if guard else out["pose"].to(torch.float32)[:, None]
            v = self.last_verify = self.verify_poses(cand, out["status"], self.verify_inputs(*sides, clouds=clouds))
            pick = v["best"].to(torch.int64)
            out["verify_counts"], out["verify_score"] = v["counts"], v["score"].gather(1, pick[:, None])[:, 0]
            if guard:                                            # [solver's, refined]: the solver's pose wins an exact tie
                out["pose_refined"], out["verify_best"] = out["pose"], v["best"]
                out["pose"] = cand.gather(1, pick[:, None, None, None].expand(-1, 1, 4, 4))[:, 0].contiguous()
            self._verify_log.append((out["status"], out["verify_score"], v["best"]))
        anchor_pose = batch["anchor"]["pose"].to(dev, torch.float32)
        out["pred_q"] = torch.bmm(out["pose"], anchor_pose)
        if res is not None:
            out["iou_a"], out["iou_q"] = res["iou_a"], res["iou_q"]
        return out

    # ------------------------------------------------------------------ validation (pipeline.py:196-247, 579-590)
    @property
    def feature_loss(self):
        """The reference's `self.feature_loss` (pipeline.py:60), built on first use."""
        if self._feature_loss is None:
            from .losses import FeatureLoss
            self._feature_loss = FeatureLoss(self.args, self.device)
        return self._feature_loss

    def reduce_losses(self, losses: Dict) -> Tuple[Tensor, Dict]:
        """pipeline.py:579-590: every loss times its weight `loss.w[k]`, and their sum."""
        w_losses = {}
        final_loss = 0.0
        weights = self.args.loss.w
        for k in losses.keys():
            w_loss = losses[k] * weights[k]
            final_loss = final_loss + w_loss
            w_losses[k] = w_loss
        return final_loss, w_losses

    # ------------------------------------------------------------------ training (pipeline.py:100-152, 170-181)
    def configure_optimizers(self):
        """pipeline.py:100-152: SGD or AdamW ('Adam') over model.get_trainable_parameters(), and the scheduler `step` (x gamma after 50,
        75 and 90 % of the epochs), `cosine` (down to gamma lr over n_epochs - 1), `exp` or 'None' (a step that never comes).  The
        scheduler steps once per epoch.  -> ([optimizer], [scheduler]), also kept as self.optimizer / self.scheduler."""
        opt, n_epochs = self.args.optimization, self.args.training.n_epochs
        parameters = self.model.get_trainable_parameters()
        if opt.optim_type == "SGD":
            optimizer = torch.optim.SGD(params=parameters, lr=opt.lr, momentum=opt.momentum, weight_decay=opt.w_decay, nesterov=False)
        elif opt.optim_type == "Adam":
            optimizer = torch.optim.AdamW(params=parameters, lr=opt.lr, weight_decay=opt.w_decay)
        else:
            raise RuntimeError("Optimizer type {} not implemented!".format(opt.optim_type))
        sched = torch.optim.lr_scheduler
        if opt.scheduler_type == "step":
            scheduler = sched.MultiStepLR(optimizer, milestones=[math.ceil(n_epochs * s) for s in (0.5, 0.75, 0.9)], gamma=opt.gamma)
        elif opt.scheduler_type == "cosine":
            scheduler = sched.CosineAnnealingLR(optimizer, T_max=n_epochs - 1, eta_min=opt.gamma * opt.lr)
        elif opt.scheduler_type == "exp":
            scheduler = sched.ExponentialLR(optimizer, gamma=opt.gamma)
        elif opt.scheduler_type in ("None", None):
            scheduler = sched.MultiStepLR(optimizer, milestones=[n_epochs * 2], gamma=opt.gamma)
        else:
            raise RuntimeError("Scheduler type {} not implemented!".format(opt.scheduler_type))
        self.optimizer, self.scheduler = optimizer, scheduler
        return [optimizer], [scheduler]

    def training_step(self, batch: Dict, batch_idx: int = 0):
        """pipeline.py:170-181: the model in train mode, forward, feature_loss.forward, reduce_losses, evaluator.register_train (the
        batch's IoUs).  -> (the weighted loss, differentiable with respect to the trainable parameters; {'train/mask', 'train/pos',
        'train/neg', 'train/loss'} detached, what the reference's structured_log records)."""
        from .evaluation import Evaluator
        if self.train_evaluator is None:
            self.train_evaluator = Evaluator(exp_tag="train", compute_iou=True)
        if hasattr(self.model, "train"):                     # PrecomputedFeatures has no modes
            self.model.train()
        with torch.enable_grad():
            outputs = self.model.forward(batch)
            losses, results = self.feature_loss.forward(batch, outputs)
            loss, w_losses = self.reduce_losses(losses)
        self.train_evaluator.register_train(results, clear=True)
        self.last_training = dict(losses={k: v.detach() for k, v in losses.items()}, results=results)
        log = {"train/" + k: v.detach() for k, v in w_losses.items()}
        log["train/loss"] = loss.detach()
        return loss, log

    def on_validation_start(self, objects: Optional[Dict] = None, compute_vsd: bool = False) -> None:
        """A fresh evaluator in validation mode (evaluator.init_validation).  objects[cls_id] = {'pts' [N,3] mm, 'diameter' mm (BOP),
        'syms' [S,3,4]} as evaluation.evaluate_batch takes them (the reference's add_object_info of the validation dataset); None = one
        stand-in model for every class, a 512-point sphere of 0.2 m, what the synthetic drivers score against."""
        from .evaluation import Evaluator
        self.evaluator = Evaluator(exp_tag="valid", compute_iou=True, compute_vsd=compute_vsd)
        self.evaluator.init_validation()
        self._valid_objects = dict(objects) if objects is not None else None
        self._valid_log, self._valid_fmr = [], []
        self.last_validation = None

    def add_validation_objects(self, objects: Dict) -> None:
        """More object models for the running validation pass (the reference's add_object_info, called as classes turn up)."""
        self._valid_objects = {**(self._valid_objects or {}), **objects}

    @staticmethod
    def _stand_in_object() -> Dict:
        sphere = np.random.default_rng(0).normal(size=(512, 3))
        sphere = 100.0 * sphere / np.linalg.norm(sphere, axis=1, keepdims=True)
        return {"pts": sphere, "diameter": 200.0, "syms": np.eye(3, 4)[None]}

    def gt_featmap_corrs(self, batch: Dict, net_output: Dict, idx: int) -> Tensor:
        """The batch's ground-truth correspondences of pair idx in feature-map pixels [N,4] (losses.py:77-78)."""
        from .losses import batch_corrs, featmap_corrs
        CH, CW = batch["anchor"]["rgb"].shape[2:]
        FH, FW = net_output["featmap_a"].shape[2:]
        return featmap_corrs(batch_corrs(batch)[idx:idx + 1], (CH, CW), (FH, FW))[0]

    def validation_step(self, batch: Dict, batch_idx: int = 0):
        """pipeline.py:196-247: forward, feature_loss.forward, then per pair is_detection_valid -> get_featmap_corrs -> get_pose ->
        evaluator.register_eval, or register_valid_failure; returns (the weighted loss, {'valid/mask', 'valid/pos', 'valid/neg',
        'valid/loss'}) - what the reference returns and what its structured_log records.  The masks fed to the matcher follow test.mask.
        args.debug_valid: the pose is solved from the batch's GROUND-TRUTH correspondences (rescaled to the feature-map frame, the same
        get_pose) instead of the matcher's; a pair with valid != 1 goes to the failure path.  That is what the flag's comment in
        configs/config.yaml:11 promises; the reference at this commit only prints a warning (pipeline.py:293-294) and changes the
        sampling of its datasets (datasets.py:126-127)."""
        from .evaluation import evaluate_batch, fmr_from_distances
        if self.evaluator is None:
            self.on_validation_start()
        outputs = self.model.forward(batch)
        losses, results = self.feature_loss.forward(batch, outputs)
        BS = outputs["featmap_a"].shape[0]
        poses, status = [], []
        for i_b in range(BS):
            st, pred_pose = PAIR_OK, torch.eye(4)
            if self.args.debug_valid:
                if int(batch["valid"][i_b]) == 1:
                    pred_pose = self.get_pose(batch, self.gt_featmap_corrs(batch, outputs, i_b), idx=i_b, results=results)
                else:
                    st = PAIR_NO_CORR
            elif self.is_detection_valid(results, batch, i_b):
                pred_corrs, _, _ = self.get_featmap_corrs(batch, outputs, results, idx=i_b)
                if pred_corrs is not None:
                    pred_pose = self.get_pose(batch, pred_corrs, idx=i_b, results=results, offsets=self._subpixel_offsets_of_step())
                else:
                    st = PAIR_NO_CORR
            else:
                st = PAIR_NO_MASK
            poses.append(pred_pose.cpu())
            status.append(st)
        cls_ids = list(batch["cls_id"])
        objects = self._valid_objects
        if objects is None:
            stand_in = self._stand_in_object()
            objects = {k: stand_in for k in dict.fromkeys(cls_ids)}
        depth = None
        if self.evaluator.compute_vsd:
            depth = [np.asarray(d.squeeze().cpu().numpy(), dtype=np.float32) for d in batch["query"]["eval_depth"]]
        evaluate_batch(self.evaluator, pred_pose_rel=torch.stack(poses).numpy(), anchor_pose=batch["anchor"]["pose"].cpu().numpy(),
                       gt_pose=batch["query"]["pose"].cpu().numpy(), K=batch["query"]["camera"].cpu().numpy().reshape(-1, 3, 3),
                       status=status, cls_ids=cls_ids, instance_ids=[None] * BS, objects=objects,
                       iou_a=results["iou_a"].cpu().numpy(), iou_q=results["iou_q"].cpu().numpy(), device=self.device, depth=depth,
                       validation=True)
        loss, w_losses = self.reduce_losses(losses)
        log = {"valid/" + k: v for k, v in w_losses.items()}
        log["valid/loss"] = loss
        self._valid_log.append({k: float(v) for k, v in log.items()})
        keep = [i for i in range(BS) if int(batch["valid"][i]) == 1]
        if keep:
            self._valid_fmr.extend(fmr_from_distances(results["d_pos"][keep], self.args.test.dist_th, 0.05).tolist())
        self.last_validation = dict(poses=poses, status=status, results=results, losses=losses)
        return loss, log

    def on_validation_end(self) -> Dict:
        """The epoch's summary: the means of the logged (weighted) losses, FMR at (test.dist_th, 0.05) over the valid pairs, the
        evaluator's means and its failure counts."""
        out: Dict[str, object] = {}
        for k in ("valid/mask", "valid/pos", "valid/neg", "valid/loss"):
            out[k] = float(np.mean([r[k] for r in self._valid_log])) if self._valid_log else None
        out["FMR"] = float(np.mean(self._valid_fmr)) if self._valid_fmr else None
        if self.evaluator is not None:
            out.update(self.evaluator.get_means())
            out.update({k: int(sum(v)) for k, v in self.evaluator.counts.items()})
        return out
