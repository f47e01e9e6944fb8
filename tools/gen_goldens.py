#!/usr/bin/env python3
"""Golden-vector generator (runs ONLY in the build container, where /root/reference exists).

Imports the reference's own hot-path modules (read-only, no bytecode written) with `sys.modules`
stubs for packages that are imported but never called on the path (cv2, omegaconf, easydict;
SURVEY.md Appendix C), runs them on small seeded inputs and writes inputs + expected outputs as
`.npz` fixtures under tests/golden/.  The fixtures are data only; no reference source travels.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_goldens.py

Reference entry points executed here:
  utils/pcd.py        pdist('inv_norm_cosine'), nn_correspondences, lift_pcd
  utils/coordinates.py scale_coords, get_valid_coords
  models/pointdsc/common.py   rigid_transform_3d, knn
  models/pointdsc/PointDSC.py PointDSC (encoder, classification, pick_seeds, cal_seed_trans,
                              cal_leading_eigenvector, post_refinement, forward)
  utils/pointdsc/init.py      get_pointdsc_pose
  utils/geo6d.py              best_fit_transform_with_RANSAC (gen_ransac; `python tools/gen_goldens.py ransac`)
  utils/evaluator.py          Evaluator(compute_vsd=True) + bop_toolkit_lib/pose_error.py vsd, misc.py, visibility.py (gen_vsd;
                              `python tools/gen_goldens.py vsd`; the OpenGL renderer is stood in for by evaluation.rasterize_depth)
  losses.py                   FeatureLoss.forward (sample_positives, sample_hardest_negatives, sample_negatives, mask_loss) and
                              utils/metrics.py compute_fmr (gen_feature_loss; `python tools/gen_goldens.py floss`); the same forward
                              followed by torch's backward (gen_feature_loss_grad; `python tools/gen_goldens.py floss_grad`)
  utils/geo6d.py              icp over nearest_neighbor + best_fit_transform_icp (gen_icp; `python tools/gen_goldens.py icp`)
  scripts/data/make_toyl_test.py  pcd_correspondences (gen_gt_corrs; `python tools/gen_goldens.py gt_corrs`): recorded results only
"""
import json
import os
import time
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
for _name, _attrs in {"cv2": {}, "omegaconf": {"DictConfig": dict, "OmegaConf": object},
                      "easydict": {"EasyDict": dict}}.items():
    _m = types.ModuleType(_name)
    _m.__dict__.update(_attrs)
    sys.modules[_name] = _m

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from utils.pcd import nn_correspondences, lift_pcd, pdist  # noqa: E402  (reference)
from utils import coordinates  # noqa: E402  (reference)
from utils.pointdsc.init import get_pointdsc_pose  # noqa: E402  (reference)
from models.pointdsc.PointDSC import PointDSC  # noqa: E402  (reference)
from models.pointdsc.common import rigid_transform_3d, knn  # noqa: E402  (reference)

from oracle.oryon_oracle import analytic_pointdsc_params  # noqa: E402  (ours: closed-form weights)
from oryon_amd.synth import make_pair  # noqa: E402  (ours: synthetic pair)

OUT = os.path.join(ROOT, "tests", "golden")
os.makedirs(OUT, exist_ok=True)
torch.set_num_threads(8)


def save(name, **arrays):
    conv = {}
    for k, v in arrays.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        conv[k] = np.asarray(v)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **conv)
    print(f"wrote {name}.npz  ({sum(a.nbytes for a in conv.values()) / 1024:.1f} KiB raw)")


# ---------------------------------------------------------------------------------------------- G1
def matcher_case(tag, C, H, W, seed, mask_kind, threshold=0.25, ties=False, zero_desc=False, correlated=True):
    g = torch.Generator().manual_seed(seed)
    f1 = torch.randn(C, H, W, generator=g)
    f2 = torch.randn(C, H, W, generator=g)
    if correlated:  # make a share of query pixels near-copies of anchor pixels so some rows pass the threshold
        perm = torch.randperm(H * W, generator=g)
        n = (H * W) // 2
        f2v = f2.view(C, -1)
        f2v[:, perm[:n]] = f1.view(C, -1)[:, perm[n:2 * n]] + 0.15 * torch.randn(C, n, generator=g)
    m1 = torch.zeros(H, W, dtype=torch.int32)
    m2 = torch.zeros(H, W, dtype=torch.int32)
    if mask_kind == "boxes":
        m1[H // 4:3 * H // 4, W // 5:4 * W // 5] = 1
        m2[H // 6:5 * H // 6, W // 6:5 * W // 6] = 1
    elif mask_kind == "ones":
        m1[:] = 1
        m2[:] = 1
    elif mask_kind == "random":
        m1 = (torch.rand(H, W, generator=g) > 0.6).to(torch.int32)
        m2 = (torch.rand(H, W, generator=g) > 0.4).to(torch.int32)
    elif mask_kind == "empty_a":
        m2[:] = 1
    elif mask_kind == "single":
        m1[H // 2, W // 2] = 1
        m2[H // 3, W // 3] = 1
        m2[H // 3, W // 3 + 1] = 1
    elif mask_kind == "values":   # mask holding values other than {0,1}: only ==1 counts
        m1 = torch.randint(0, 3, (H, W), generator=g, dtype=torch.int32)
        m2 = torch.randint(0, 3, (H, W), generator=g, dtype=torch.int32)
    if ties:       # duplicate query descriptors -> exact ties, first index must win
        f2v = f2.view(C, -1)
        f2v[:, 1::2] = f2v[:, 0::2][:, : f2v[:, 1::2].shape[1]]
    if zero_desc:  # all-zero descriptors exercise the eps clamp
        f1[:, H // 2, :] = 0
        f2[:, :, W // 2] = 0
    roi1 = torch.nonzero(m1 == 1)
    roi2 = torch.nonzero(m2 == 1)
    out = dict(feats1=f1, feats2=f2, mask1=m1, mask2=m2, threshold=np.float32(threshold), roi1=roi1, roi2=roi2)
    if roi1.shape[0] and roi2.shape[0]:
        a = f1[:, roi1[:, 0], roi1[:, 1]].T.to(torch.float32)
        b = f2[:, roi2[:, 0], roi2[:, 1]].T.to(torch.float32)
        dist = pdist(a, b, "inv_norm_cosine")                       # reference utils/pcd.py:202
        min_dist = torch.amin(dist, dim=1)                          # :203
        arg = torch.argmin(dist, dim=1)                             # :204
        if dist.shape[1] > 1:
            top2 = torch.topk(dist, 2, dim=1, largest=False)[0]
            gap = top2[:, 1] - top2[:, 0]
        else:
            gap = torch.full_like(min_dist, float("inf"))
        # a row is an exact tie if another column holds exactly the minimum
        ntie = (dist == min_dist[:, None]).sum(dim=1)
        out.update(min_dist=min_dist, argmin=arg, valid=(min_dist < threshold), gap=gap, n_at_min=ntie)
    torch.manual_seed(1)
    corrs = nn_correspondences(f1.clone(), f2.clone(), m1, m2, threshold, 500, 5000, "cpu")   # full reference call
    out["sampled_is_none"] = np.bool_(corrs is None)
    if corrs is not None:
        out["sampled_corrs"] = corrs
    save(f"g1_matcher_{tag}", **out)


def matcher_half_case():
    """The reference's corrs_device='cuda' branch (descriptors cast to float16, utils/pcd.py:195-197), executed on CPU half tensors."""
    g = torch.Generator().manual_seed(77)
    C, H, W = 32, 24, 24
    f1 = torch.randn(C, H, W, generator=g)
    f2 = torch.randn(C, H, W, generator=g)
    perm = torch.randperm(H * W, generator=g)
    n = (H * W) // 2
    f2.view(C, -1)[:, perm[:n]] = f1.view(C, -1)[:, perm[n:2 * n]] + 0.15 * torch.randn(C, n, generator=g)
    m1 = (torch.rand(H, W, generator=g) > 0.3).to(torch.int32)
    m2 = (torch.rand(H, W, generator=g) > 0.2).to(torch.int32)
    roi1, roi2 = torch.nonzero(m1 == 1), torch.nonzero(m2 == 1)
    a = f1[:, roi1[:, 0], roi1[:, 1]].T.to(torch.float16)
    b = f2[:, roi2[:, 0], roi2[:, 1]].T.to(torch.float16)
    dist = pdist(a, b, "inv_norm_cosine")
    top2 = torch.topk(dist.float(), 2, dim=1, largest=False)[0]
    save("g1_matcher_half", feats1=f1, feats2=f2, mask1=m1, mask2=m2, threshold=np.float32(0.25),
         min_dist=torch.amin(dist, dim=1).float(), argmin=torch.argmin(dist, dim=1), gap=top2[:, 1] - top2[:, 0])


def gen_matcher():
    matcher_half_case()
    matcher_case("c32_24", 32, 24, 24, 11, "boxes")
    matcher_case("c256_16", 256, 16, 16, 12, "ones")
    matcher_case("c32_48", 32, 48, 48, 13, "random")
    matcher_case("ties", 16, 20, 20, 14, "ones", ties=True)
    matcher_case("zero", 8, 16, 16, 15, "ones", zero_desc=True)
    matcher_case("empty_a", 8, 12, 12, 16, "empty_a")
    matcher_case("single", 8, 12, 12, 17, "single")
    matcher_case("values", 24, 20, 28, 18, "values")
    matcher_case("nomatch", 64, 16, 16, 19, "ones", correlated=False)      # nothing under threshold -> None
    matcher_case("subsample", 8, 80, 80, 20, "ones")                        # N1 = 6400 > 5000 -> first RNG draw


# ---------------------------------------------------------------------------------------------- G2
def lift_case(tag, HA, WA, HQ, WQ, FH, FW, K_a, K_q, seed, depth_dtype):
    g = torch.Generator().manual_seed(seed)
    n = 300
    corrs = torch.stack([torch.randint(0, FH, (n,), generator=g), torch.randint(0, FW, (n,), generator=g),
                         torch.randint(0, FH, (n,), generator=g), torch.randint(0, FW, (n,), generator=g)], dim=1)
    corrs[:4] = torch.tensor([[0, 0, 0, 0], [FH - 1, FW - 1, FH - 1, FW - 1], [0, FW - 1, FH - 1, 0], [FH - 1, 0, 0, FW - 1]])
    depth_a = torch.randint(300, 3000, (HA, WA), generator=g).to(depth_dtype)
    depth_q = torch.randint(300, 3000, (HQ, WQ), generator=g).to(depth_dtype)
    depth_a[torch.rand(HA, WA, generator=g) < 0.1] = 0     # zero-depth pixels are NOT filtered by the reference
    depth_q[torch.rand(HQ, WQ, generator=g) < 0.1] = 0
    cam_a = torch.tensor(K_a, dtype=torch.float64).reshape(9)
    cam_q = torch.tensor(K_q, dtype=torch.float64).reshape(9)
    sizes_a, sizes_q = torch.tensor([HA, WA]), torch.tensor([HQ, WQ])
    HAt, WAt = sizes_a     # 0-dim int64 tensors, exactly what pipeline.py:438-439 holds
    HQt, WQt = sizes_q
    ca, cq = corrs[:, :2].clone(), corrs[:, 2:].clone()
    ca = coordinates.scale_coords(ca, (FH, FW), (HAt, WAt))          # pipeline.py:447
    cq = coordinates.scale_coords(cq, (FH, FW), (HQt, WQt))          # :448
    va = coordinates.get_valid_coords(ca, (HAt, WAt))                # :449
    vq = coordinates.get_valid_coords(cq, (HQt, WQt))                # :450
    valid = torch.logical_and(va, vq)
    ca, cq = ca[valid].to(torch.long), cq[valid].to(torch.long)      # :453-456
    pcd_a = lift_pcd(depth_a.unsqueeze(-1), cam_a, (ca[:, 1], ca[:, 0])) / 1000.   # :459
    pcd_q = lift_pcd(depth_q.unsqueeze(-1), cam_q, (cq[:, 1], cq[:, 0])) / 1000.   # :460
    save(f"g2_lift_{tag}", corrs=corrs.to(torch.int16), depth_a=depth_a.to(torch.int16), depth_q=depth_q.to(torch.int16),
         depth_is_float=np.bool_(depth_dtype == torch.float32),
         cam_a=cam_a, cam_q=cam_q, feat_hw=np.array([FH, FW]), size_a=np.array([HA, WA]), size_q=np.array([HQ, WQ]),
         valid=valid, pix_a=ca.to(torch.int16), pix_q=cq.to(torch.int16), pcd_a=pcd_a, pcd_q=pcd_q,
         pcd_dtype=str(pcd_a.dtype))


def gen_lift():
    K_nocs = [[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]]        # datasets.py:398
    K_toyl = [[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]]  # datasets.py:573
    lift_case("nocs", 480, 640, 480, 640, 192, 192, K_nocs, K_nocs, 21, torch.int32)
    lift_case("toyl", 480, 640, 480, 640, 192, 192, K_toyl, K_toyl, 22, torch.float32)
    lift_case("nonsquare", 375, 501, 240, 320, 192, 192, K_nocs, K_toyl, 23, torch.int32)
    lift_case("feat224", 224, 224, 224, 224, 224, 224, [[280.0, 0, 112.0], [0, 280.0, 112.0], [0, 0, 1]],
              [[280.0, 0, 112.0], [0, 280.0, 112.0], [0, 0, 1]], 24, torch.float32)


# ---------------------------------------------------------------------------------------------- G3
def _rand_rot(g):
    q = torch.randn(4, generator=g, dtype=torch.float64)
    q = q / q.norm()
    w, x, y, z = q
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def gen_kabsch():
    g = torch.Generator().manual_seed(31)
    bs, m = 12, 40
    A = torch.randn(bs, m, 3, generator=g) * 0.2
    B = torch.zeros_like(A)
    for b in range(bs):
        R = _rand_rot(g).float()
        t = torch.randn(3, generator=g) * 0.3
        B[b] = A[b] @ R.T + t + 0.002 * torch.randn(m, 3, generator=g)
    w = torch.rand(bs, m, generator=g)
    w[0] = 1.0
    w[1, ::2] = 0.0                       # zero weights
    w[2, :5] = -0.5                       # negative weights are clipped (common.py:20)
    A[3, :, 2] = 0.0                      # coplanar source
    B[3] = A[3] @ _rand_rot(g).float().T + 0.1
    B[4] = A[4] * torch.tensor([1.0, 1.0, -1.0])   # reflection: det correction must kick in
    w[5] = 0.0
    w[5, 3] = 1.0                         # single effective point
    w_in = w.clone()
    T = rigid_transform_3d(A.clone(), B.clone(), w_in)              # reference common.py:7-45 (mutates w_in)
    T_now = rigid_transform_3d(A.clone(), B.clone(), None)
    save("g3_kabsch", A=A, B=B, w=w, T=T, T_noweights=T_now)


# ---------------------------------------------------------------------------------------------- G4
def synthetic_corr_set(n, seed, inlier_ratio=0.6, extent=0.15, dup=0):
    """n putative 3D-3D correspondences on an object-sized cloud, a share of them outliers."""
    g = torch.Generator().manual_seed(seed)
    src = (torch.rand(n, 3, generator=g) - 0.5) * 2 * extent + torch.tensor([0.0, 0.0, 0.8])
    R = _rand_rot(g).float()
    t = torch.randn(3, generator=g) * 0.1
    tgt = src @ R.T + t + 0.001 * torch.randn(n, 3, generator=g)
    n_out = int(n * (1 - inlier_ratio))
    out_idx = torch.randperm(n, generator=g)[:n_out]
    tgt[out_idx] = (torch.rand(n_out, 3, generator=g) - 0.5) * 2 * extent + tgt.mean(0)
    if dup:
        src[-dup:] = src[:dup]
        tgt[-dup:] = tgt[:dup]
    T = torch.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return src, tgt, T


def pointdsc_case(tag, n, num_layers, C, seed, extent=0.15, inlier_ratio=0.6, dup=0, pseed=0):
    cfg = dict(num_layers=num_layers, num_channels=C, num_iterations=10, ratio=0.1, sigma_d=0.1, k=40, nms_radius=0.1,
               inlier_threshold=0.1)
    model = PointDSC(in_dim=6, num_layers=num_layers, num_channels=C, num_iterations=10, ratio=0.1, sigma_d=0.1,
                     k=40, nms_radius=0.1)                     # exactly the kwargs init.py:41-50 forwards
    model.load_state_dict(analytic_pointdsc_params(num_layers, C, seed=pseed), strict=True)
    model.eval()
    src, tgt, T_gt = synthetic_corr_set(n, seed, inlier_ratio, extent, dup)
    with torch.no_grad():
        corr_pos = torch.cat([src, tgt], dim=-1)
        corr_pos = corr_pos - corr_pos.mean(0)                 # init.py:18-19
        s, t_ = src[None], tgt[None]
        src_dist = torch.norm((s[:, :, None, :] - s[:, None, :, :]), dim=-1)                     # PointDSC.py:151
        comp = src_dist - torch.norm((t_[:, :, None, :] - t_[:, None, :, :]), dim=-1)
        comp = torch.clamp(1.0 - comp ** 2 / model.sigma_spat ** 2, min=0)                        # :153
        feats = model.encoder(corr_pos[None].permute(0, 2, 1), comp).permute(0, 2, 1)            # :155
        nfeats = F.normalize(feats, p=2, dim=-1)                                                   # :156
        conf = model.classification(feats.permute(0, 2, 1)).squeeze(1)                            # :171
        rel = (conf.T >= conf) | (src_dist[0] >= model.nms_radius)
        is_local_max = rel.min(-1)[0]                                                              # :212-216
        seeds = model.pick_seeds(src_dist, conf, R=model.nms_radius, max_num=int(n * model.ratio))  # :174
        k = min(model.k, n - 1)
        knn_all = knn(nfeats, k=k, ignore_self=True, normalized=True)                             # :250
        seed_trans, seed_fit, init_trans, labels = model.cal_seed_trans(seeds, nfeats, s, t_)    # :182
        final = model.post_refinement(init_trans, s, t_)                                          # :186
        full = model({"corr_pos": corr_pos[None], "src_keypts": s, "tgt_keypts": t_, "testing": True})
        pose = get_pointdsc_pose(model, src, tgt, "cpu")                                          # init.py:10-29
        # number of strictly positive local maxima -> are the seeds well-defined (no zero-key ties)?
        n_pos_max = int(((conf[0] > 0) & is_local_max.bool()).sum())
    assert torch.equal(full["final_trans"][0], final[0])
    save(f"g4_pointdsc_{tag}", src=src, tgt=tgt, T_gt=T_gt, n=n, num_layers=num_layers, C=C, pseed=pseed,
         SC_rows=comp[0, :32], src_dist_rows=src_dist[0, :32], feat=feats[0], confidence=conf[0],
         is_local_max=is_local_max, seeds=seeds[0].to(torch.int16), n_pos_max=n_pos_max, knn_all=knn_all[0].to(torch.int16),
         seed_trans=seed_trans[0], seed_fitness=seed_fit[0], init_trans=init_trans[0], init_labels=labels[0],
         final_trans=final[0], final_labels=full["final_labels"][0], pose=pose)


def gen_pointdsc():
    pointdsc_case("l2c32_n41", 41, 2, 32, 41)
    pointdsc_case("l2c32_n128", 128, 2, 32, 42)
    pointdsc_case("l12c128_n128", 128, 12, 128, 43)
    pointdsc_case("l12c128_n500", 500, 12, 128, 44, extent=0.4)   # scene-sized: many local maxima
    pointdsc_case("l12c128_n500_obj", 500, 12, 128, 45, extent=0.12, dup=60)  # object-sized + duplicate rows
    pointdsc_case("l6c128_n200", 200, 6, 128, 46, inlier_ratio=0.3, pseed=1)
    gen_pointdsc_edge()


def gen_pointdsc_edge():
    """Edge sizes of the reference: k = n - 1 < 40, a single seed (int(n * 0.1) == 1), two seeds, and an outlier-dominated set."""
    pointdsc_case("l2c32_n10", 10, 2, 32, 47, inlier_ratio=0.8)           # 1 seed, k = 9
    pointdsc_case("l12c128_n12", 12, 12, 128, 48, inlier_ratio=0.8)       # 1 seed, k = 11
    pointdsc_case("l6c128_n22", 22, 6, 128, 49, inlier_ratio=0.7)         # 2 seeds, k = 21
    pointdsc_case("l12c128_n300_out", 300, 12, 128, 50, inlier_ratio=0.15, extent=0.3)


# ---------------------------------------------------------------------------------------------- G6
def gen_end_to_end():
    H = W = 48
    C = 32
    p = make_pair(3, H, W, C)
    cfg = dict(num_layers=2, C=32)
    model = PointDSC(in_dim=6, num_layers=2, num_channels=32, num_iterations=10, ratio=0.1, sigma_d=0.1, k=40, nms_radius=0.1)
    model.load_state_dict(analytic_pointdsc_params(2, 32), strict=True)
    model.eval()
    f1, f2, m1, m2 = p["feat_a"], p["feat_q"], p["mask_a"], p["mask_q"]
    roi1 = torch.nonzero(m1 == 1)
    roi2 = torch.nonzero(m2 == 1)
    a = f1[:, roi1[:, 0], roi1[:, 1]].T
    b = f2[:, roi2[:, 0], roi2[:, 1]].T
    dist = pdist(a, b, "inv_norm_cosine")
    min_dist, arg = torch.amin(dist, 1), torch.argmin(dist, 1)
    top2 = torch.topk(dist, 2, dim=1, largest=False)[0]
    torch.manual_seed(1)
    corrs = nn_correspondences(f1.clone(), f2.clone(), m1, m2, 0.25, 500, 5000, "cpu")
    sizes = torch.tensor([H, W])
    Ht, Wt = sizes
    ca = coordinates.scale_coords(corrs[:, :2].clone(), (H, W), (Ht, Wt))
    cq = coordinates.scale_coords(corrs[:, 2:].clone(), (H, W), (Ht, Wt))
    valid = torch.logical_and(coordinates.get_valid_coords(ca, (Ht, Wt)), coordinates.get_valid_coords(cq, (Ht, Wt)))
    ca, cq = ca[valid].to(torch.long), cq[valid].to(torch.long)
    cam = p["camera"].reshape(9)
    pcd_a = lift_pcd(p["depth_a"].unsqueeze(-1), cam, (ca[:, 1], ca[:, 0])) / 1000.
    pcd_q = lift_pcd(p["depth_q"].unsqueeze(-1), cam, (cq[:, 1], cq[:, 0])) / 1000.
    pose = get_pointdsc_pose(model, pcd_a, pcd_q, "cpu")
    anchor_pose = torch.eye(4)
    anchor_pose[:3, 3] = torch.tensor([0.01, -0.02, 0.8])
    pred_q = pose @ anchor_pose                                         # pipeline.py:320
    save("g6_end_to_end", pair_index=3, H=H, W=W, C=C, roi1=roi1, roi2=roi2, min_dist=min_dist, argmin=arg,
         gap=top2[:, 1] - top2[:, 0], valid=min_dist < 0.25, sampled_corrs=corrs, lift_valid=valid,
         pcd_a=pcd_a, pcd_q=pcd_q, pose=pose, pose_gt=p["pose"], anchor_pose=anchor_pose, pred_q=pred_q)


# ---------------------------------------------------------------------------------------------- G5
def gen_backbone():
    """Reference ImageTextFusion (models/fusion.py:533-625) and StandardDecoder (models/decoder.py:44-108) on closed-form
    weights and inputs.  fusion.py imports timm.models.layers {Mlp, DropPath, to_2tuple, to_ntuple}: timm is not installed,
    so a shim with the published semantics (fc1 -> GELU -> fc2; identity drop-path) stands in - the goldens therefore pin
    everything in fusion.py except timm's Mlp itself."""
    import torch.nn as nn
    from oracle.oryon_oracle import analytic_state_dict, hashed_tensor

    class Mlp(nn.Module):
        def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
            super().__init__()
            self.fc1 = nn.Linear(in_features, hidden_features or in_features)
            self.act = act_layer()
            self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)

        def forward(self, x):
            return self.fc2(self.act(self.fc1(x)))

    layers = types.ModuleType("timm.models.layers")
    layers.Mlp, layers.DropPath = Mlp, nn.Identity
    layers.to_2tuple = lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x, x)
    layers.to_ntuple = lambda n: (lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x,) * n)
    for name in ("timm", "timm.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["timm.models.layers"] = layers
    from models.fusion import ImageTextFusion          # reference
    from models.decoder import StandardDecoder         # reference

    fusion = ImageTextFusion("cpu").eval()
    fusion.load_state_dict(analytic_state_dict(fusion.state_dict(), seed=3), strict=True)
    decoder = StandardDecoder("cpu", True, True, input_dim=128, decoder_dims=[64, 32]).eval()
    decoder.load_state_dict(analytic_state_dict(decoder.state_dict(), seed=4), strict=True)
    B = 2
    img = hashed_tensor((B, 1024, 24, 24), 100, 0, 1.0)
    text = hashed_tensor((B, 1, 80, 768), 101, 0, 1.0)
    guid = [hashed_tensor((B, 512, 24, 24), 102, 0, 1.0), hashed_tensor((B, 256, 48, 48), 103, 0, 1.0),
            hashed_tensor((B, 128, 96, 96), 104, 0, 1.0)]
    with torch.no_grad():
        feats = fusion(img, text, guid)
        mask, featmap = decoder(feats, guid)
    save("g5_backbone", fusion_out=feats, mask=mask[:, :, ::2, ::2], featmap_sub=featmap[:, :, ::4, ::4],
         featmap_sum=featmap.double().sum(dim=(2, 3)), featmap_abs_sum=featmap.double().abs().sum(dim=(2, 3)),
         fusion_keys=np.array(list(fusion.state_dict().keys())), decoder_keys=np.array(list(decoder.state_dict().keys())))


# ---------------------------------------------------------------------------------------------- G7
def gen_metrics():
    from utils.metrics import compute_add, compute_adds, compute_RT_distances, mask_iou      # reference
    g = torch.Generator().manual_seed(71)
    pcd = (torch.rand(800, 3, generator=g).numpy() - 0.5) * 0.2
    n = 6
    pred, gt = np.tile(np.eye(4), (n, 1, 1)), np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        gt[i, :3, :3] = _rand_rot(g).numpy()
        gt[i, :3, 3] = torch.randn(3, generator=g).numpy() * 0.3 + np.array([0, 0, 0.8])
        dR = _rand_rot(g).numpy()
        ang = 0.02 * (i + 1)
        pred[i, :3, :3] = gt[i, :3, :3] @ (np.eye(3) * (1 - ang) + dR * ang)     # not exactly orthonormal: exercises the det normalisation
        pred[i, :3, 3] = gt[i, :3, 3] + 0.004 * (i + 1)
    add = np.array([compute_add(pcd, pred[i], gt[i]) for i in range(n)])
    adds = np.array([compute_adds(pcd, pred[i], gt[i]) for i in range(n)])
    theta, shift = compute_RT_distances(pred, gt)
    m1 = (torch.rand(3, 20, 20, generator=g) > 0.5)
    m2 = (torch.rand(3, 20, 20, generator=g) > 0.5)
    m2[2] = 0
    m1[2] = 0
    iou = mask_iou(m1.float(), m2.float())
    save("g7_metrics", pcd=pcd, pred=pred, gt=gt, add=add, adds=adds, theta=theta, shift=shift, mask1=m1, mask2=m2, iou=iou)



def gen_bop_metrics():
    """G9: the reference's Evaluator (utils/evaluator.py, compute_vsd=False) run for real on fabricated objects and poses:
    register_test (ADD(S)-0.1d, MSSD, MSPD, R / T errors, recalls, zero-pose and failed-pose bookkeeping), register_test_failure,
    get_means / get_latex_str, plus the raw my_mssd / my_mspd errors (bop_toolkit_lib/pose_error.py) and the symmetry sets of
    bop_toolkit_lib/misc.get_symmetry_transformations for an asymmetric, a discretely and a continuously symmetric model."""
    from utils.evaluator import Evaluator                                             # reference
    from bop_toolkit_lib.misc import get_symmetry_transformations, format_sym_set    # reference
    from bop_toolkit_lib.pose_error import my_mssd, my_mspd                           # reference
    from utils.pcd import get_diameter                                                # reference
    g = torch.Generator().manual_seed(91)
    infos = {
        "box": {"diameter": 180.0},
        "brick": {"diameter": 210.0, "symmetries_discrete": [[-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]]},
        "can": {"diameter": 150.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}],
                "symmetries_discrete": [[1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]]},
    }
    models, diams, symms = {}, {}, {}
    for i, (name, info) in enumerate(infos.items()):
        pts = (torch.rand(300 + 57 * i, 3, generator=g, dtype=torch.float64).numpy() - 0.5) * np.array([120.0, 90.0, 60.0 + 30 * i])
        if name == "can":                                     # a body of revolution about z
            r = np.hypot(pts[:, 0], pts[:, 1]).clip(1e-3)
            pts[:, :2] *= (45.0 / r)[:, None]
        models[name] = {"pts": pts}
        diams[name] = info["diameter"]
        symms[name] = get_symmetry_transformations(info, max_sym_disc_step=0.05)
    ev = Evaluator("g9", compute_vsd=False, compute_iou=True)
    ev.add_object_info(models, diams, symms)
    ev.init_test()
    K = np.array([[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]])
    names = list(infos)
    n = 12
    cls = [names[i % 3] for i in range(n)]
    gt = np.tile(np.eye(4), (n, 1, 1))
    anchor = np.tile(np.eye(4), (n, 1, 1))
    rel = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        gt[i, :3, :3] = _rand_rot(g).numpy()
        gt[i, :3, 3] = torch.randn(3, generator=g).numpy() * 0.08 + np.array([0.02, -0.03, 0.9])
        anchor[i, :3, :3] = _rand_rot(g).numpy()
        anchor[i, :3, 3] = torch.randn(3, generator=g).numpy() * 0.08 + np.array([0.0, 0.0, 0.8])
        err = np.eye(4)
        ang = [0.0, 0.01, 0.03, 0.08, 0.2, 0.6][i % 6]
        axis = torch.randn(3, generator=g).numpy()
        axis /= np.linalg.norm(axis)
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        err[:3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
        err[:3, 3] = torch.randn(3, generator=g).numpy() * [0.0, 0.002, 0.006, 0.02, 0.05, 0.1][i % 6]
        rel[i] = err @ gt[i] @ np.linalg.inv(anchor[i])       # pred_q = rel @ anchor = err @ gt
    rel[7] = np.eye(4)                                         # "failed pose": the identity came back
    rel[10] = 0.0                                              # "zero pose" (utils/evaluator.py:229-231)
    rel32, anchor32, gt_t = rel.astype(np.float32), anchor.astype(np.float32), gt.copy()
    mssd_raw, mspd_raw = np.zeros(n), np.zeros(n)
    failures = {3}
    for i in range(n):
        iou_a, iou_q = torch.tensor([0.5 + 0.04 * i]), torch.tensor([0.9 - 0.05 * i])
        if i in failures:
            ev.register_test_failure({"iou_a": iou_a, "iou_q": iou_q, "cls_id": [cls[i]], "instance_id": [f"inst{i}"]})
            continue
        pred_rel = torch.tensor(rel32[i])
        pred_q = pred_rel @ torch.tensor(anchor32[i])         # pipeline.py:320 (fp32)
        ev.register_test({"iou_a": iou_a, "iou_q": iou_q, "gt_pose": torch.tensor(gt_t[i]).unsqueeze(0), "pred_pose": pred_q.unsqueeze(0),
                          "pred_pose_rel": pred_rel.unsqueeze(0), "cls_id": [cls[i]], "camera": [K.copy()], "depth": [np.zeros((2, 2))],
                          "instance_id": [f"inst{i}"]})
        pq = pred_q.numpy().copy()
        if np.count_nonzero(rel32[i]) <= 1:
            pq = np.eye(4, dtype=np.float32)
        p16, g16 = pq.astype(np.float16), gt_t[i].astype(np.float16)
        sy = format_sym_set(symms[cls[i]])
        mssd_raw[i] = my_mssd(p16[:3, :3], np.expand_dims(p16[:3, 3], 1) * 1000, g16[:3, :3], np.expand_dims(g16[:3, 3], 1) * 1000,
                              models[cls[i]]["pts"], sy)
        mspd_raw[i] = my_mspd(p16[:3, :3], np.expand_dims(p16[:3, 3], 1) * 1000, g16[:3, :3], np.expand_dims(g16[:3, 3], 1) * 1000,
                              K, models[cls[i]]["pts"], sy)
    means = ev.get_means()
    out = {f"metric_{k}": np.asarray(v, dtype=np.float64) for k, v in ev.metrics.items() if k not in ("cls_id", "instance_id")}
    out.update({f"count_{k}": np.asarray(v) for k, v in ev.counts.items()})
    save("g9_bop_metrics", K=K, gt=gt_t, anchor=anchor32, rel=rel32, cls=np.array(cls), failures=np.array(sorted(failures)),
         mssd_raw=mssd_raw, mspd_raw=mspd_raw, latex=np.array(ev.get_latex_str()), mean_names=np.array(list(means)),
         mean_values=np.array([means[k] for k in means]), add_diam=np.array([get_diameter(models[c]["pts"]) / 1000.0 for c in names]),
         info_json=np.array(json.dumps(infos)), model_names=np.array(names),
         **{f"pts_{k}": v["pts"] for k, v in models.items()}, **{f"syms_{k}": format_sym_set(v) for k, v in symms.items()}, **out)


def gen_tokenizer():
    """G10: the reference's SimpleTokenizer (models/tokenizer.py:64-151) run on a FABRICATED merge table (a few hundred merges learnt
    here from the prompt corpus by plain BPE counting - the published 16e6 vocabulary file is not in the tree) and a set of prompts:
    templates, punctuation, digits, apostrophes, HTML entities, runs of blanks, upper case, non-ASCII bytes, and one prompt longer
    than the 77-token context.  `ftfy` is absent; its fix_text is stubbed with the identity, so the golden pins everything of the
    reference's encode path except ftfy's mojibake repair (a no-op on the datasets' plain-ASCII object names and templates)."""
    import gzip
    import collections
    ft = types.ModuleType("ftfy")
    ft.fix_text = lambda t: t
    sys.modules["ftfy"] = ft
    from models.tokenizer import SimpleTokenizer, bytes_to_unicode                    # reference
    names = ["mug", "laptop", "camera", "bowl", "can", "bottle", "toy car", "power drill", "rubber duck", "cereal box"]
    templates = ["a photo of a {}.", "a bad photo of the {}.", "a close-up photo of a {}.", "itap of my {}.", "a rendering of a {}.",
                 "a {} in a video game.", "art of the {}.", "a black and white photo of the {}.", "the origami {}.", "a low resolution photo of the {}."]
    corpus = [t.format(n) for n in names for t in templates]
    b2u = bytes_to_unicode()
    words = collections.Counter()
    import regex as re
    pat = re.compile(r"""'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+""", re.IGNORECASE)
    for line in corpus:
        for tok in re.findall(pat, line.lower()):
            u = "".join(b2u[b] for b in tok.encode("utf-8"))
            words[tuple(u[:-1]) + (u[-1] + "</w>",)] += 1
    merges = []
    for _ in range(400):
        pairs = collections.Counter()
        for w, c in words.items():
            for a, b in zip(w, w[1:]):
                pairs[(a, b)] += c
        if not pairs:
            break
        best = max(sorted(pairs), key=lambda p_: pairs[p_])
        merges.append(best)
        new = collections.Counter()
        for w, c in words.items():
            out, i = [], 0
            while i < len(w):
                if i < len(w) - 1 and (w[i], w[i + 1]) == best:
                    out.append(w[i] + w[i + 1]); i += 2
                else:
                    out.append(w[i]); i += 1
            new[tuple(out)] += c
        words = new
    bpe_path = os.path.join(OUT, "bpe_fabricated.txt.gz")
    with gzip.open(bpe_path, "wb") as f:
        f.write(("#version: fabricated for tests (not the CLIP vocabulary)\n" + "\n".join(" ".join(m) for m in merges) + "\n").encode("utf-8"))
    tok = SimpleTokenizer(bpe_path)
    texts = corpus[::7] + ["A  Photo   of  THE Mug!!", "it's the robot's toy-car (no. 42)", "caf\u00e9 &amp; cr\u00e8me &lt;bowl&gt;", "x",
                           "  leading and trailing blanks  ", "a photo of a " + " ".join(["very"] * 90) + " long prompt", "3d rendering, 100% real?"]
    ids = torch.stack([tok(t) for t in texts])
    print(f"fabricated BPE table: {len(merges)} merges, {len(texts)} prompts, longest {int((ids != 0).sum(1).max())} tokens")
    save("g10_tokenizer", texts=np.array(texts), ids=ids.numpy(), n_merges=len(merges))

def gen_data():
    """G8: raw samples -> utils/data/common.preprocess_item -> utils/augmentations.resize -> datasets.CollateWrapper, all
    REFERENCE code.  The modules import with permissive stubs for packages that are imported but never called on this path
    (plyfile, open3d, vispy, ...).  torchvision is absent too, and its `functional.resize` IS called by augmentations.resize:
    it is replaced by oracle.tv_resize, a restatement of torchvision 0.13's tensor resize on torch `interpolate` - so this
    golden pins the reference's own arithmetic (mask selection, box, sizes, scaling of boxes / correspondences, collate
    layout and dtypes) and torch's resampling, not torchvision's wrapper."""
    class _Any(types.ModuleType):
        def __getattr__(self, k):
            if k.startswith("__"):
                raise AttributeError(k)
            return type(k, (), {})
    for name in ("plyfile", "open3d", "trimesh", "vispy", "matplotlib", "matplotlib.pyplot", "omegaconf.dictconfig", "torchvision",
                 "torchvision.transforms", "torchvision.transforms.functional"):
        sys.modules[name] = _Any(name)
    sys.modules["omegaconf.dictconfig"].DictConfig = dict
    from oracle.oryon_oracle import tv_resize

    class _Mode:
        BILINEAR, NEAREST = "bilinear", "nearest"
    tvf = sys.modules["torchvision.transforms.functional"]
    tvf.InterpolationMode = _Mode
    tvf.resize = lambda img, size, interpolation: tv_resize(img, size, interpolation)
    sys.modules["torchvision.transforms"].Compose = lambda l: l
    sys.modules["torchvision.transforms"].functional = tvf
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    from utils.data import common  # noqa: E402  (reference)
    import utils.augmentations as aug  # noqa: E402  (reference)
    import datasets as ref_datasets  # noqa: E402  (reference)
    from oryon_amd.data import make_raw_item
    H, W, size, corr_n = 96, 128, (56, 56), 8
    g = torch.Generator().manual_seed(11)
    data, corrs_in = [], []
    for i in range(2):
        raw_a, raw_q = make_raw_item(2 * i, H, W), make_raw_item(2 * i + 1, H, W)
        item_a, item_q = common.preprocess_item(raw_a), common.preprocess_item(raw_q)
        corrs = torch.stack([torch.randint(0, H, (20,), generator=g), torch.randint(0, W, (20,), generator=g),
                             torch.randint(0, H, (20,), generator=g), torch.randint(0, W, (20,), generator=g)], dim=1)
        corrs_in.append(corrs.clone())
        item_a, item_q, res_corrs = aug.resize(size)((item_a, item_q, corrs))
        pose = np.eye(4) * (i + 1)
        data.append((item_a, item_q, ["mug"] + ["a photo of a mug"] * 2, res_corrs[:corr_n], res_corrs, pose, "mug", f"pair{i}", True))
    batch = ref_datasets.CollateWrapper(corr_n)(data)
    out = {"size": np.asarray(size), "hw": np.asarray((H, W)), "corr_n": corr_n, "corrs_in": torch.stack(corrs_in)}
    for side in ("anchor", "query"):
        for k in ("rgb", "mask", "depth", "camera", "pose", "box", "sizes"):
            out[f"{side}_{k}"] = batch[side][k]
        out[f"{side}_orig_depth"] = torch.stack(batch[side]["orig_depth"])
    out["corrs"], out["valid"], out["pose"] = batch["corrs"], batch["valid"], batch["pose"]
    save("g8_data", **out)


# ---------------------------------------------------------------------------------------------- G11
def _ransac_data(kind, n, n_in, sigma, g):
    """A [n,3], B [n,3] float32: n_in rows related by a random rigid motion + N(0, sigma) noise, the rest uniform in the box."""
    ext = 0.15
    A = g.uniform(-ext, ext, (n, 3))
    R = _rand_rot(torch.Generator().manual_seed(int(g.integers(1 << 30)))).double().numpy()
    t = np.array([g.uniform(-0.2, 0.2), g.uniform(-0.2, 0.2), g.uniform(0.4, 0.7)])
    Bm = A @ R.T + t + g.normal(0.0, sigma, (n, 3))
    out = t + g.uniform(-ext, ext, (n, 3))
    is_in = np.zeros(n, bool)
    is_in[g.permutation(n)[:n_in]] = True
    if kind == "all_out":
        is_in[:] = False
    Bm = np.where(is_in[:, None], Bm, out)
    return A.astype(np.float32), Bm.astype(np.float32)


def gen_ransac():
    """utils/geo6d.py:75-120 on seeded problems.  The index table the run will draw is recorded first (one bulk randint gives the rows
    of the reference's per-iteration calls: the comparison with the restatement below would fail otherwise), then the reference's
    own function runs from the same seed.  Every fixture's conditions are asserted; a seed that misses one is redrawn.
    Points are float32 values handed to the reference as float64 arrays, so its fits and its inlier test are float64."""
    sys.modules["cv2"].imshow = sys.modules["cv2"].waitKey = lambda *a, **k: None
    if "numpy.lib.function_base" not in sys.modules:
        try:
            import numpy.lib.function_base  # noqa: F401
        except ImportError:
            fb = types.ModuleType("numpy.lib.function_base")
            fb.append = np.append
            sys.modules["numpy.lib.function_base"] = fb
    from utils.geo6d import best_fit_transform_with_RANSAC as ref_ransac  # noqa: E402  (reference)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ransac_restatement as rr  # noqa: E402  (ours)

    REFP = dict(match_err=0.001, fix_percent=0.9999)            # pipeline.py:463
    # tag, n, inliers, sigma, K, parameters, kind, what must hold.  (1, 3, 5, 6 share K and parameters: max_iter, match_err and
    # fix_percent are per-call arguments of the kernel, so these four run as ONE batch of mixed n in the GPU test)
    cases = [
        ("1_best_of_k", 500, 300, 2e-5, 256, REFP, "mixed", dict(exited=False, min_count=20, max_excl=0.10)),
        ("2_exit_sampled", 200, 160, 1e-3, 256, dict(match_err=0.015, fix_percent=0.7), "mixed", dict(exited=True, k_pos=True, min_count=20, max_excl=0.10)),
        ("3_exit_at_0", 64, 64, 2e-5, 256, REFP, "mixed", dict(exited=True, k_zero=True, max_excl=0.10)),
        # 50 % of 37 rows is 18: the bound of 20 on the winner's count needs 20 inlier rows (54 %)
        ("4_n37", 37, 20, 2e-5, 128, REFP, "mixed", dict(min_count=20, max_excl=0.10)),
        ("5_all_zero", 500, 0, 0.0, 256, REFP, "all_out", dict(zero=True, distinct4=True, max_excl=0.10)),
        ("6_n3", 3, 3, 2e-5, 256, REFP, "mixed", dict(zero=True)),
        ("7_workload", 500, 300, 2e-5, 10000, REFP, "mixed", dict(min_count=20, max_excl=0.02)),
    ]
    for tag, n, n_in, sigma, K, prm, kind, want in cases:
        for seed in range(1000, 3000):
            A, B = _ransac_data(kind, n, n_in, sigma, np.random.default_rng(seed))
            A64, B64 = A.astype(np.float64), B.astype(np.float64)
            np.random.seed(seed)
            idx = np.random.randint(0, n, (K, 4))
            np.random.seed(seed)
            t0 = time.perf_counter()
            pose = np.asarray(ref_ransac(A64, B64, max_iter=K, **prm), np.float64)
            t_ref = time.perf_counter() - t0
            state = np.random.get_state()
            t0 = time.perf_counter()
            r = rr.restate(A64, B64, idx, K, prm["match_err"], prm["fix_percent"])
            t_res = time.perf_counter() - t0
            ok = True
            n_excl = 0
            if n >= 4:
                bad = rr.rank_deficient(idx, K)
                n_excl = int(bad.sum())
                near = np.abs(r["err"][~bad] - prm["match_err"]) < rr.G
                ok &= not near.any() and n_excl <= want["max_excl"] * K and (r["winner"] <= 0 or not bad[r["winner"]])
            if "exited" in want:
                ok &= r["exited"] == want["exited"]
            if want.get("k_pos"):
                ok &= r["winner"] > 0
            if want.get("k_zero"):
                ok &= r["winner"] == 0
            if "min_count" in want:
                ok &= r["winner"] >= 0 and r["counts"][r["winner"]] >= want["min_count"]
            if want.get("zero"):
                ok &= r["winner"] == -1 and not pose.any()
            if want.get("distinct4"):
                ok &= all(len(set(row.tolist())) == 4 for row in idx)
            if not ok:
                continue
            d = float(np.abs(pose - r["pose"]).max())
            assert d <= 1e-5, (tag, seed, d)
            print(f"ransac_{tag}: seed {seed}, winner {r['winner']}, exited {r['exited']}, count "
                  f"{int(r['counts'][r['winner']]) if r['winner'] >= 0 else 0}, {n_excl} rank-deficient rows of {K}, |ref - restatement| {d:.2e}; "
                  f"CPU time on this host: reference {t_ref:.3f} s, restatement {t_res:.3f} s")
            save(f"ransac_{tag}", A=A, B=B, idx=idx.astype(np.int32), max_iter=np.int32(K), match_err=np.float64(prm["match_err"]),
                 fix_percent=np.float64(prm["fix_percent"]), pose=pose, seed=np.int64(seed), state_words=state[1][:8].copy(),
                 state_pos=np.int64(state[2]))
            break
        else:
            raise RuntimeError(f"ransac_{tag}: no seed satisfies the fixture's conditions")


# ---------------------------------------------------------------------------------------------- G11 (VSD)
def gen_vsd():
    """g11_vsd: the reference's Evaluator with compute_vsd=True run for real (add_object_info, register_test, register_test_failure,
    get_means, get_latex_str) and bop_toolkit_lib/pose_error.vsd called directly, on the closed-form meshes, poses and test depth
    images of oryon_amd/synth.py.  The one thing the reference cannot do here - bop_toolkit_lib/renderer_vispy (vispy + EGL + a GL
    driver) - is replaced by a stand-in module whose RendererVispy renders with oryon_amd.evaluation.rasterize_depth, the numpy
    statement of the project's rasteriser; everything downstream of the depth render is the reference's own code.  The counts are
    taken with the reference's depth_im_to_dist_im_fast and visibility functions on the same renders."""
    from oryon_amd import synth
    from oryon_amd.evaluation import rasterize_depth

    class RendererVispy:
        def __init__(self, width, height, mode="depth"):
            self.width, self.height, self.models = width, height, {}

        def my_add_object(self, model, obj_id):
            self.models[obj_id] = model

        def render_object(self, obj_id, R, t, fx, fy, cx, cy):
            P = np.eye(4, dtype=np.float32)
            P[:3, :3], P[:3, 3] = R, np.asarray(t).squeeze()
            K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
            m = self.models[obj_id]
            return {"depth": rasterize_depth(P, K, m["pts"], m["faces"], self.height, self.width)}
    stand_in = types.ModuleType("bop_toolkit_lib.renderer_vispy")
    stand_in.RendererVispy = RendererVispy
    sys.modules["bop_toolkit_lib.renderer_vispy"] = stand_in
    from utils.evaluator import Evaluator                                             # reference
    from bop_toolkit_lib.misc import get_symmetry_transformations, depth_im_to_dist_im_fast    # reference
    from bop_toolkit_lib import pose_error, visibility                                # reference
    objects = synth.vsd_objects()
    models = {k: {"pts": o["pts"], "faces": o["faces"]} for k, o in objects.items()}
    diams = {k: o["diameter"] for k, o in objects.items()}
    symms = {k: get_symmetry_transformations({"diameter": o["diameter"]}, max_sym_disc_step=0.05) for k, o in objects.items()}
    H, W, K = synth.VSD_H, synth.VSD_W, np.array(synth.VSD_K)
    gt, pred = synth.vsd_poses()
    cls, n = list(synth.VSD_CLS), len(synth.VSD_CLS)
    rel32, anchor32 = pred.astype(np.float32), np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    ev = Evaluator("g11", compute_vsd=True, compute_iou=True)
    ev0 = Evaluator("g11", compute_vsd=False, compute_iou=True)
    for e in (ev, ev0):
        e.add_object_info(models, diams, symms)
        e.init_test()
    renderer = ev.renderer
    assert isinstance(renderer, RendererVispy)
    taus, delta = ev.vsd_taus, ev.vsd_delta
    counts, errors, crops = np.zeros((n, 2 + len(taus)), np.int32), np.zeros((n, len(taus))), {}
    for i in range(n):
        p16, g16 = (rel32[i] @ anchor32[i]).astype(np.float16), gt[i].astype(np.float16)
        Re, te, Rg, tg = p16[:3, :3], np.expand_dims(p16[:3, 3], 1) * 1000, g16[:3, :3], np.expand_dims(g16[:3, 3], 1) * 1000
        d_gt = renderer.render_object(cls[i], Rg, tg, K[0, 0], K[1, 1], K[0, 2], K[1, 2])["depth"]
        d_est = renderer.render_object(cls[i], Re, te, K[0, 0], K[1, 1], K[0, 2], K[1, 2])["depth"]
        depth = synth.vsd_test_depth(d_gt)
        errors[i] = pose_error.vsd(Re, te, Rg, tg, depth, K, delta, taus, True, diams[cls[i]], renderer, cls[i])
        dist_t, dist_g, dist_e = (depth_im_to_dist_im_fast(d, K) for d in (depth, d_gt, d_est))
        vis_g = visibility.estimate_visib_mask_gt(dist_t, dist_g, delta, visib_mode="bop19")
        vis_e = visibility.estimate_visib_mask_est(dist_t, dist_e, vis_g, delta, visib_mode="bop19")
        inter = np.logical_and(vis_g, vis_e)
        dists = np.abs(dist_g[inter] - dist_e[inter]) / diams[cls[i]]
        counts[i] = [np.logical_or(vis_g, vis_e).sum(), inter.sum()] + [(dists >= tau).sum() for tau in taus]
        u = counts[i, 0]
        assert np.array_equal(errors[i], (counts[i, 2:] + (u - counts[i, 1])) / float(u) if u else np.ones(len(taus))), i
        if i == 1:
            crops["crop_gt_1"] = d_gt[230:278, 270:334].copy()
        if i == 3:
            crops["crop_est_3"] = d_est[200:248, 290:354].copy()
        iou_a, iou_q = torch.tensor([0.5 + 0.04 * i]), torch.tensor([0.9 - 0.05 * i])
        for e in (ev, ev0):
            if i in synth.VSD_FAILURES:
                e.register_test_failure({"iou_a": iou_a, "iou_q": iou_q, "cls_id": [cls[i]], "instance_id": [f"inst{i}"]})
                continue
            pred_rel = torch.tensor(rel32[i])
            e.register_test({"iou_a": iou_a, "iou_q": iou_q, "gt_pose": torch.tensor(gt[i]).unsqueeze(0),
                             "pred_pose": (pred_rel @ torch.tensor(anchor32[i])).unsqueeze(0), "pred_pose_rel": pred_rel.unsqueeze(0),
                             "cls_id": [cls[i]], "camera": [K.copy()], "depth": [depth], "instance_id": [f"inst{i}"]})
        print(f"vsd pair {i} ({cls[i]}): counts {counts[i].tolist()}, errors {np.round(errors[i], 3).tolist()}")
    assert (counts[:, 0] > 0).all() and (errors[0] == 0).all() and (errors[5] == 1).all()
    means = ev.get_means()
    out = {f"metric_{k}": np.asarray(v, dtype=np.float64) for k, v in ev.metrics.items() if k not in ("cls_id", "instance_id")}
    out.update({f"count_{k}": np.asarray(v) for k, v in ev.counts.items()})
    out.update(crops)
    save("g11_vsd", K=K, hw=np.array([H, W]), gt=gt, pred=pred, cls=np.array(cls), failures=np.array(synth.VSD_FAILURES),
         iou_a=np.array([0.5 + 0.04 * i for i in range(n)], np.float32), iou_q=np.array([0.9 - 0.05 * i for i in range(n)], np.float32),
         taus=np.asarray(taus, np.float64), delta=np.float64(delta), diameters=np.array([diams[c] for c in cls]), counts=counts,
         errors=errors, crop_gt_1_origin=np.array([230, 270]), crop_est_3_origin=np.array([200, 290]),
         mean_names=np.array(list(means)), mean_values=np.array([means[k] for k in means], np.float64),
         latex=np.array(ev.get_latex_str()), latex_no_vsd=np.array(ev0.get_latex_str()), **out)


# ---------------------------------------------------------------------------------------------- validation step (floss_*)
def gen_feature_loss():
    """floss_*.npz: the reference's FeatureLoss.forward (losses.py:64-141) run for real on the CPU - the form that is fp32 throughout -
    on seeded inputs, with the stubs of SURVEY Appendix C plus permissive ones for the packages utils/metrics.py imports and never
    calls here.  Stored per fixture: the maps (fp16-valued, as float16), corrs, valid, the pool tables the run drew, logits and
    ground-truth masks; the reference's losses, results and per-correspondence distances; compute_fmr of the positives; the float64
    top-2 gap of every row's penalised cost.
    Asserted (a seed that misses is redrawn):
      * every row of a fixture in GAP has a top-2 gap >= 1e-5 - except rows whose positive descriptor is zero: all their costs are
        exactly 0.5 in any arithmetic (every product is 0), the lowest unpenalised position wins, `gap_exempt` marks them;
      * fixtures outside GAP (penalised ties are their point): no PENALISED candidate's float64 cost d + penalty lies within 1e-5 of
        the midpoint of two neighbouring float32 values, so the float32 sum rounds the same way whatever the last bits of d; a row
        that has unpenalised candidates (one of them wins) has its gap >= 1e-5 like everywhere else."""
    class _Any(types.ModuleType):
        def __getattr__(self, k):
            if k.startswith("__"):
                raise AttributeError(k)
            return type(k, (), {})
    for name in ("tqdm", "sklearn", "sklearn.neighbors", "scipy.optimize"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = _Any(name)
    if isinstance(sys.modules.get("tqdm"), _Any):
        sys.modules["tqdm"].tqdm = lambda x, *a, **k: x
    import losses as ref_losses  # noqa: E402  (reference)
    from utils.metrics import compute_fmr as ref_fmr  # noqa: E402  (reference)
    from types import SimpleNamespace as NS
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import feature_loss_restatement as fr  # noqa: E402  (ours)

    # tag, B, invalid pairs, C, (FH, FW), image, N, hard negatives
    cases = [("1_rescale", 3, (1,), 32, (40, 40), 48, 64), ("2_nonsquare", 2, (), 20, (40, 44), 48, 37),
             ("3_pool", 2, (), 32, (48, 48), 56, 500), ("4_c256", 1, (), 256, (16, 16), 32, 64), ("5_disc", 1, (), 8, (6, 6), 6, 16),
             ("6_zero_dup_border", 2, (), 32, (24, 24), 24, 32), ("7_none_valid", 2, (0, 1), 32, (24, 24), 24, 32)]
    GAP = ("1_rescale", "2_nonsquare", "3_pool", "4_c256", "6_zero_dup_border")
    args = NS(loss=NS(pos_margin=0.2, neg_margin=0.9, neg_kernel_size=5, hard_negatives=True, mask_type="dice"), test=NS(mask_threshold=0.5))
    real_multinomial, real_cuda = torch.multinomial, torch.Tensor.cuda
    for tag, B, invalid, C, (FH, FW), IMG, N in cases:
        for seed in range(100, 400):
            g = torch.Generator().manual_seed(seed)
            corrs = torch.randint(0, IMG, (B, N, 4), generator=g)
            if tag == "6_zero_dup_border":
                corrs[:, 1] = corrs[:, 0]                                  # duplicates
                corrs[:, 2] = torch.tensor([0, 0, IMG - 1, IMG - 1])       # the corners
                corrs[:, 3] = torch.tensor([IMG - 1, 0, 0, IMG - 1])
                corrs[:, 4, :2] = torch.tensor([12, 12])
            fa = torch.randn(B, C, FH, FW, generator=g)
            fq = torch.randn(B, C, FH, FW, generator=g)
            pix = torch.from_numpy(fr.feature_pixels(corrs.numpy(), (IMG, IMG), (FH, FW)))
            for b in range(B):                                              # query = anchor + noise of a per-correspondence size
                nz = torch.rand(N, generator=g) * 1.5
                fq[b][:, pix[b, :, 2], pix[b, :, 3]] = fa[b][:, pix[b, :, 0], pix[b, :, 1]] + nz[None] * torch.randn(C, N, generator=g)
            if tag == "6_zero_dup_border":
                fa[0][:, 12, 12] = 0.0                                      # a zero descriptor at a positive (corrs[0, 4]) ...
                fa[1][:, 3, 17] = 0.0                                       # ... and one that is only in the pool
                fq[1][:, 20, 5] = 0.0
            fa, fq = fa.half().float(), fq.half().float()
            logits_a = (3.0 * torch.randn(B, 1, FH, FW, generator=g)).half().float()
            logits_q = (3.0 * torch.randn(B, 1, FH, FW, generator=g)).half().float()
            yy, xx = torch.meshgrid(torch.arange(IMG), torch.arange(IMG), indexing="ij")
            gt_a = torch.stack([((yy - IMG // 2 - b) ** 2 + (xx - IMG // 2) ** 2 < (IMG // 3) ** 2).float() for b in range(B)])
            gt_q = torch.stack([((yy > IMG // 4) & (yy < IMG - 2 - b) & (xx > IMG // 5)).float() for b in range(B)])
            valid = torch.tensor([0.0 if b in invalid else 1.0 for b in range(B)])
            batch = {"corrs": corrs.clone(), "valid": valid, "anchor": {"rgb": torch.zeros(B, 3, IMG, IMG), "mask": gt_a},
                     "query": {"rgb": torch.zeros(B, 3, IMG, IMG), "mask": gt_q}}
            outputs = {"featmap_a": fa, "featmap_q": fq, "mask_a": logits_a, "mask_q": logits_q}
            drawn = []

            def recording_multinomial(*a, **k):
                r = real_multinomial(*a, **k)
                drawn.append(r.clone())
                return r
            floss = ref_losses.FeatureLoss(args, "cpu")
            torch.manual_seed(seed)
            torch.multinomial, torch.Tensor.cuda = recording_multinomial, (lambda self, *a, **k: self)    # losses.py:109-111 on a CPU host
            try:
                t0 = time.perf_counter()
                losses, results = floss.forward(batch, outputs)
                t_ref = time.perf_counter() - t0
            finally:
                torch.multinomial, torch.Tensor.cuda = real_multinomial, real_cuda
            n_valid = int(valid.sum())
            HW = FH * FW
            pool = None
            if HW > 2000:
                assert len(drawn) == 2 * n_valid
                pool = torch.zeros(B, 2, 2000, dtype=torch.int64)
                it = iter(drawn)
                for side in (0, 1):
                    for b in range(B):
                        if valid[b] == 1:
                            pool[b, side] = next(it)
            # per-correspondence distances with the reference's own expressions (losses.py:82,91-93)
            gtc = torch.clamp(ref_losses.rescale_coords(corrs.clone(), (IMG, IMG), (FH, FW)), min=0, max=FH - 1)
            assert np.array_equal(gtc.numpy(), pix.numpy()), "coordinate restatement differs from the reference"
            pos_a, pos_q = floss.sample_positives(fa, fq, gtc, valid)

            def rows_at(fm, yx):
                yx = yx.long()
                return torch.stack([fm[b][:, yx[b, :, 0], yx[b, :, 1]].T for b in range(B)])
            d_pos = 0.5 * (-1 * F.cosine_similarity(pos_a, pos_q, dim=2) + 1)
            d_neg_a = 0.5 * (-1 * F.cosine_similarity(pos_a, rows_at(fa, results["neg_a"]), dim=2) + 1)
            d_neg_q = 0.5 * (-1 * F.cosine_similarity(pos_q, rows_at(fq, results["neg_q"]), dim=2) + 1)
            for b in range(B):
                if valid[b] != 1:
                    d_pos[b], d_neg_a[b], d_neg_q[b] = 0.0, 0.0, 0.0
            fmr = ref_fmr(pos_a, pos_q, 0.25, 0.05).numpy()
            # float64 costs: gaps, margins to the float32 rounding boundaries
            gap = np.full((B, 2, N), np.inf)
            exempt = np.zeros((B, 2, N), dtype=bool)
            margin = np.inf
            for b in range(B):
                if valid[b] != 1:
                    continue
                for side, fm in ((0, fa), (1, fq)):
                    rows = fr.unit(fm[b].reshape(C, HW).T.double().numpy())
                    pl = np.arange(HW) if pool is None else pool[b, side].numpy()
                    yx = pix[b].numpy()[:, 2 * side:2 * side + 2]
                    p = rows[yx[:, 0] * FW + yx[:, 1]]
                    d = 0.5 * (1.0 - p @ rows[pl].T)
                    for n in range(N):
                        pen = fr.penalty32(yx[n, 0], yx[n, 1], pl // FW, pl % FW, 5).astype(np.float64)
                        c = np.sort(d[n] + pen)
                        gap[b, side, n] = c[1] - c[0]
                        exempt[b, side, n] = not p[n].any()
                        if tag not in GAP and (pen == 0).any() and gap[b, side, n] < 1e-5:
                            margin = 0.0                                    # an unpenalised winner needs its gap like everywhere else
                        if tag not in GAP:
                            v = (d[n] + pen)[pen > 0]
                            if v.size == 0:
                                continue
                            f32 = v.astype(np.float32)
                            lo = np.minimum(f32, np.nextafter(f32, np.float32(-np.inf))).astype(np.float64)
                            hi = np.maximum(f32, np.nextafter(f32, np.float32(np.inf))).astype(np.float64)
                            mids = np.stack([(f32.astype(np.float64) + lo) / 2, (f32.astype(np.float64) + hi) / 2])
                            margin = min(margin, float(np.abs(mids - v[None]).min()))
            if tag in GAP and not (gap[~exempt] >= 1e-5).all():
                continue
            if tag not in GAP and not margin >= 1e-5:
                continue
            r = fr.restate(fa.numpy(), fq.numpy(), corrs.numpy(), valid.numpy(), (IMG, IMG), None if pool is None else pool.numpy())
            want_idx = np.stack([results["neg_a"].numpy(), results["neg_q"].numpy()], axis=1)
            got_idx = np.stack([r["neg_idx"] // FW, r["neg_idx"] % FW], axis=-1)
            assert np.array_equal(want_idx, got_idx), (tag, seed, "restatement argmin differs from the reference")
            if tag == "6_zero_dup_border":
                assert exempt.sum() == 1 and exempt[0, 0, 4]
            if tag == "5_disc":                         # the point of the fixture: some positive has its whole pool inside the disc
                yx = pix[0].numpy()
                far = [(np.hypot(np.arange(HW) // FW - y, np.arange(HW) % FW - x) >= 5).any() for y, x in yx[:, :2]]
                if all(far):
                    continue
            print(f"floss_{tag}: seed {seed}, min gap {gap[~exempt].min() if (~exempt).any() and np.isfinite(gap).any() else float('nan'):.2e}, "
                  f"losses {[float(losses[k]) for k in ('mask', 'pos', 'neg')]}, reference forward {t_ref:.3f} s on this host")
            save(f"floss_{tag}", feat_a=fa.numpy().astype(np.float16), feat_q=fq.numpy().astype(np.float16), corrs=corrs.numpy().astype(np.int32),
                 valid=valid.numpy(), image_hw=np.array([IMG, IMG], np.int32), pool=(np.zeros((0,), np.int32) if pool is None else pool.numpy().astype(np.int32)),
                 logits_a=logits_a.numpy().astype(np.float16), logits_q=logits_q.numpy().astype(np.float16), gt_a=gt_a.numpy().astype(np.uint8),
                 gt_q=gt_q.numpy().astype(np.uint8), seed=np.int64(seed),
                 loss_mask=np.float32(losses["mask"]), loss_pos=np.float32(losses["pos"]), loss_neg=np.float32(losses["neg"]),
                 neg_a=results["neg_a"], neg_q=results["neg_q"], mask_a=results["mask_a"].numpy().astype(np.uint8),
                 mask_q=results["mask_q"].numpy().astype(np.uint8), iou_a=results["iou_a"], iou_q=results["iou_q"],
                 d_pos=d_pos, d_neg_a=d_neg_a, d_neg_q=d_neg_q, fmr=fmr, gap=gap, gap_exempt=exempt, has_gap=np.bool_(tag in GAP))
            break
        else:
            raise RuntimeError(f"floss_{tag}: no seed satisfies the fixture's conditions")


# ---------------------------------------------------------------------------------------------- training step (flossgrad_*)
def gen_feature_loss_grad():
    """flossgrad_*.npz: the gradients torch autograd gives the reference's FeatureLoss.forward (losses.py:64-141) on the CPU, for the
    inputs and the seed of every floss_*.npz, of 1.0 mask + 0.5 pos + 0.5 neg (config.yaml's loss.w) with respect to the two maps and
    the two logit tensors; fixture 1 a second time with neg_margin = 0.2 (`1_rescale_m02`), where part of the negative rows is
    clamped.  (The files are not named floss_grad_*: tests/test_feature_loss_restatement.py takes every floss_*.npz for a forward
    fixture.)  Stored as fp32 - the zero descriptor of fixture 6 produces entries of 1e5 - the map gradients sparsely: `pix_a`,
    `pix_q` [K] = pair * FH * FW + pixel of every pixel some slot sits at, `vec_a`, `vec_q` [K,C]; the logit gradients dense.
    Asserted: the run's negatives are the forward fixture's; every element outside the listed pixels is exactly 0; every valid row's
    float64 |d_pos - m_pos| and |m_neg - d_neg| is >= 1e-5; a fixture with valid pairs has active and clamped positive rows; the file is
    no larger than the largest forward fixture."""
    class _Any(types.ModuleType):
        def __getattr__(self, k):
            if k.startswith("__"):
                raise AttributeError(k)
            return type(k, (), {})
    for name in ("tqdm", "sklearn", "sklearn.neighbors", "scipy.optimize"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = _Any(name)
    if isinstance(sys.modules.get("tqdm"), _Any):
        sys.modules["tqdm"].tqdm = lambda x, *a, **k: x
    import glob
    import losses as ref_losses  # noqa: E402  (reference)
    from types import SimpleNamespace as NS
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import feature_loss_restatement as fr  # noqa: E402  (ours)
    import feature_loss_grad_restatement as gr  # noqa: E402  (ours)

    forward = sorted(glob.glob(os.path.join(OUT, "floss_*.npz")))
    limit = max(os.path.getsize(p) for p in forward)
    real_cuda = torch.Tensor.cuda
    for path in forward:
        tag = os.path.basename(path)[len("floss_"):-len(".npz")]
        z = np.load(path)
        for suffix, neg_margin in (("", 0.9),) + ((("_m02", 0.2),) if tag == "1_rescale" else ()):
            args = NS(loss=NS(pos_margin=0.2, neg_margin=neg_margin, neg_kernel_size=5, hard_negatives=True, mask_type="dice"),
                      test=NS(mask_threshold=0.5))
            fa, fq = (torch.from_numpy(z[k].astype(np.float32)).requires_grad_() for k in ("feat_a", "feat_q"))
            la, lq = (torch.from_numpy(z[k].astype(np.float32)).requires_grad_() for k in ("logits_a", "logits_q"))
            B, C, FH, FW = fa.shape
            IH, IW = (int(v) for v in z["image_hw"])
            valid = torch.from_numpy(z["valid"])
            batch = {"corrs": torch.from_numpy(z["corrs"]).long(), "valid": valid,
                     "anchor": {"rgb": torch.zeros(B, 3, IH, IW), "mask": torch.from_numpy(z["gt_a"]).float()},
                     "query": {"rgb": torch.zeros(B, 3, IH, IW), "mask": torch.from_numpy(z["gt_q"]).float()}}
            floss = ref_losses.FeatureLoss(args, "cpu")
            torch.manual_seed(int(z["seed"]))
            torch.Tensor.cuda = lambda self, *a, **k: self                   # losses.py:109-111 on a CPU host
            try:
                losses, results = floss.forward(batch, {"featmap_a": fa, "featmap_q": fq, "mask_a": la, "mask_q": lq})
            finally:
                torch.Tensor.cuda = real_cuda
            assert np.array_equal(results["neg_a"].numpy(), z["neg_a"]) and np.array_equal(results["neg_q"].numpy(), z["neg_q"]), tag
            total = 1.0 * losses["mask"] + 0.5 * losses["pos"] + 0.5 * losses["neg"]
            total.backward()
            grads = [np.zeros((B, C, FH, FW), np.float32) if t.grad is None else t.grad.numpy() for t in (fa, fq)]
            assert all(g.dtype == np.float32 and np.isfinite(g).all() for g in grads)
            pix = fr.feature_pixels(z["corrs"], (IH, IW), (FH, FW))
            neg_idx = np.stack([z["neg_a"][..., 0] * FW + z["neg_a"][..., 1], z["neg_q"][..., 0] * FW + z["neg_q"][..., 1]], axis=1).astype(np.int64)
            on = gr.touched(pix, z["valid"], neg_idx, (FH, FW))
            sparse = {}
            for s, key in enumerate("aq"):
                rows = grads[s].transpose(0, 2, 3, 1).reshape(B * FH * FW, C)
                flat = on[s].reshape(-1)
                assert not rows[~flat].any(), (tag, key, "gradient outside the touched pixels")
                sparse["pix_" + key] = np.flatnonzero(flat).astype(np.int32)
                sparse["vec_" + key] = rows[flat]
            r = fr.restate(z["feat_a"].astype(np.float32), z["feat_q"].astype(np.float32), z["corrs"], z["valid"], (IH, IW),
                           z["pool"].astype(np.int64) if z["pool"].size else None, 0.2, neg_margin)
            keep = z["valid"] == 1
            if keep.any():
                m_pos, m_neg = np.abs(r["d_pos"][keep] - 0.2).min(), np.abs(neg_margin - r["d_neg"][keep]).min()
                act = (r["d_pos"][keep] - 0.2 > 0).mean()
                act_neg = (neg_margin - r["d_neg"][keep] > 0).mean()
                assert m_pos >= 1e-5 and m_neg >= 1e-5, (tag, m_pos, m_neg)
                assert 0.0 < act < 1.0, (tag, act)
                print(f"flossgrad_{tag}{suffix}: closest row to a margin {m_pos:.1e} (pos) {m_neg:.1e} (neg); active rows {act:.0%} (pos) "
                      f"{act_neg:.0%} (neg); largest |gradient| {max(np.abs(g).max() for g in grads):.3g}")
            else:
                assert fa.grad is None and fq.grad is None
            name = f"flossgrad_{tag}{suffix}"
            save(name, fixture=np.array("floss_" + tag), pos_margin=np.float64(0.2), neg_margin=np.float64(neg_margin),
                 g=np.array([0.5, 0.25, 0.25], np.float32), g_mask=np.float32(0.5), grad_logits_a=la.grad.numpy()[:, 0],
                 grad_logits_q=lq.grad.numpy()[:, 0], **sparse)
            size = os.path.getsize(os.path.join(OUT, name + ".npz"))
            assert size <= limit, (name, size, limit)


def _reference_pcd_correspondences():
    """The reference's own `pcd_correspondences` (scripts/data/make_toyl_test.py:47-85), compiled from its file without importing the
    script around it (whose module level pulls in the dataset readers, PIL, matplotlib and an argument parser)."""
    import ast
    from typing import Tuple
    path = os.path.join(REF, "scripts", "data", "make_toyl_test.py")
    tree = ast.parse(open(path).read(), filename=path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "pcd_correspondences"]
    assert len(fn) == 1
    ns = {"torch": torch, "Tensor": torch.Tensor, "Tuple": Tuple}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["pcd_correspondences"]


def gen_gt_corrs():
    """Ground-truth correspondences: the reference's pcd_correspondences on the CPU (torch.cdist float64, amin / argmin, the multinomial
    draws) on the seeded clouds of tests/gt_corrs_restatement.py.  A fixture holds the RECORDED RESULTS and the seeds only: the tests
    regenerate the clouds.  Asserted here for every fixture, so that the reference's matmul-form cdist and the direct form of the
    definition cannot disagree on it: every row's best and second-best distance are exact duplicates or at least 1e-9 apart (relative
    to the larger), and no row's minimum lies within 1e-9 (relative) of the threshold."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gt_corrs_restatement as R
    ref_fn = _reference_pcd_correspondences()
    for name, (seed, n1, n2, threshold, max_corrs, tseed) in R.GOLDEN_CASES.items():
        f1, f2 = R.golden_clouds(name)
        assert f1.shape == (n1, 3) and f2.shape == (n2, 3)
        torch.manual_seed(tseed)
        i1, i2 = ref_fn(torch.as_tensor(f1), torch.as_tensor(f2), threshold, max_corrs)
        state = torch.get_rng_state().numpy().copy()
        # the margins, on the clouds the distance matrix was built on (the same draws again)
        torch.manual_seed(tseed)
        s1 = f1[torch.multinomial(torch.ones(n1, dtype=float), R.SAMPLE, replacement=False).numpy()] if n1 >= R.SAMPLE else f1
        s2 = f2[torch.multinomial(torch.ones(n2, dtype=float), R.SAMPLE, replacement=False).numpy()] if n2 >= R.SAMPLE else f2
        idx, d2, d2b = R.nearest(s1, s2, second=True)
        best, sec = np.sqrt(d2), np.sqrt(d2b)
        fin = np.isfinite(sec)
        with np.errstate(invalid="ignore"):
            gap = np.where(fin, (sec - best) / np.where(fin & (sec > 0), sec, 1.0), np.inf)
        assert np.all((gap == 0.0) | (gap >= 1e-9)), (name, float(gap[gap > 0].min()))
        margin = R.threshold_margin(d2, threshold)
        assert margin >= 1e-9, (name, margin)
        d_ref = torch.cdist(torch.as_tensor(s1), torch.as_tensor(s2), p=2)
        assert np.array_equal(torch.argmin(d_ref, dim=1).numpy(), idx), name
        err = float((torch.amin(d_ref, dim=1) - torch.as_tensor(best)).abs().max())
        n_kept = int(R.keep(d2, threshold).sum())
        print(f"gtcorr_{name}: {n1} x {n2}, kept {n_kept}, returned {i1.shape[0]}; |d - d_ref| <= {err:.1e}; smallest positive gap "
              f"{float(gap[gap > 0].min()) if (gap > 0).any() else float('inf'):.1e}, threshold margin {margin:.1e}")
        save(f"gtcorr_{name}", case=np.array(name), numpy_seed=np.int64(seed), torch_seed=np.int64(tseed), n1=np.int64(n1), n2=np.int64(n2),
             threshold=np.float64(threshold), max_corrs=np.int64(max_corrs), n_kept=np.int64(n_kept), idx1=i1.numpy(), idx2=i2.numpy(),
             rng_state=state)
        assert os.path.getsize(os.path.join(OUT, f"gtcorr_{name}.npz")) <= 256 * 1024


def gen_icp():
    """utils/geo6d.py:157-208 `icp` on the seeded clouds of tests/icp_restatement.py, on the CPU (sklearn's NearestNeighbors).  The
    reference returns no iteration count: its `nearest_neighbor` is called once per executed iteration, so the calls are counted.
    Asserted for every fixture and every iteration, so that neither the neighbour indices nor the iteration count can turn on a
    rounding: the relative gap between a row's best and second-best squared distance is >= 1e-9, | |prev - mean| - tolerance | >= 1e-9,
    and the second singular value of every H is >= 1e-2 of the first.  A seed that misses one is replaced in GOLDEN_CASES."""
    sys.modules["cv2"].imshow = sys.modules["cv2"].waitKey = lambda *a, **k: None
    if "numpy.lib.function_base" not in sys.modules:
        try:
            import numpy.lib.function_base  # noqa: F401
        except ImportError:
            fb = types.ModuleType("numpy.lib.function_base")
            fb.append = np.append
            sys.modules["numpy.lib.function_base"] = fb
    from utils import geo6d as ref_geo6d  # noqa: E402  (reference)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import icp_restatement as R  # noqa: E402  (ours)

    calls = [0]
    ref_nn = ref_geo6d.nearest_neighbor

    def counted(src, dst):
        calls[0] += 1
        return ref_nn(src, dst)
    ref_geo6d.nearest_neighbor = counted
    try:
        for name, c in R.GOLDEN_CASES.items():
            A, B, init, tol = R.golden_case(name)
            rec = {}
            # every fixture is recorded at its own tolerance AND at both TOLERANCE and FINE_TOLERANCE: tolerance is an argument of the
            # call, not of the pair, and the GPU test runs all fixtures as one batch
            for tag, t in (("", tol), ("_coarse", R.TOLERANCE), ("_fine", R.FINE_TOLERANCE)):
                calls[0] = 0
                T_ref = ref_geo6d.icp(A.copy(), B.copy(), init_pose=None if init is None else init.copy(), max_iterations=R.MAX_ITER, tolerance=t)
                iters = calls[0]
                r = R.icp(A, B, init, R.MAX_ITER, t)
                gap = float(np.abs(r["T"][:3] - T_ref).max())
                print(f"icp_{name} tolerance {t:g}: n {A.shape[0]}, iters {iters} (restatement {r['iters']}), |T - T_ref| <= {gap:.1e}, nn gap "
                      f"{r['nn_gap']:.1e}, convergence gap {r['conv_gap']:.1e}, s2/s1 >= {r['sv_ratio']:.2e}, det < 0 in {r['det_negative']} fits")
                assert r["nn_gap"] >= 1e-9 and r["conv_gap"] >= 1e-9 and r["sv_ratio"] >= 1e-2, name
                assert iters == r["iters"] and gap <= 1e-12, name
                if c["kind"] == "mirrored":
                    assert r["det_negative"] >= 1, name
                if c["kind"] == "far" and t == 1e-6:
                    assert iters == R.MAX_ITER, name
                if c["kind"] == "identity":
                    assert iters < R.MAX_ITER, name
                rec["T" + tag], rec["iters" + tag] = T_ref, np.int64(iters)
            save(f"icp_{name}", case=np.array(name), seed=np.int64(c["seed"]), A=A, B=B, has_init=np.int64(init is not None),
                 init_pose=np.eye(4) if init is None else init, tolerance=np.float64(tol), tolerance_coarse=np.float64(R.TOLERANCE), tolerance_fine=np.float64(R.FINE_TOLERANCE),
                 max_iterations=np.int64(R.MAX_ITER), **rec)
            assert os.path.getsize(os.path.join(OUT, f"icp_{name}.npz")) <= 64 * 1024
    finally:
        ref_geo6d.nearest_neighbor = ref_nn


if __name__ == "__main__":
    if "icp" in sys.argv[1:]:
        gen_icp()
    which = sys.argv[1:] or ["matcher", "lift", "kabsch", "pointdsc", "e2e", "backbone", "metrics", "bop", "tokenizer", "data"]
    if "data" in which:
        gen_data()
    if "matcher" in which:
        gen_matcher()
    if "lift" in which:
        gen_lift()
    if "kabsch" in which:
        gen_kabsch()
    if "pointdsc" in which:
        gen_pointdsc()
    if "pointdsc_edge" in which:
        gen_pointdsc_edge()
    if "e2e" in which:
        gen_end_to_end()
    if "backbone" in which:
        gen_backbone()
    if "metrics" in which:
        gen_metrics()
    if "bop" in which:
        gen_bop_metrics()
    if "tokenizer" in which:
        gen_tokenizer()
    if "ransac" in which:
        gen_ransac()
    if "vsd" in which:
        gen_vsd()
    if "floss" in which:
        gen_feature_loss()
    if "floss_grad" in which:
        gen_feature_loss_grad()
    if "gt_corrs" in which:
        gen_gt_corrs()
