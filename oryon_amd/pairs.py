"""Ground-truth correspondences of RGB-D pairs with known poses, and the builder of fixed splits that stores them.

Restated from the reference's data-preparation scripts (scripts/data/make_toyl_test.py, make_nocs_test.py: pcd_correspondences :47-85
and the pair loop :87-252) with the all-pairs nearest-neighbour search on the device (ops.pcd_nearest / ops.gt_corrs, csrc/gt_corrs.hip;
definition in include/oryon_hip.h, oryon_gt_corrs) instead of a 20 000 x 20 000 float64 torch.cdist on the host.  What it writes is the
`fixed_split/<split>/{instance_list.txt, annots.pkl}` pair that datasets.FixedSplit reads (format: the header of datasets.py).

The draws that cap a side at 20 000 points and the kept rows at max_corrs are the reference's own calls in the reference's order
(torch.multinomial over a float64 vector of ones, without replacement, from the global CPU generator: anchors, queries, kept rows), so a
seeded call returns the reference's rows and leaves the generator where the reference leaves it.  The PAIR selection of
make_fixed_split draws from its own seeded numpy generator: row-for-row equality with a split the reference would draw (it uses the
global numpy state, unseeded) is not claimed.
"""
from __future__ import annotations

import json
import os
import pickle
from os.path import join
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .datasets import NOCS_K, TOYL_K, _png

SAMPLE = 20000                    # make_toyl_test.py:53: points per side the distance matrix is built on


def _device(device=None) -> torch.device:
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _draw(n: int, k: int) -> torch.Tensor:
    """The reference's draw (make_toyl_test.py:57-58): k of n without replacement, uniform, global CPU generator."""
    return torch.multinomial(torch.ones(n, dtype=float), k, replacement=False)


def pcd_correspondences(feats1: torch.Tensor, feats2: torch.Tensor, threshold: float, max_corrs: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Drop-in for the reference's pcd_correspondences (make_toyl_test.py:47-85): feats1 [n1,3], feats2 [n2,3] point clouds -> two CPU
    int64 index tensors (rows of feats1 within `threshold` of their nearest row of feats2, and that row).  The distance matrix is never
    built: the device returns each row's first minimiser and its squared distance in float64.  An empty cloud gives two empty tensors
    (the reference raises on the empty reduction)."""
    n1, n2 = feats1.shape[0], feats2.shape[0]
    idxs1, idxs2 = torch.arange(0, n1), torch.arange(0, n2)
    if n1 >= SAMPLE:
        idxs1 = idxs1[_draw(n1, SAMPLE)]
        feats1 = feats1[idxs1.to(feats1.device)]
    if n2 >= SAMPLE:
        idxs2 = idxs2[_draw(n2, SAMPLE)]
        feats2 = feats2[idxs2.to(feats2.device)]
    if feats1.shape[0] == 0 or feats2.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    idx, d2 = ops.pcd_nearest(feats1[:, :3].double(), feats2[:, :3].double())
    idx, d2 = idx[0].cpu().to(torch.int64), d2[0].cpu()
    valid = torch.nonzero(torch.sqrt(d2) <= threshold).squeeze(1)
    idxs1, idxs2 = idxs1[valid], idxs2[idx[valid]]
    if valid.shape[0] > max_corrs:
        chosen = _draw(valid.shape[0], max_corrs)
        idxs1, idxs2 = idxs1[chosen], idxs2[chosen]
    return idxs1, idxs2


def _pixel_list(mask, mask_idx: int, dev: torch.device) -> Tuple[torch.Tensor, int]:
    """Row-major linear pixels where mask == mask_idx, as a [1, max(n, 1)] int32 device list through the reference's 20 000-point draw."""
    m = (torch.as_tensor(np.array(mask)).to(dev) == int(mask_idx)).to(torch.int32)           # a copy: PIL hands out read-only buffers
    roi, count = ops.roi_compact(m[None])
    n = int(count[0])
    pix = roi[0, :n]
    if n >= SAMPLE:
        pix = pix[_draw(n, SAMPLE).to(dev)]
        n = SAMPLE
    if n == 0:
        pix = torch.zeros(1, dtype=torch.int32, device=dev)
    return pix[None].contiguous(), n


def _depth32(depth, dev: torch.device) -> torch.Tensor:
    return torch.as_tensor(np.asarray(depth).astype(np.float32)).to(dev)[None].contiguous()


def lift_object(depth, mask, mask_idx: int, K, device=None) -> Dict[str, torch.Tensor]:
    """toyl.get_pcd + filter_pcd (utils/data/toyl.py:237-278; nocs alike) for one object: depth [H,W] millimetres, mask [H,W] instance
    ids, K [3,3] -> {'xyz' [n,3] float64 metres, 'yx_map' [n,2] float64 (y, x)} on the CPU, rows in row-major pixel order.  No
    20 000-point draw here: the reference makes it inside pcd_correspondences."""
    dev = _device(device)
    m = (torch.as_tensor(np.array(mask)).to(dev) == int(mask_idx)).to(torch.int32)           # a copy: PIL hands out read-only buffers
    roi, count = ops.roi_compact(m[None])
    n = int(count[0])
    if n == 0:
        return {"xyz": torch.zeros((0, 3), dtype=torch.float64), "yx_map": torch.zeros((0, 2), dtype=torch.float64)}
    cam = torch.as_tensor(np.asarray(K, dtype=np.float64)).reshape(1, 9)
    xyz, yx = ops.gtc_lift(_depth32(depth, dev), roi[:, :n].contiguous(), [n], cam)
    return {"xyz": xyz[0].cpu(), "yx_map": yx[0].cpu().to(torch.float64)}


def relative_pose(pose_a, pose_q) -> np.ndarray:
    """pose_q @ inv(pose_a) in numpy float64 (make_toyl_test.py:212): maps anchor-camera points to query-camera points, metres."""
    return np.asarray(pose_q, dtype=np.float64) @ np.linalg.inv(np.asarray(pose_a, dtype=np.float64))


def _mask_idx(item: dict, mask_idx: Optional[int]) -> int:
    return int(item["metadata"]["mask_ids"][0]) if mask_idx is None else int(mask_idx)


def pair_correspondences(item_a: dict, item_q: dict, pose_a, pose_q, mask_idx_a: Optional[int] = None, mask_idx_q: Optional[int] = None,
                         threshold: float = 0.002, max_corrs: int = 10000, device=None) -> Tuple[np.ndarray, np.ndarray]:
    """The correspondences the reference stores for one pair (make_toyl_test.py:175-243).  item_*: dicts with 'depth' [H,W]
    millimetres, 'mask' [H,W] instance ids and 'camera' [3,3] (datasets.FixedSplit.get_item's, before preprocess_item); pose_* [4,4]
    object-to-camera, metres; mask_idx_* default to the item's metadata['mask_ids'][0].
    -> (rows [n,4] float64 (y_a, x_a, y_q, x_q), pose_aq [4,4] float64 with the translation in MILLIMETRES, as annots.pkl stores both)."""
    dev = _device(device)
    pose_aq = relative_pose(pose_a, pose_q)
    stored = pose_aq.copy()
    stored[:3, 3] = stored[:3, 3] * 1000.0
    pix_a, n_a = _pixel_list(item_a["mask"], _mask_idx(item_a, mask_idx_a), dev)     # the anchor side draws first, as the reference does
    pix_q, n_q = _pixel_list(item_q["mask"], _mask_idx(item_q, mask_idx_q), dev)
    if n_a == 0 or n_q == 0:
        return np.zeros((0, 4), dtype=np.float64), stored
    cam_a = torch.as_tensor(np.asarray(item_a["camera"], dtype=np.float64)).reshape(1, 9)
    cam_q = torch.as_tensor(np.asarray(item_q["camera"], dtype=np.float64)).reshape(1, 9)
    out = ops.gt_corrs(_depth32(item_a["depth"], dev), _depth32(item_q["depth"], dev), pix_a, [n_a], pix_q, [n_q], cam_a, cam_q,
                       torch.as_tensor(pose_aq[None]), threshold)
    n = int(out["n_corr"][0])
    rows = out["corrs"][0, :n].cpu()
    if n > max_corrs:
        rows = rows[_draw(n, max_corrs)]
    return rows.numpy().astype(np.float64), stored


# ---------------------------------------------------------------------------------------------------- the instance tables of a source split
def _toyl_instances(base: str, src_split: str) -> List[dict]:
    """utils/data/toyl.py:91-136 get_part_data, flattened as make_toyl_test.py:101-111 does: one row per (image, object id).  The
    per-image dict is keyed by the object id, so of several annotations of one object the LAST wins; masks are numbered by annotation order."""
    rows = []
    split_dir = join(base, "split", src_split)
    for folder in sorted(os.listdir(split_dir)):
        if not os.path.isfile(join(split_dir, folder, "scene_gt.json")):
            continue
        with open(join(split_dir, folder, "scene_gt.json")) as f:
            gts = json.load(f)
        for img_k, objs in gts.items():
            per_cls = {}
            for i, g in enumerate(objs):
                pose = np.eye(4)
                pose[:3, :3] = np.asarray(g["cam_R_m2c"], dtype=np.float64).reshape(3, 3)
                pose[:3, 3] = np.asarray(g["cam_t_m2c"], dtype=np.float64) / 1000.0
                per_cls[int(g["obj_id"])] = dict(scene=int(folder), image=int(img_k), obj=int(g["obj_id"]), key=int(g["obj_id"]), mask_idx=i + 1,
                                                 pose=pose, name=None)
            rows += list(per_cls.values())
    return rows


def _nocs_instances(base: str, src_split: str) -> List[dict]:
    """make_nocs_test.py:99-120: one row per line of every listed image's _meta.txt ("<mask_id> <cat_id> <obj_name>"); two rows show
    the same object when their names agree.  Poses are the stored gt_RTs rows as they are (scaled rotations: the scale cancels in
    pose_q @ inv(pose_a) for one object)."""
    rows = []
    with open(join(base, "split", src_split, "instance_list.txt")) as f:
        listed = [line.split() for line in f if line.strip()]
    for scene_id, img_id in listed:
        scene, img = int(scene_id), int(img_id)
        with open(join(base, "gts", src_split, f"results_{src_split}_scene_{scene}_{img:04d}.pkl"), "rb") as f:
            rts = np.asarray(pickle.load(f)["gt_RTs"], dtype=np.float64)
        with open(join(base, "split", src_split, f"scene_{scene}", f"{img:04d}_meta.txt")) as f:
            for line in f:
                if not line.strip():
                    continue
                mask_idx, cat_id, name = line.split()
                rows.append(dict(scene=scene, image=img, obj=int(cat_id), key=name, mask_idx=int(mask_idx), pose=rts[int(mask_idx) - 1].copy(),
                                 name=name))
    return rows


def _load_view(kind: str, base: str, src_split: str, row: dict, camera) -> dict:
    if kind == "toyl":
        d = join(base, "split", src_split, f"{row['scene']:06d}")
        return {"depth": _png(join(d, "depth", f"{row['image']:06d}.png"), None), "mask": _png(join(d, "mask_visib", f"{row['image']:06d}.png"), "L"),
                "camera": TOYL_K if camera is None else camera}
    stem = join(base, "split", src_split, f"scene_{row['scene']}", f"{row['image']:04d}")
    return {"depth": _png(stem + "_depth.png", None), "mask": _png(stem + "_mask.png", "L"), "camera": NOCS_K if camera is None else camera}


def make_fixed_split(kind: str, root: str, src_split: str, dest_split: str, n_elems: int, seed: int, threshold: float = 0.002,
                     max_corrs: int = 10000, min_corrs: int = 100, max_fail: int = 200000, device=None, log=None, camera=None) -> int:
    """Draw `n_elems` view pairs of `<root>/split/<src_split>` and write `<root>/fixed_split/<dest_split>/{instance_list.txt, annots.pkl}`
    (make_toyl_test.py:87-252 / make_nocs_test.py with scene_type 'same').  root is the dataset's own directory (`<dataset.root>/<name>`
    of FixedSplit).  camera: [3,3] intrinsics of the source images (None = the dataset's published camera, datasets.NOCS_K / TOYL_K).
    Returns the number of pairs written.

    The reference's rules: anchor instance uniform over all (image, object) rows; query uniform over the rows of the same object in the
    same scene; the same row twice, a pair already chosen or fewer than `min_corrs` correspondences count as failures, and `max_fail`
    failures end the run early.  The draws come from numpy.random.default_rng(seed) and the correspondence draws from a torch
    generator state seeded with `seed` (restored afterwards), so one seed writes the same files every time; equality with a split the
    reference's unseeded run would draw is not claimed.  A draw that fails no rule but is skipped without being counted (below) is
    bounded by 10 * max_fail + n_elems draws in all - the reference would loop forever on a tree where every draw is such a skip."""
    if kind not in ("nocs", "toyl"):
        raise ValueError(f"unknown dataset kind {kind!r}")
    say = log if log is not None else (lambda *a: None)
    rows = _toyl_instances(root, src_split) if kind == "toyl" else _nocs_instances(root, src_split)
    if not rows:
        raise ValueError(f"{join(root, 'split', src_split)}: no annotated object instance found")
    scenes = np.asarray([r["scene"] for r in rows])
    keys = np.asarray([r["key"] for r in rows])
    rng = np.random.default_rng(seed)
    lines, gt_dict, chosen = [], {}, set()
    i = fail_i = draws = 0
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        while i < n_elems and fail_i < max_fail and draws < 10 * max_fail + n_elems:
            draws += 1
            idx_a = int(rng.integers(0, len(rows)))
            a = rows[idx_a]
            pool = np.nonzero(np.logical_and(keys == a["key"], scenes == a["scene"]))[0]      # never empty: it holds idx_a
            idx_q = int(rng.choice(pool))
            if idx_a == idx_q:
                fail_i += 1
                continue
            q = rows[idx_q]
            # make_toyl_test.py:157 reads `abs(int(image_q)-int(image_a) < 10)`: the parenthesis closes after the comparison, so this is
            # abs(True / False) and the pair is skipped whenever image_q - image_a < 10, i.e. only pairs whose query frame lies at least
            # ten ids AFTER the anchor's survive.  Kept as written (the published splits were drawn this way), and not a counted failure.
            if kind == "toyl" and abs(int(q["image"]) - int(a["image"]) < 10):
                continue
            total = (a["scene"], a["image"], q["scene"], q["image"], a["obj"])
            if total in chosen:
                fail_i += 1
                continue
            item_a, item_q = _load_view(kind, root, src_split, a, camera), _load_view(kind, root, src_split, q, camera)
            if not (np.asarray(item_a["mask"]) == a["mask_idx"]).any() or not (np.asarray(item_q["mask"]) == q["mask_idx"]).any():
                say(f"empty mask: {a['scene']} {a['image']} / {q['scene']} {q['image']} object {a['obj']}")
                continue
            corrs, pose_aq = pair_correspondences(item_a, item_q, a["pose"], q["pose"], a["mask_idx"], q["mask_idx"], threshold, max_corrs, device)
            if corrs.shape[0] < min_corrs:
                say(f"not enough corrs: {corrs.shape[0]}")
                fail_i += 1
                continue
            ids = [a["scene"], a["image"], q["scene"], q["image"], a["obj"]]
            if kind == "nocs":
                lines.append("{}, {} {}, {} {}, {} {}\n".format(src_split, *ids, a["name"]))
                ids.append(a["name"])
            else:
                lines.append("{}, {} {}, {} {}, {}\n".format(src_split, *ids))
            gt_dict["_".join(str(e) for e in ids)] = {"gt": pose_aq, "corrs": corrs}
            chosen.add(total)
            i += 1
    if i < n_elems:
        say(f"stopped at {i} of {n_elems} pairs after {fail_i} failures and {draws} draws")
    dest = join(root, "fixed_split", dest_split)
    os.makedirs(dest, exist_ok=True)
    with open(join(dest, "instance_list.txt"), "w") as f:
        f.writelines(lines)
    with open(join(dest, "annots.pkl"), "wb") as f:
        pickle.dump(gt_dict, f)
    return i
