"""The ground-truth correspondence kernels (csrc/gt_corrs.hip) on the device against the numpy statement of their definition
(tests/gt_corrs_restatement.py): the nearest stage bit for bit, the whole routine row for row on synthetic pairs, the drop-in
`pairs.pcd_correspondences` against what the reference returned (tests/golden/gtcorr_*.npz), and the fixed-split builder read back
through datasets.FixedSplit and DeviceCollate."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import gt_corrs_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TILE = 1024                                        # GTC_TILE of csrc/gt_corrs.hip: query points per LDS tile
N_SRC = (1, 255, 256, 257, 1025)                   # around the 256-thread workgroup, more than one workgroup
N_DST = (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def clouds():
    """One source and one query cloud at the largest sizes (every case is a prefix) and the restatement's answers for every size pair."""
    rng = np.random.default_rng(21)
    src, dst = rng.normal(size=(max(N_SRC), 3)), rng.normal(size=(max(N_DST), 3))
    want = {(ns, nd): R.nearest(src[:ns], dst[:nd]) for ns in N_SRC for nd in N_DST}
    return src, dst, want


@pytest.mark.parametrize("nd", N_DST)
def test_pcd_nearest_equals_the_restatement(clouds, nd):
    """Every n_src of the list as one pair of a batch (different counts per pair), rows beyond n filled with NaN on both sides."""
    from oryon_amd import ops
    src, dst, want = clouds
    B, cap_s, cap_d = len(N_SRC), max(N_SRC) + 3, nd + 5
    S, D = np.full((B, cap_s, 3), np.nan), np.full((B, cap_d, 3), np.nan)
    for b, ns in enumerate(N_SRC):
        S[b, :ns], D[b, :nd] = src[:ns], dst[:nd]
    idx, d2 = ops.pcd_nearest(torch.from_numpy(S).cuda(), torch.from_numpy(D).cuda(), n_src=list(N_SRC), n_dst=[nd] * B)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    for b, ns in enumerate(N_SRC):
        wi, wd = want[(ns, nd)]
        assert np.array_equal(idx[b, :ns], wi), (ns, nd)
        assert np.array_equal(_bits(d2[b, :ns]), _bits(wd)), (ns, nd)


def test_pcd_nearest_batch_with_an_empty_pair_and_duplicates():
    """B = 3 with different counts on both sides, one pair with n = 0 on each side in turn, duplicated query points (the lowest index
    wins), NaN beyond n; counts as device tensors; untouched rows stay untouched."""
    from oryon_amd import ops
    rng = np.random.default_rng(22)
    n_src, n_dst = [300, 0, 77], [TILE + 9, 40, 0]
    cap_s, cap_d = 300, TILE + 9
    S, D = np.full((3, cap_s, 3), np.nan), np.full((3, cap_d, 3), np.nan)
    base = rng.normal(size=(200, 3))
    D[0, :n_dst[0]] = base[rng.integers(0, 200, n_dst[0])]              # ~5 copies of every point, spread over both tiles
    S[0, :300] = base[rng.integers(0, 200, 300)] + 1e-3 * rng.normal(size=(300, 3))
    D[1, :40] = rng.normal(size=(40, 3))
    S[2, :77] = rng.normal(size=(77, 3))
    ns = torch.tensor(n_src, dtype=torch.int32).cuda()
    nd = torch.tensor(n_dst, dtype=torch.int32).cuda()
    idx, d2 = ops.pcd_nearest(torch.from_numpy(S).cuda(), torch.from_numpy(D).cuda(), ns, nd)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    wi, wd = R.nearest(S[0, :300], D[0, :n_dst[0]])
    assert np.array_equal(idx[0], wi) and np.array_equal(_bits(d2[0]), _bits(wd))
    first = {tuple(p): j for j, p in reversed(list(enumerate(map(tuple, D[0, :n_dst[0]]))))}
    assert all(first[tuple(D[0, j])] == j for j in idx[0]), "a duplicated query point was not resolved to its lowest index"
    assert (idx[2, :77] == -1).all() and np.isinf(d2[2, :77]).all()          # no query point at all
    # an exact tie between two DIFFERENT points: the anchor halfway between them
    A = np.array([[[0.5, 0.0, 0.0]]])
    Q = np.array([[[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]])
    i2, dd = ops.pcd_nearest(torch.from_numpy(A).cuda(), torch.from_numpy(Q).cuda())
    assert int(i2[0, 0]) == 0 and float(dd[0, 0]) == 0.25


def _views(index, H, W, mask_id=1, zero_patches=False, far=False):
    """A synth.make_pair pair as two single views: depth [H,W] fp32 mm, instance masks with ids {0, mask_id, 9}, K, pose_aq [4,4]."""
    from oryon_amd.synth import make_pair
    p = make_pair(index, H, W, 1)
    da, dq = p["depth_a"].numpy().copy(), p["depth_q"].numpy().copy()
    ma, mq = p["mask_a"].numpy().astype(np.int32) * mask_id, p["mask_q"].numpy().astype(np.int32) * mask_id
    ma[0, :3][ma[0, :3] == 0] = 9                          # another instance id in the image
    mq[-1, -3:][mq[-1, -3:] == 0] = 9
    if zero_patches:                                       # sensor holes INSIDE the masks: kept, lifted to the origin
        da[H // 2:H // 2 + 3, W // 2:W // 2 + 4] = 0.0
        ys, xs = np.nonzero(mq == mask_id)
        dq[ys[len(ys) // 2], xs[len(xs) // 2]] = 0.0
        dq[ys[len(ys) // 3], xs[len(xs) // 3]] = 0.0
    T = p["pose"].numpy().copy()
    if far:
        T[:3, 3] += 0.5                                    # half a metre off: nothing is within any threshold used here
    return da, dq, ma, mq, p["camera"].numpy(), T


CASES = [  # (tag, H, W, pair indices (one batch), mask id, zero-depth patches, far)
    ("33x47", 33, 47, (3, 4), 1, False, False),
    ("64x80_mask7", 64, 80, (5, 6, 7), 7, False, False),
    ("96x96_holes", 96, 96, (8, 9), 1, True, False),
    ("64x80_far", 64, 80, (5,), 1, False, True),
]


@pytest.mark.parametrize("threshold", [0.002, 0.01])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gt_corrs_equals_the_restatement(case, threshold):
    from oryon_amd import ops
    tag, H, W, indices, mask_id, holes, far = case
    views = [_views(i, H, W, mask_id, holes, far) for i in indices]
    B = len(views)
    lists = [(R.pixel_list(v[2], mask_id), R.pixel_list(v[3], mask_id)) for v in views]
    cap_a, cap_q = max(len(a) for a, _ in lists) + 2, max(len(q) for _, q in lists) + 2
    pix_a, pix_q = np.full((B, cap_a), H * W + 11, np.int32), np.full((B, cap_q), -5, np.int32)          # never read beyond n
    for b, (a, q) in enumerate(lists):
        pix_a[b, :len(a)], pix_q[b, :len(q)] = a, q
    st = lambda k, dt: torch.from_numpy(np.stack([v[k] for v in views]).astype(dt)).cuda()
    out = ops.gt_corrs(st(0, np.float32), st(1, np.float32), torch.from_numpy(pix_a).cuda(), [len(a) for a, _ in lists],
                       torch.from_numpy(pix_q).cuda(), [len(q) for _, q in lists], st(4, np.float64), st(4, np.float64), st(5, np.float64),
                       threshold, want_nn=True)
    n_corr, corrs = out["n_corr"].cpu().numpy(), out["corrs"].cpu().numpy()
    idx, d2 = out["idx"].cpu().numpy(), out["d2"].cpu().numpy()
    total = 0
    for b, v in enumerate(views):
        a, q = lists[b]
        want = R.gt_corrs(v[0], v[1], a, q, v[4], v[4], v[5][:3], threshold)
        assert R.threshold_margin(want["d2"], threshold) >= 1e-9, "the case has a minimum ON the threshold: choose another pair"
        if holes:
            assert (v[0].reshape(-1)[a] == 0).sum() >= 12 and (v[1].reshape(-1)[q] == 0).sum() == 2
        assert np.array_equal(idx[b, :len(a)], want["idx"]) and np.array_equal(_bits(d2[b, :len(a)]), _bits(want["d2"])), (tag, b)
        assert int(n_corr[b]) == want["corrs"].shape[0], (tag, b, int(n_corr[b]), want["corrs"].shape[0])
        assert np.array_equal(corrs[b, :n_corr[b]], want["corrs"]), (tag, b)                            # rows AND their order
        total += int(n_corr[b])
    assert (total == 0) if far else (total > 0), (tag, total)


def test_gt_corrs_skips_pairs_with_a_status():
    from oryon_amd import ops
    H, W = 33, 47
    views = [_views(i, H, W) for i in (3, 4, 3)]
    lists = [(R.pixel_list(v[2], 1), R.pixel_list(v[3], 1)) for v in views]
    cap_a, cap_q = max(len(a) for a, _ in lists), max(len(q) for _, q in lists)
    pix_a, pix_q = np.zeros((3, cap_a), np.int32), np.zeros((3, cap_q), np.int32)
    for b, (a, q) in enumerate(lists):
        pix_a[b, :len(a)], pix_q[b, :len(q)] = a, q
    st = lambda k, dt: torch.from_numpy(np.stack([v[k] for v in views]).astype(dt)).cuda()
    status = torch.tensor([0, 2, 0], dtype=torch.int32).cuda()
    out = ops.gt_corrs(st(0, np.float32), st(1, np.float32), torch.from_numpy(pix_a).cuda(), [len(a) for a, _ in lists],
                       torch.from_numpy(pix_q).cuda(), [len(q) for _, q in lists], st(4, np.float64), st(4, np.float64), st(5, np.float64),
                       0.01, status=status)
    n = out["n_corr"].cpu().numpy()
    want = R.gt_corrs(views[0][0], views[0][1], *lists[0], views[0][4], views[0][4], views[0][5][:3], 0.01)["corrs"]
    assert n[1] == 0 and n[0] == n[2] == want.shape[0] > 0
    assert np.array_equal(out["corrs"][0, :n[0]].cpu().numpy(), want) and np.array_equal(out["corrs"][2, :n[2]].cpu().numpy(), want)


def test_lift_object_equals_the_restatement():
    from oryon_amd import pairs
    da, _, ma, _, K, _ = _views(5, 64, 80, mask_id=7, zero_patches=True)
    got = pairs.lift_object(da, ma, 7, K)
    xyz, yx = R.lift(da, R.pixel_list(ma, 7), K)
    assert np.array_equal(_bits(got["xyz"].numpy()), _bits(xyz)) and np.array_equal(got["yx_map"].numpy(), yx.astype(np.float64))
    assert pairs.lift_object(da, ma, 4, K)["xyz"].shape == (0, 3)


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_drop_in_returns_what_the_reference_returned(name):
    """pairs.pcd_correspondences through the device on the golden clouds: the reference's indices (kept set, order, both draws) and
    the generator left where the reference leaves it."""
    from oryon_amd import pairs
    g = np.load(os.path.join(GOLDEN, f"gtcorr_{name}.npz"))
    f1, f2 = R.golden_clouds(name)
    saved = torch.get_rng_state()
    try:
        torch.manual_seed(int(g["torch_seed"]))
        i1, i2 = pairs.pcd_correspondences(torch.from_numpy(f1), torch.from_numpy(f2), float(g["threshold"]), int(g["max_corrs"]))
        state = torch.get_rng_state().numpy()
    finally:
        torch.set_rng_state(saved)
    assert i1.device.type == "cpu" and i1.dtype == torch.int64
    assert np.array_equal(i1.numpy(), g["idx1"]) and np.array_equal(i2.numpy(), g["idx2"])
    assert np.array_equal(state, g["rng_state"])


# ------------------------------------------------------------------------------------------------------------------------ the builder
H_T, W_T, OBJ = 96, 96, 5
SCENES = {1: 11, 2: 12, 3: 13}                     # scene id -> synth pair index; image 0 is the anchor view, image 10 the query view


def _write_toyl_tree(base):
    """A TOYL-layout tree (the header of oryon_amd/datasets.py) of three scenes with two views each, from synth.make_pair: 16-bit depth
    in millimetres, instance masks (annotation 1 is another object without visible pixels, annotation 2 the object), scene_gt.json."""
    from PIL import Image
    views = {}
    P0 = np.eye(4)
    P0[:3, 3] = (0.01, -0.02, 0.8)                         # object-to-camera pose of the anchor view, metres
    for scene, index in SCENES.items():
        da, dq, ma, mq, K, T = _views(index, H_T, W_T)
        d = os.path.join(base, "split", "test", f"{scene:06d}")
        for sub in ("rgb", "mask_visib", "depth"):
            os.makedirs(os.path.join(d, sub))
        gts, infos = {}, {}
        for img, depth, mask, pose in ((0, da, ma, P0), (10, dq, mq, T @ P0)):
            depth16 = np.rint(depth).astype(np.uint16)
            mask8 = np.where(mask == 1, 2, 0).astype(np.uint8)
            Image.fromarray(depth16).save(os.path.join(d, "depth", f"{img:06d}.png"))
            Image.fromarray(mask8).save(os.path.join(d, "mask_visib", f"{img:06d}.png"))
            Image.fromarray(np.full((H_T, W_T, 3), 90 + img, np.uint8)).save(os.path.join(d, "rgb", f"{img:06d}.png"))
            t_mm = [float(x) for x in pose[:3, 3] * 1000.0]
            gts[str(img)] = [{"cam_R_m2c": [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], "cam_t_m2c": [0.0, 0.0, 500.0], "obj_id": 9},
                             {"cam_R_m2c": [float(x) for x in pose[:3, :3].reshape(-1)], "cam_t_m2c": t_mm, "obj_id": OBJ}]
            infos[str(img)] = [{"bbox_visib": [0, 0, 1, 1]}, {"bbox_visib": [0, 0, W_T, H_T]}]
            parsed = np.eye(4)
            parsed[:3, :3], parsed[:3, 3] = pose[:3, :3], np.asarray(t_mm) / 1000.0
            views[(scene, img)] = dict(depth=depth16.astype(np.float32), mask=mask8, pose=parsed, K=K)
        with open(os.path.join(d, "scene_gt.json"), "w") as f:
            json.dump(gts, f)
        with open(os.path.join(d, "scene_gt_info.json"), "w") as f:
            json.dump(infos, f)
    for name, obj in (("templates.json", ["a photo of a {}.", "there is a {} in the scene."]), ("object_splits.json", {"all": [OBJ, 9]}),
                      ("models_name.json", {str(OBJ): ["thing", "a small thing", "a red thing"], "9": ["other", "x", "y"]})):
        with open(os.path.join(base, name), "w") as f:
            json.dump(obj, f)
    return views


def test_make_fixed_split_writes_what_fixed_split_reads(tmp_path):
    from oryon_amd import pairs
    from oryon_amd.data import DeviceCollate
    from oryon_amd.datasets import FixedSplit
    base = str(tmp_path / "toyl")
    views = _write_toyl_tree(base)
    K = next(iter(views.values()))["K"]
    threshold, min_corrs = 0.004, 20
    torch.manual_seed(77)
    before = torch.get_rng_state()
    n = pairs.make_fixed_split("toyl", base, "test", "mine", 3, seed=4, threshold=threshold, min_corrs=min_corrs, max_fail=200, camera=K)
    assert n == 3 and torch.equal(torch.get_rng_state(), before)               # the global generator is the caller's
    dest = os.path.join(base, "fixed_split", "mine")
    files = {f: open(os.path.join(dest, f), "rb").read() for f in ("instance_list.txt", "annots.pkl")}
    lines = files["instance_list.txt"].decode().splitlines()
    assert sorted(lines) == [f"test, {s} 0, {s} 10, {OBJ}" for s in sorted(SCENES)]
    annots = pickle.loads(files["annots.pkl"])
    split = FixedSplit("toyl", str(tmp_path), "toyl", "mine")
    assert len(split) == 3
    items = [split[i] for i in range(3)]
    for i, line in enumerate(lines):
        scene = int(line.split(",")[1].split()[0])
        a, q = views[(scene, 0)], views[(scene, 10)]
        pose_aq = q["pose"] @ np.linalg.inv(a["pose"])
        want = R.gt_corrs(a["depth"], q["depth"], R.pixel_list(a["mask"], 2), R.pixel_list(q["mask"], 2), K, K, pose_aq[:3], threshold)
        assert R.threshold_margin(want["d2"], threshold) >= 1e-9
        rec = annots[f"{scene}_0_{scene}_10_{OBJ}"]
        assert rec["corrs"].dtype == np.float64 and rec["corrs"].shape[0] >= min_corrs
        assert np.array_equal(rec["corrs"], want["corrs"].astype(np.float64))
        gt_mm = pose_aq.copy()
        gt_mm[:3, 3] = gt_mm[:3, 3] * 1000.0
        assert np.array_equal(rec["gt"], gt_mm)
        item_a, item_q, prompt, sampled, corrs, pose, cls_id, instance_id, valid = items[i]
        assert valid and cls_id == OBJ and np.array_equal(corrs.numpy(), rec["corrs"]) and sampled.shape == (split.max_corrs, 4)
        assert np.allclose(pose[:3, 3] * 1000.0, gt_mm[:3, 3], rtol=0, atol=1e-9) and np.array_equal(pose[:3, :3], gt_mm[:3, :3])
    batch = DeviceCollate(split.max_corrs, (48, 48))(items)
    assert batch["valid"].tolist() == [1.0, 1.0, 1.0] and tuple(batch["corrs"].shape) == (3, split.max_corrs, 4)
    assert all(np.array_equal(batch["all_corrs"][i].numpy(), items[i][4].numpy()) for i in range(3))
    # the same seed writes the same files
    assert pairs.make_fixed_split("toyl", base, "test", "again", 3, seed=4, threshold=threshold, min_corrs=min_corrs, max_fail=200, camera=K) == 3
    for f, blob in files.items():
        assert open(os.path.join(base, "fixed_split", "again", f), "rb").read() == blob, f


def _write_nocs_tree(base):
    """A NOCS-layout tree of two scenes with two views each: `<img>_{color,mask,depth}.png`, `_meta.txt`, `_detection.txt`, the gts
    pickles with SCALED rotations (as NOCS stores them; the scale cancels in pose_q @ inv(pose_a)) and split/real_test/instance_list.txt."""
    from PIL import Image
    views, listed = {}, []
    P0 = np.eye(4)
    P0[:3, :3] *= 0.3
    P0[:3, 3] = (0.02, 0.01, 0.7)
    for scene, index in ((1, 11), (2, 12)):
        da, dq, ma, mq, K, T = _views(index, H_T, W_T)
        d = os.path.join(base, "split", "real_test", f"scene_{scene}")
        os.makedirs(d)
        os.makedirs(os.path.join(base, "gts", "real_test"), exist_ok=True)
        for img, depth, mask, pose in ((0, da, ma, P0), (10, dq, mq, T @ P0)):
            depth16, mask8 = np.rint(depth).astype(np.uint16), np.where(mask == 1, 2, 255).astype(np.uint8)
            stem = os.path.join(d, f"{img:04d}")
            Image.fromarray(depth16).save(stem + "_depth.png")
            Image.fromarray(mask8).save(stem + "_mask.png")
            Image.fromarray(np.full((H_T, W_T, 3), 60 + img, np.uint8)).save(stem + "_color.png")
            with open(stem + "_meta.txt", "w") as f:
                f.write("1 4 other_b\n2 3 thing_a\n")
            with open(stem + "_detection.txt", "w") as f:
                f.write("4 0 0 1 1\n3 0 0 %d %d\n" % (H_T, W_T))
            with open(os.path.join(base, "gts", "real_test", f"results_real_test_scene_{scene}_{img:04d}.pkl"), "wb") as f:
                pickle.dump({"gt_RTs": np.stack([np.eye(4), pose])}, f)
            views[(scene, img)] = dict(depth=depth16.astype(np.float32), mask=mask8, pose=pose, K=K)
            listed.append(f"{scene} {img}\n")
    with open(os.path.join(base, "split", "real_test", "instance_list.txt"), "w") as f:
        f.writelines(listed)
    for name, obj in (("templates.json", ["a photo of a {}."]), ("object_splits.json", {"all": [3, 4]}),
                      ("obj_names.json", {"thing_a": ["thing", "a small thing", "a red thing"], "other_b": ["other", "x", "y"]})):
        with open(os.path.join(base, name), "w") as f:
            json.dump(obj, f)
    return views


def test_make_fixed_split_nocs_layout(tmp_path):
    """The NOCS reader of the builder: rows from `_meta.txt`, poses from the gts pickles as stored (scaled rotations), both directions
    of a view pair (no frame-distance rule on NOCS), the `<cat> <name>` instance line and annotation key FixedSplit parses."""
    from oryon_amd import pairs
    from oryon_amd.datasets import FixedSplit
    base = str(tmp_path / "nocs")
    views = _write_nocs_tree(base)
    K = next(iter(views.values()))["K"]
    threshold = 0.004
    assert pairs.make_fixed_split("nocs", base, "real_test", "mine", 3, seed=2, threshold=threshold, min_corrs=20, max_fail=200, camera=K) == 3
    dest = os.path.join(base, "fixed_split", "mine")
    lines = open(os.path.join(dest, "instance_list.txt")).read().splitlines()
    annots = pickle.load(open(os.path.join(dest, "annots.pkl"), "rb"))
    assert len(lines) == len(set(lines)) == 3 == len(annots)
    for line in lines:
        part, ida, idq, cat = [t.strip() for t in line.split(",")]
        (sa, ia), (sq, iq) = (int(x) for x in ida.split()), (int(x) for x in idq.split())
        assert part == "real_test" and cat == "3 thing_a" and sa == sq and {ia, iq} == {0, 10}
        a, q = views[(sa, ia)], views[(sq, iq)]
        pose_aq = q["pose"] @ np.linalg.inv(a["pose"])
        want = R.gt_corrs(a["depth"], q["depth"], R.pixel_list(a["mask"], 2), R.pixel_list(q["mask"], 2), K, K, pose_aq[:3], threshold)
        assert R.threshold_margin(want["d2"], threshold) >= 1e-9
        rec = annots[f"{sa}_{ia}_{sq}_{iq}_3_thing_a"]
        assert want["corrs"].shape[0] >= 20 and np.array_equal(rec["corrs"], want["corrs"].astype(np.float64))
        gt_mm = pose_aq.copy()
        gt_mm[:3, 3] = gt_mm[:3, 3] * 1000.0
        assert np.array_equal(rec["gt"], gt_mm)
    split = FixedSplit("nocs", str(tmp_path), "nocs", "mine")
    assert len(split) == 3 and all(split[i][8] for i in range(3))


def test_make_split_driver_on_the_fabricated_tree(tmp_path, capsys):
    """`python make_split.py` end to end (in process).  The driver has the dataset's published camera, which does not fit the synthetic
    views, so it is run with --min-corrs 0: every drawn pair is written whatever it keeps, and FixedSplit reads the result."""
    import make_split
    from oryon_amd.datasets import FixedSplit
    base = str(tmp_path / "toyl")
    _write_toyl_tree(base)
    summary = make_split.main(["--kind", "toyl", "--data-root", base, "--dest-split", "drv", "--pairs", "2", "--seed", "3", "--min-corrs", "0"])
    assert summary["pairs_written"] == 2 and json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == summary
    split = FixedSplit("toyl", str(tmp_path), "toyl", "drv")
    assert len(split) == 2 and all(c.ndim == 2 and c.shape[1] == 4 and c.dtype == np.float64 for c in split.corrs)
    assert [i[:4] for i in split.instances] == [(int(l.split(",")[1].split()[0]), 0, int(l.split(",")[1].split()[0]), 10)
                                                for l in open(os.path.join(base, "fixed_split", "drv", "instance_list.txt"))]
