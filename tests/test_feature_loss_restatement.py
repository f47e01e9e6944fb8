"""CPU tests of the validation step's ground truth and plumbing: the float64 restatement (tests/feature_loss_restatement.py) reproduces
what the reference's FeatureLoss.forward recorded (tests/golden/floss_*.npz, written by tools/gen_goldens.py gen_feature_loss from
losses.py:64-220), compute_fmr and the evaluator's validation registrations agree with the reference's values / the test registrations,
pair_gt_corrs agrees with make_pair, and the new C-ABI symbols exist on every layer.

Bars (ISSUE "Bars"): negative indices equal on EVERY row; distances, per-pair terms, batch losses and the dice loss within 1e-6 of the
reference's fp32 values (4x the largest fp32-vs-float64 difference of the reference on these shapes)."""
import glob
import os

import numpy as np
import pytest
import torch

import feature_loss_restatement as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "floss_*.npz")))
NAMES = [os.path.basename(f)[len("floss_"):-len(".npz")] for f in FIXTURES]
BAR = 1e-6


def load(path):
    z = np.load(path)
    f = {k: z[k] for k in z.files}
    f["feat_a"], f["feat_q"] = f["feat_a"].astype(np.float32), f["feat_q"].astype(np.float32)
    f["logits_a"], f["logits_q"] = f["logits_a"].astype(np.float32), f["logits_q"].astype(np.float32)
    f["pool"] = f["pool"].astype(np.int64) if f["pool"].size else None
    f["image_hw"] = tuple(int(v) for v in f["image_hw"])
    return f


def test_all_seven_fixtures_are_present():
    assert NAMES == ["1_rescale", "2_nonsquare", "3_pool", "4_c256", "5_disc", "6_zero_dup_border", "7_none_valid"]
    for p in FIXTURES:
        assert os.path.getsize(p) < (1 << 20)


def test_fixtures_pin_what_they_are_for():
    f = {n: load(p) for n, p in zip(NAMES, FIXTURES)}
    assert f["1_rescale"]["valid"].tolist() == [1.0, 0.0, 1.0] and f["1_rescale"]["feat_a"].shape == (3, 32, 40, 40)
    assert f["2_nonsquare"]["feat_a"].shape == (2, 20, 40, 44) and f["2_nonsquare"]["corrs"].shape == (2, 37, 4)
    pix = fr.feature_pixels(f["2_nonsquare"]["corrs"], (48, 48), (40, 44))
    scaled_x = np.trunc(f["2_nonsquare"]["corrs"][..., 1].astype(np.float32) * np.float32(44 / 48))
    assert (scaled_x > 39).any() and pix[..., 1].max() == 39              # x reached past FH - 1 and was clamped by FH
    assert f["3_pool"]["pool"].shape == (2, 2, 2000) and f["3_pool"]["corrs"].shape[1] == 500
    assert all(len(set(r.tolist())) == 2000 for r in f["3_pool"]["pool"].reshape(-1, 2000))
    assert f["4_c256"]["feat_a"].shape == (1, 256, 16, 16)
    assert f["7_none_valid"]["valid"].tolist() == [0.0, 0.0]
    assert f["7_none_valid"]["loss_pos"] == 0 and f["7_none_valid"]["loss_neg"] == 0 and f["7_none_valid"]["loss_mask"] > 0
    for n in NAMES:
        ok = ~f[n]["gap_exempt"] & np.isfinite(f[n]["gap"])
        if f[n]["has_gap"]:
            assert (f[n]["gap"][ok] >= 1e-5).all(), n
    # 5: some positive has its whole pool inside the disc, and its reference negative is a penalised pixel
    yx = fr.feature_pixels(f["5_disc"]["corrs"], (6, 6), (6, 6))[0]
    inside = [all(np.hypot(y - cy, x - cx) < 5 for cy in range(6) for cx in range(6)) for y, x in yx[:, :2]]
    assert any(inside)
    # 6: exactly one exempt row, the zero positive; duplicates and the four corners are there
    g = f["6_zero_dup_border"]
    assert g["gap_exempt"].sum() == 1 and g["gap_exempt"][0, 0, 4] and not g["feat_a"][0][:, 12, 12].any()
    assert np.array_equal(g["corrs"][:, 0], g["corrs"][:, 1]) and g["corrs"][0, 2].tolist() == [0, 0, 23, 23]


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_restatement_reproduces_the_reference(path):
    f = load(path)
    FW = f["feat_a"].shape[3]
    r = fr.restate(f["feat_a"], f["feat_q"], f["corrs"], f["valid"], f["image_hw"], f["pool"])
    want_idx = np.stack([f["neg_a"], f["neg_q"]], axis=1)                  # [B,2,N,2] (y,x), zero rows for invalid pairs
    got_idx = np.stack([r["neg_idx"] // FW, r["neg_idx"] % FW], axis=-1)
    assert np.array_equal(got_idx, want_idx), f"{int((got_idx != want_idx).any(-1).sum())} rows differ"
    d = {"d_pos": np.abs(r["d_pos"] - f["d_pos"]).max(), "d_neg_a": np.abs(r["d_neg"][:, 0] - f["d_neg_a"]).max(),
         "d_neg_q": np.abs(r["d_neg"][:, 1] - f["d_neg_q"]).max(), "pos": abs(r["losses"][0] - f["loss_pos"]),
         "neg": abs(0.5 * (r["losses"][1] + r["losses"][2]) - f["loss_neg"])}
    la, mask_a, iou_a = fr.mask_terms(f["logits_a"], f["gt_a"], 0.5)
    lq, mask_q, iou_q = fr.mask_terms(f["logits_q"], f["gt_q"], 0.5)
    d["mask"] = abs(0.5 * (la + lq) - f["loss_mask"])
    print(os.path.basename(path), {k: f"{v:.2e}" for k, v in d.items()})
    assert max(d.values()) <= BAR, d
    assert np.array_equal(mask_a, f["mask_a"]) and np.array_equal(mask_q, f["mask_q"])
    assert np.allclose(iou_a, f["iou_a"], rtol=1e-6, equal_nan=True) and np.allclose(iou_q, f["iou_q"], rtol=1e-6, equal_nan=True)
    if not f["valid"].any():
        assert not r["losses"].any() and not r["pair_terms"].any()


def test_restatement_random_negatives_mode():
    """loss.hard_negatives = False: the drawn pixel is the negative; the distance is the plain cosine distance to it."""
    f = load(FIXTURES[NAMES.index("1_rescale")])
    rng = np.random.default_rng(0)
    pool = rng.integers(0, 1600, (3, 2, 64))
    r = fr.restate(f["feat_a"], f["feat_q"], f["corrs"], f["valid"], f["image_hw"], pool, per_positive=True)
    assert np.array_equal(r["neg_idx"][0], pool[0]) and not r["neg_idx"][1].any() and not r["d_neg"][1].any()
    pix = r["pix"]
    a = torch.from_numpy(f["feat_a"][0][:, pix[0, :, 0], pix[0, :, 1]].T).double()
    n = torch.from_numpy(f["feat_a"][0].reshape(32, -1)[:, pool[0, 0]].T).double()
    want = 0.5 * (1 - torch.nn.functional.cosine_similarity(a, n, dim=1))
    assert np.abs(r["d_neg"][0, 0] - want.numpy()).max() < 1e-12


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_compute_fmr_matches_the_reference(path):
    from oryon_amd import evaluation as ev
    f = load(path)
    pix = fr.feature_pixels(f["corrs"], f["image_hw"], f["feat_a"].shape[2:])
    B = len(pix)
    pos_a = np.stack([f["feat_a"][b][:, pix[b, :, 0], pix[b, :, 1]].T * (f["valid"][b] == 1) for b in range(B)])
    pos_q = np.stack([f["feat_q"][b][:, pix[b, :, 2], pix[b, :, 3]].T * (f["valid"][b] == 1) for b in range(B)])
    got = ev.compute_fmr(torch.from_numpy(pos_a), torch.from_numpy(pos_q), 0.25, 0.05)
    assert np.array_equal(got, f["fmr"])
    assert np.array_equal(ev.compute_fmr(pos_a[0], pos_q[0], 0.25, 0.05), f["fmr"][:1])          # the unbatched form
    valid = f["valid"] == 1
    if valid.any():                                                        # from the distances directly (what FeatureLoss returns)
        assert np.array_equal(ev.fmr_from_distances(f["d_pos"][valid], 0.25, 0.05), f["fmr"][valid])
    assert ev.fmr_from_distances(np.array([0.1, 0.3, 0.3, 0.3]), 0.25, 0.2).tolist() == [1.0]
    assert ev.fmr_from_distances(np.array([0.1, 0.3, 0.3, 0.3]), 0.25, 0.25).tolist() == [0.0]


def test_evaluator_validation_registrations_match_the_test_ones():
    from oryon_amd.evaluation import Evaluator
    rng = np.random.default_rng(3)
    rows = [dict(pred_pose_rel=np.eye(4) if i == 2 else rng.normal(size=(4, 4)), rot_deg=float(rng.uniform(0, 20)),
                 trans_cm=float(rng.uniform(0, 25)), add_s=float(rng.uniform(0, 0.05)), add_diam=0.2, mssd_mm=float(rng.uniform(0, 60)),
                 mspd_px=float(rng.uniform(0, 40)), bop_diam_mm=200.0, iou_a=float(rng.uniform()), iou_q=float(rng.uniform()),
                 vsd_errs=rng.uniform(0, 1, 10)) for i in range(5)]
    for vsd in (False, True):
        t, v = Evaluator(compute_vsd=vsd), Evaluator(compute_vsd=vsd)
        v.init_validation()
        assert "cls_id" not in v.metrics and "instance_id" not in v.metrics
        assert [k for k in t.metrics if k not in ("cls_id", "instance_id")] == list(v.metrics) and list(t.counts) == list(v.counts)
        for i, row in enumerate(rows):
            if i == 3:
                t.register_test_failure(cls_id=1, instance_id="x", iou_a=row["iou_a"], iou_q=row["iou_q"])
                v.register_valid_failure(iou_a=row["iou_a"], iou_q=row["iou_q"])
            else:
                t.register_test(cls_id=1, instance_id=f"p{i}", **row)
                v.register_eval(**row)
        for k in v.metrics:
            assert v.metrics[k] == t.metrics[k] and len(v.metrics[k]) == 5, k
        assert v.counts == t.counts and v.counts["Missing segm"] == [0, 0, 0, 1, 0] and v.counts["Failed pose"][2] == 1
        assert t.metrics["cls_id"] == [1] * 5 and t.metrics["instance_id"] == ["p0", "p1", "p2", "x", "p4"]
        assert v.get_means() == t.get_means()


def test_pair_gt_corrs_agrees_with_make_pair():
    from oryon_amd.synth import make_pair, pair_gt_corrs
    H = W = 48
    for index in (0, 3):
        p = make_pair(index, H, W, 32)
        c = pair_gt_corrs(index, H, W, 500)
        assert c.dtype == torch.int64 and c.shape[1] == 4 and 50 < c.shape[0] <= 500
        assert len({tuple(r) for r in c[:, 2:].tolist()}) == c.shape[0]                    # one per query pixel
        assert bool(p["mask_a"][c[:, 0], c[:, 1]].all()) and bool(p["mask_q"][c[:, 2], c[:, 3]].all())
        diff = p["feat_q"][:, c[:, 2], c[:, 3]] - p["feat_a"][:, c[:, 0], c[:, 1]]       # the anchor's descriptor plus 0.05 N(0,1)
        assert 0.03 < float(diff.std()) < 0.07 and float(diff.abs().max()) < 0.05 * 6
        few = pair_gt_corrs(index, H, W, 40)
        assert few.shape == (40, 4) and {tuple(r) for r in few.tolist()} <= {tuple(r) for r in pair_gt_corrs(index, H, W, 10**6).tolist()}


def test_new_symbols_and_defaults():
    import re
    from oryon_amd import _lib
    from oryon_amd.pipeline import Pipeline, default_args
    hdr = open(os.path.join(ROOT, "include", "oryon_hip.h")).read()
    L = _lib.lib()
    for name in ("oryon_feature_loss_workspace_bytes", "oryon_feature_loss", "oryon_mask_dice_sums"):
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\s*\(", hdr) and hasattr(L, name)
    assert L.oryon_feature_loss_workspace_bytes(64, 500, 2000) > 0 and L.oryon_feature_loss_workspace_bytes(0, 500, 2000) == 0
    assert L.oryon_feature_loss_workspace_bytes(1, 0, 0) == 0
    # argument checks come before any launch or dereference (0x1000 stands for a non-NULL pointer); each rejection names its check
    nul = [None] * 6

    def rejected(code, why):
        msg = L.oryon_last_error().decode()
        assert code == -1 and why in msg, (code, msg)
    rejected(L.oryon_feature_loss(None, None, 1, 257, 8, 8, None, 4, None, None, 0, 0, 0.2, 0.9, 5.0, None, 0, *nul), "exceeds 256 channels")
    rejected(L.oryon_feature_loss(None, None, 1, 32, 8, 8, None, 4, None, None, 0, 1, 0.2, 0.9, 5.0, None, 0, *nul),
             "pool ? n_pool > 0 : pool_mode == 0")                         # one negative per positive, but no table
    rejected(L.oryon_feature_loss(None, None, 1, 32, 8, 8, None, 4, None, 0x1000, 5, 1, 0.2, 0.9, 5.0, None, 0, *nul),
             "n_pool == n_corr")                                           # a pool-per-positive table of the wrong length
    rejected(L.oryon_feature_loss(None, None, 1, 32, 8, 8, None, 4, None, 0x1000, 0, 0, 0.2, 0.9, 5.0, None, 0, *nul),
             "pool ? n_pool > 0 : pool_mode == 0")                         # a table of no candidates
    rejected(L.oryon_feature_loss(None, None, 1, 32, 8, 8, None, 4, None, None, 0, 2, 0.2, 0.9, 5.0, None, 0, *nul), "pool_mode == 0 || pool_mode == 1")
    rejected(L.oryon_feature_loss(None, None, 1, 32, 8, 8, None, 4, None, None, 0, 0, 0.2, 0.9, 5.0, None, 0, *nul), "losses")   # no outputs
    rejected(L.oryon_mask_dice_sums(None, None, 1, 8, 8, 0.5, None, None, None, None), "logits && gt")
    a = default_args()
    assert a.debug_valid is False and a.loss.hard_negatives is True and (a.loss.pos_margin, a.loss.neg_margin, a.loss.neg_kernel_size) == (0.2, 0.9, 5)
    assert a.loss.mask_type == "dice" and a.loss.w == {"mask": 1.0, "pos": 0.5, "neg": 0.5}
    pipe = Pipeline(default_args(**{"test.solver": "ransac"}))
    loss, w = pipe.reduce_losses({"mask": torch.tensor(0.4), "pos": torch.tensor(0.2), "neg": torch.tensor(0.6)})
    assert abs(float(loss) - (0.4 + 0.1 + 0.3)) < 1e-6 and set(w) == {"mask", "pos", "neg"} and abs(float(w["neg"]) - 0.3) < 1e-6
    from oryon_amd.losses import FeatureLoss
    for kind in ("lovasz", "focal"):
        with pytest.raises(NotImplementedError, match=kind):
            FeatureLoss(default_args(**{"loss.mask_type": kind}), "cuda")
    import run_valid
    assert run_valid.parse(["--pairs", "4", "--debug-valid"]).debug_valid and not run_valid.parse([]).debug_valid
