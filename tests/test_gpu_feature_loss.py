"""GPU tests of the validation step: csrc/feature_loss.hip through ops.feature_loss / ops.mask_dice_sums, losses.FeatureLoss,
Pipeline.validation_step and run_valid.py, against the reference's recorded results (tests/golden/floss_*.npz) and the float64
restatement (tests/feature_loss_restatement.py).

Bars (ISSUE "Bars"): negative indices equal to the golden's on EVERY row; distances, per-pair terms, batch losses and the dice loss
within 1e-6.  The four dice sums against the restatement's float64 sums: both sides add the same float64 terms p, p^2 (exp, one
division, one product: <= 4 u relative each, u = 2^-53) in different orders (<= n u relative), so 8 n u with n = H W bounds the
difference; that is 2.1e-12 at 48 x 48."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feature_loss_restatement as fr
from test_feature_loss_restatement import BAR, FIXTURES, NAMES, ROOT, load

pytestmark = pytest.mark.gpu
DEV = "cuda"
_cache = {}


def fixture(name):
    """The golden, the restatement of it (computed once, shared, never modified) and its device tensors."""
    if name not in _cache:
        f = load(FIXTURES[NAMES.index(name)])
        r = fr.restate(f["feat_a"], f["feat_q"], f["corrs"], f["valid"], f["image_hw"], f["pool"])
        _cache[name] = (f, r)
    return _cache[name]


def padded(real: torch.Tensor, fill, extra=4096):
    """`real` as a contiguous view at the start of a larger buffer whose tail holds `fill`: a kernel that read past the end of its input
    would pick `fill` up; nothing outside the allocation is ever touched."""
    buf = torch.full((real.numel() + extra,), fill, dtype=real.dtype, device=DEV)
    buf[:real.numel()] = real.flatten().to(DEV)
    return buf[:real.numel()].view(real.shape)


def device_inputs(f, r, copies=1):
    rep = lambda x: np.concatenate([x] * copies)
    fa = padded(torch.from_numpy(rep(f["feat_a"])), float("nan"))
    fq = padded(torch.from_numpy(rep(f["feat_q"])), float("nan"))
    corrs = padded(torch.from_numpy(rep(r["pix"])).to(torch.int32), 1 << 30)
    valid = padded(torch.from_numpy(rep(f["valid"])).to(torch.int32), 1)
    pool = None if f["pool"] is None else padded(torch.from_numpy(rep(f["pool"])).to(torch.int32), 1 << 30)
    return fa, fq, corrs, valid, pool


@pytest.mark.parametrize("name", NAMES)
def test_feature_loss_kernel_against_the_reference(name):
    from oryon_amd import ops
    f, r = fixture(name)
    FW = f["feat_a"].shape[3]
    out = {k: v.cpu().numpy() for k, v in ops.feature_loss(*device_inputs(f, r)).items()}
    want_idx = np.stack([f["neg_a"], f["neg_q"]], axis=1)
    got_idx = np.stack([out["neg_idx"] // FW, out["neg_idx"] % FW], axis=-1)
    assert np.array_equal(r["neg_idx"] // FW, want_idx[..., 0]) and np.array_equal(r["neg_idx"] % FW, want_idx[..., 1])   # the restatement first
    wrong = int((got_idx != want_idx).any(-1).sum())
    d = {"d_pos": np.abs(out["d_pos"] - f["d_pos"]).max(), "d_neg_a": np.abs(out["d_neg"][:, 0] - f["d_neg_a"]).max(),
         "d_neg_q": np.abs(out["d_neg"][:, 1] - f["d_neg_q"]).max(), "pair_terms": np.abs(out["pair_terms"] - r["pair_terms"]).max(),
         "pos": abs(out["losses"][0] - f["loss_pos"]), "neg": abs(0.5 * (float(out["losses"][1]) + float(out["losses"][2])) - f["loss_neg"]),
         "losses_vs_restatement": np.abs(out["losses"] - r["losses"]).max()}
    print(name, f"rows with another negative: {wrong} of {want_idx[..., 0].size};", {k: f"{v:.2e}" for k, v in d.items()})
    assert np.isfinite(out["d_pos"]).all() and np.isfinite(out["d_neg"]).all()
    assert wrong == 0
    assert max(d.values()) <= BAR, d
    for b, v in enumerate(f["valid"]):
        if v != 1:                                                         # an invalid pair: zeros, exactly
            assert not out["d_pos"][b].any() and not out["d_neg"][b].any() and not out["neg_idx"][b].any() and not out["pair_terms"][b].any()
    if not f["valid"].any():
        assert out["losses"].tolist() == [0.0, 0.0, 0.0]


def test_feature_loss_one_negative_per_positive():
    """loss.hard_negatives = False: the pool table names every positive's negative; no exclusion disc, no search."""
    from oryon_amd import ops
    f, r = fixture("1_rescale")
    pool = np.random.default_rng(0).integers(0, 1600, (3, 2, 64))
    want = fr.restate(f["feat_a"], f["feat_q"], f["corrs"], f["valid"], f["image_hw"], pool, per_positive=True)
    fa, fq, corrs, valid, _ = device_inputs(f, r)
    out = ops.feature_loss(fa, fq, corrs, valid, padded(torch.from_numpy(pool).to(torch.int32), 1 << 30), pool_per_positive=True)
    assert np.array_equal(out["neg_idx"].cpu().numpy(), want["neg_idx"])
    d = max(np.abs(out["d_neg"].cpu().numpy() - want["d_neg"]).max(), np.abs(out["pair_terms"].cpu().numpy() - want["pair_terms"]).max(),
            np.abs(out["losses"].cpu().numpy() - want["losses"]).max())
    print(f"one negative per positive: max difference {d:.2e}")
    assert d <= BAR


@pytest.mark.parametrize("name", ["2_nonsquare", "3_pool", "7_none_valid"])
def test_mask_dice_sums(name):
    from oryon_amd import ops
    from oryon_amd.pipeline import mask_iou
    f, _ = fixture(name)
    for key in ("a", "q"):
        logits = torch.from_numpy(f["logits_" + key][:, 0])
        gt = torch.from_numpy(fr.resize_nearest(f["gt_" + key], logits.shape[1:]).astype(np.int32))
        sums, mask, counts = ops.mask_dice_sums(padded(logits, float("nan")), padded(gt, 1), 0.5)
        want = fr.dice_sums(logits.numpy(), gt.numpy())
        n = logits.shape[1] * logits.shape[2]
        rel = float(np.abs(sums.cpu().numpy() - want).max() / want.max())
        loss = fr.dice_loss(sums.cpu().numpy(), n)
        ref_loss, ref_mask, _ = fr.mask_terms(f["logits_" + key], f["gt_" + key], 0.5)
        print(f"{name} {key}: sums rel {rel:.2e} (bound {8 * n * 2.0 ** -53:.2e}), dice {loss:.9f} vs restatement {ref_loss:.9f}")
        assert rel <= 8 * n * 2.0 ** -53 and abs(loss - ref_loss) <= BAR
        m0 = ops.mask_from_logits(logits.to(DEV), 0.5)
        assert torch.equal(mask, m0) and np.array_equal(mask.cpu().numpy(), f["mask_" + key])
        iou = counts[:, 0].float() / counts[:, 1].float()
        assert torch.equal(iou, mask_iou(gt.to(DEV), m0)) and np.allclose(iou.cpu().numpy(), f["iou_" + key], rtol=1e-6)


def _batch_of(f):
    B, _, IH, IW = (len(f["valid"]), 3) + f["image_hw"]
    batch = {"corrs": torch.from_numpy(f["corrs"]).long(), "valid": torch.from_numpy(f["valid"]),
             "anchor": {"rgb": torch.zeros(B, 3, IH, IW), "mask": torch.from_numpy(f["gt_a"])},
             "query": {"rgb": torch.zeros(B, 3, IH, IW), "mask": torch.from_numpy(f["gt_q"])}}
    outputs = {"featmap_a": torch.from_numpy(f["feat_a"]).to(DEV), "featmap_q": torch.from_numpy(f["feat_q"]).to(DEV),
               "mask_a": torch.from_numpy(f["logits_a"]).to(DEV), "mask_q": torch.from_numpy(f["logits_q"]).to(DEV)}
    return batch, outputs


@pytest.mark.parametrize("name", NAMES)
def test_feature_loss_forward_against_the_reference(name, monkeypatch):
    """losses.FeatureLoss.forward with the reference's names and shapes.  Fixture 3's pool is a random draw; the golden's tables (drawn
    by the reference on the CPU generator) are replayed through torch.multinomial, which also checks the arguments and the order of the
    calls: anchors first, one per valid pair."""
    from oryon_amd.losses import FeatureLoss
    from oryon_amd.pipeline import default_args
    f, _ = fixture(name)
    batch, outputs = _batch_of(f)
    HW = f["feat_a"].shape[2] * f["feat_a"].shape[3]
    if f["pool"] is not None:
        tables = iter([f["pool"][b, side] for side in (0, 1) for b in range(len(f["valid"])) if f["valid"][b] == 1])

        def replay(w, n, replacement=False):
            assert w.dtype == torch.float64 and w.shape == (HW,) and w.is_cuda and bool((w == 1).all()) and n == 2000 and not replacement
            return torch.from_numpy(next(tables)).to(w.device)
        monkeypatch.setattr(torch, "multinomial", replay)
    losses, res = FeatureLoss(default_args(), DEV).forward(batch, outputs)
    monkeypatch.undo()
    d = {k: abs(float(losses[k]) - float(f["loss_" + k])) for k in ("mask", "pos", "neg")}
    for k, g in (("d_pos", "d_pos"), ("d_neg_a", "d_neg_a"), ("d_neg_q", "d_neg_q")):
        d[k] = float(np.abs(res[k].cpu().numpy() - f[g]).max())
    print(name, {k: f"{v:.2e}" for k, v in d.items()})
    assert set(losses) == {"mask", "pos", "neg"} and max(d.values()) <= BAR, d
    for k in ("neg_a", "neg_q"):
        assert res[k].dtype == torch.float32 and np.array_equal(res[k].cpu().numpy(), f[k]), k
    for k in ("mask_a", "mask_q"):
        assert np.array_equal(res[k].cpu().numpy(), f[k])
        assert torch.equal(res["logits_" + k[-1]], outputs[k][:, 0])
        assert np.allclose(res["iou_" + k[-1]].cpu().numpy(), f["iou_" + k[-1]], rtol=1e-6)


@pytest.mark.parametrize("hard", [True, False])
def test_forward_leaves_the_generators_where_feature_loss_rng_draws_leaves_them(hard):
    from oryon_amd.losses import FeatureLoss
    from oryon_amd.pipeline import Pipeline, default_args
    f, _ = fixture("3_pool")
    batch, outputs = _batch_of(f)
    args = default_args(**{"loss.hard_negatives": hard, "test.solver": "ransac"})
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    cpu0, gpu0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    FeatureLoss(args, DEV).forward(batch, outputs)
    cpu1, gpu1 = torch.get_rng_state(), torch.cuda.get_rng_state()
    torch.set_rng_state(cpu0)
    torch.cuda.set_rng_state(gpu0)
    n = Pipeline(args).feature_loss_rng_draws(batch, outputs)
    assert n == 4
    assert torch.equal(torch.get_rng_state(), cpu1) and torch.equal(torch.cuda.get_rng_state(), gpu1)
    assert not torch.equal(gpu1, gpu0) if hard else not torch.equal(cpu1, cpu0)


def test_bit_stability_across_runs_streams_and_batch_shapes():
    from oryon_amd import ops
    f, r = fixture("3_pool")
    keys = ("d_pos", "d_neg", "neg_idx", "pair_terms", "losses")
    first = ops.feature_loss(*device_inputs(f, r))
    again = ops.feature_loss(*device_inputs(f, r))
    side = torch.cuda.Stream()
    inp = device_inputs(f, r)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.feature_loss(*inp)
    side.synchronize()
    four = ops.feature_loss(*device_inputs(f, r, copies=4))
    torch.cuda.synchronize()
    raw = lambda t: t.cpu().numpy().tobytes()
    for k in keys:
        assert raw(first[k]) == raw(again[k]) == raw(other[k]), k
    B = len(f["valid"])
    for k in keys[:-1]:
        for c in range(4):
            assert raw(four[k][c * B:(c + 1) * B]) == raw(first[k]), (k, c)
    # the batch means too: pair b sits in lane b of the xor tree, so the 4 x 2 pairs (a, b, a, b, ...) add up as 4 a + 4 b, which is
    # 4 (a + b) exactly in float64, and / 8 gives (a + b) / 2 exactly
    assert raw(four["losses"]) == raw(first["losses"])


_CHANNEL_STEPS = """
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from oryon_amd import ops
z = np.load(sys.argv[2])
out = {}
for C in (int(c) for c in sys.argv[4:]):
    fa, fq = (torch.from_numpy(np.ascontiguousarray(z[k][:, :C])).cuda() for k in ("feat_a", "feat_q"))
    r = ops.feature_loss(fa, fq, torch.from_numpy(z["pix"]).cuda(), torch.from_numpy(z["valid"]).cuda())
    torch.cuda.synchronize()
    out.update({f"{k}_{C}": v.cpu().numpy() for k, v in r.items()})
np.savez(sys.argv[3], **out)
"""


def test_channel_counts_in_any_order_within_one_process(tmp_path):
    """The kernel's dynamic LDS grows with C (512 C bytes) and the opt-in above the default limit is made once per process, so whether
    a shape runs must not depend on the calls before it.  A fresh process (the call history is the subject here) runs fixture 4 cut to
    its first 97 channels (just past the default limit), then to 128, then whole (C = 256, 128 KB), then 128 again.  Each result is held
    to the restatement of the same cut: distances, terms and losses within the 1e-6 bar (for 128 the later of its two runs).  The cuts
    have no recorded top-2 gap, so their negatives are held through d_neg and only counted; the whole map has one, and its negatives
    equal the restatement's, which equal the golden's, on every row."""
    f, r = fixture("4_c256")
    FH, FW = f["feat_a"].shape[2:]
    src = tmp_path / "in.npz"
    np.savez(src, feat_a=f["feat_a"], feat_q=f["feat_q"], pix=r["pix"].astype(np.int32), valid=f["valid"].astype(np.int32))
    steps = (97, 128, 256, 128)
    p = subprocess.run([sys.executable, "-c", _CHANNEL_STEPS, ROOT, str(src), str(tmp_path / "out.npz")] + [str(c) for c in steps],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    for C in sorted(set(steps)):
        want = fr.restate(f["feat_a"][:, :C], f["feat_q"][:, :C], f["corrs"], f["valid"], f["image_hw"])
        d = {k: float(np.abs(got[f"{k}_{C}"] - want[k]).max()) for k in ("d_pos", "d_neg", "pair_terms", "losses")}
        same = int((got[f"neg_idx_{C}"] == want["neg_idx"]).sum())
        print(f"C = {C}:", {k: f"{v:.2e}" for k, v in d.items()}, f"same negative on {same} of {want['neg_idx'].size} rows")
        assert max(d.values()) <= BAR, (C, d)
        if C == 256:
            assert same == want["neg_idx"].size
        idx = got[f"neg_idx_{C}"]
        assert ((idx >= 0) & (idx < FH * FW)).all()


def _valid_pipeline(debug_valid):
    from oryon_amd.pipeline import Pipeline, default_args
    from test_gpu_pipeline import _solver
    args = default_args(**{"test.mask": "oracle", "model.image_encoder.img_size": [48, 48], "dataset.img_size": [48, 48],
                           "debug_valid": debug_valid})
    return Pipeline(args, pointdsc_solver=_solver())


def _valid_batch():
    sys.path.insert(0, ROOT)
    import run_test
    import run_valid
    return run_valid.synthetic_valid_batch(run_test, 3, 4, 48, 32, DEV, 500)


def test_validation_step_on_synthetic_pairs():
    pl = _valid_pipeline(False)
    batch, pairs = _valid_batch()
    assert batch["corrs"].shape == (4, 500, 4) and batch["valid"].tolist() == [1.0] * 4
    torch.manual_seed(1)
    pl.on_validation_start()
    loss, log = pl.validation_step(batch, 0)
    assert set(log) == {"valid/mask", "valid/pos", "valid/neg", "valid/loss"} and float(log["valid/loss"]) == float(loss)
    assert all(np.isfinite(float(v)) for v in log.values())
    w = pl.args.loss.w
    res = pl.last_validation
    assert abs(float(loss) - sum(w[k] * float(res["losses"][k]) for k in w)) < 1e-6
    ev = pl.evaluator
    assert "cls_id" not in ev.metrics and all(len(v) == 4 for v in ev.metrics.values()) and all(len(v) == 4 for v in ev.counts.values())
    terms = res["results"]["pair_terms"].cpu().numpy()
    print("validation_step: pair terms (pos, neg_a, neg_q)", terms.tolist(), "log", {k: float(v) for k, v in log.items()})
    assert (terms[:, 0] < terms[:, 1]).all()                            # the query descriptors are the anchor's plus 0.05 noise
    for i in range(4):                                                  # the matcher's poses are the generator's
        T, gt = res["poses"][i].numpy(), pairs[i]["pose"].numpy()
        assert np.abs(T[:3, :3] - gt[:3, :3]).max() < 1e-2 and np.abs(T[:3, 3] - gt[:3, 3]).max() < 5e-3
    end = pl.on_validation_end()
    assert end["FMR"] == 1.0 and end["Missing segm"] == 0 and abs(end["valid/loss"] - float(loss)) < 1e-7 and "R error" in end


def test_validation_step_debug_valid_uses_the_ground_truth_correspondences():
    pl = _valid_pipeline(True)
    batch, pairs = _valid_batch()
    pl.on_validation_start()
    pl.validation_step(batch, 0)
    res = pl.last_validation
    outputs = pl.model.forward(batch)
    assert res["status"] == [0, 0, 0, 0]
    for i in range(4):
        corrs = pl.gt_featmap_corrs(batch, outputs, i)
        assert torch.equal(corrs, batch["corrs"][i])                    # the image frame is the map's here: the rescale is the identity
        assert torch.equal(res["poses"][i], pl.get_pose(batch, corrs, i).cpu())
    assert pl.evaluator.pose_recall_th[0] == min(pl.evaluator.pose_recall_th)
    tight = "Recall ({}deg, {}cm)".format(*pl.evaluator.pose_recall_th[0])
    print("debug_valid:", tight, pl.evaluator.metrics[tight], "R error", pl.evaluator.metrics["R error"], "T error", pl.evaluator.metrics["T error"])
    assert pl.evaluator.metrics[tight] == [1.0] * 4 and pl.evaluator.counts["Missing segm"] == [0] * 4
    batch["valid"][2] = 0.0                                             # no ground-truth correspondences: the failure path
    pl.validation_step(batch, 1)
    assert pl.last_validation["status"] == [0, 0, 2, 0] and torch.equal(pl.last_validation["poses"][2], torch.eye(4))
    assert pl.evaluator.metrics[tight] == [1.0] * 4 + [1.0, 1.0, 0, 1.0] and pl.evaluator.counts["Missing segm"] == [0] * 6 + [1, 0]


def test_run_valid_driver():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_valid.py"), "--pairs", "4", "--batch", "2", "--size", "48"],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["pairs"] == 4 and all(np.isfinite(out[k]) for k in ("valid/mask", "valid/pos", "valid/neg", "valid/loss"))
    assert 0.0 <= out["FMR"] <= 1.0 and "R error" in out and "Mean IoU" in out
