"""GPU tests of the training step: csrc/feature_loss_grad.hip through ops.feature_loss_grad / ops.mask_dice_grad, the autograd functions of
losses.FeatureLoss, Pipeline.training_step / configure_optimizers and run_train.py, against torch's recorded gradients of the reference's
loss (tests/golden/flossgrad_*.npz) and the float64 restatement (tests/feature_loss_grad_restatement.py).

Bars (derived and measured in tests/test_feature_loss_grad_restatement.py, see its docstring): every element of a map gradient within
R (|want| + S) of the golden and of the restatement, R = 4 R_REF = 5.2e-3, S = the summed magnitudes of the terms of the element; and,
because that is wide, within TIGHT S = 16 * 2^-24 S of the restatement, which is what the kernel's arithmetic (float64 slots rounded
once, at most 16 fp32 additions per pixel) allows.  Logit gradients within R (|want| + |want|) of the restatement and within
R (|want| + T) of the golden.  Untouched elements, invalid pairs and fixture 7's maps are exactly 0; everything is finite.
Parameter gradients of a training step: param_ratio <= R_PARAM = 4 R_PARAM_REF = 8.8e-4."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feature_loss_grad_restatement as gr
import feature_loss_restatement as fr
from test_feature_loss_grad_restatement import (GRAD_NAMES, R, R_PARAM, ROOT, TIGHT, load_grad, param_ratio, small_training_setup, torch_total_loss,
                                                worst_ratio)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
SENTINEL = -7.5


def padded(real: torch.Tensor, fill, extra=4096):
    """`real` as a contiguous view at the start of a larger buffer whose tail holds `fill`: a kernel that read past the end of its input
    would pick `fill` up; nothing outside the allocation is ever touched."""
    buf = torch.full((real.numel() + extra,), fill, dtype=real.dtype, device=DEV)
    buf[:real.numel()] = real.flatten().to(DEV)
    return buf[:real.numel()].view(real.shape)


def guarded(shape):
    """-> (a contiguous fp32 view of `shape` holding SENTINEL, the whole buffer): the GUARD elements behind the view must stay SENTINEL."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf[:n].view(shape), buf


def tail_intact(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def device_inputs(f, r, copies=1):
    rep = lambda x: np.concatenate([x] * copies)
    fa = padded(torch.from_numpy(rep(f["feat_a"])), float("nan"))
    fq = padded(torch.from_numpy(rep(f["feat_q"])), float("nan"))
    corrs = padded(torch.from_numpy(rep(r["pix"])).to(torch.int32), 1 << 30)
    valid = padded(torch.from_numpy(rep(f["valid"])).to(torch.int32), 1)
    pool = None if f["pool"] is None else padded(torch.from_numpy(rep(f["pool"])).to(torch.int32), 1 << 30)
    return fa, fq, corrs, valid, pool


def map_gradients(f, r, g_host, pm, nm, copies=1, pool=None, per_positive=False):
    """ops.feature_loss, then ops.feature_loss_grad on its outputs held in padded buffers, into guarded outputs."""
    from oryon_amd import ops
    fa, fq, corrs, valid, fpool = device_inputs(f, r, copies)
    out = ops.feature_loss(fa, fq, corrs, valid, fpool if pool is None else pool, pm, nm, pool_per_positive=per_positive)
    neg_idx, d_pos, d_neg = padded(out["neg_idx"], 1 << 30), padded(out["d_pos"], float("nan")), padded(out["d_neg"], float("nan"))
    g = padded(torch.tensor(g_host, dtype=torch.float32), float("nan"))
    (ga, buf_a), (gq, buf_q) = guarded(fa.shape), guarded(fa.shape)
    ops.feature_loss_grad(fa, fq, corrs, valid, neg_idx, d_pos, d_neg, g, pm, nm, out=(ga, gq))
    torch.cuda.synchronize()
    assert tail_intact(buf_a, ga.numel()) and tail_intact(buf_q, gq.numel())
    return ga, gq, out


@pytest.mark.parametrize("name", GRAD_NAMES)
def test_map_gradient_kernel_against_the_reference(name):
    f, g, w = load_grad(name)
    pm, nm = float(g["pos_margin"]), float(g["neg_margin"])
    ga, gq, out = map_gradients(f, w["r"], g["g"].tolist(), pm, nm)
    assert np.array_equal(out["neg_idx"].cpu().numpy(), w["r"]["neg_idx"])          # the same negatives as the golden's and the restatement's
    slots = max([int(np.bincount(np.concatenate([w["r"]["pix"][b, :, 2 * s] * f["feat_a"].shape[3] + w["r"]["pix"][b, :, 2 * s + 1],
                                                 w["r"]["neg_idx"][b, s]])).max()) for b in range(len(f["valid"])) for s in (0, 1)
                 if f["valid"][b] == 1], default=0)
    assert slots <= 16                                                              # TIGHT's premise
    for s, got in enumerate((ga.cpu().numpy(), gq.cpu().numpy())):
        key = "aq"[s]
        want, S = w["G"][s], w["S"][s]
        assert np.isfinite(got).all()
        ratio = {"golden": worst_ratio(got, g["grad_" + key].astype(np.float64), S), "restatement": worst_ratio(got, want, S)}
        tight = float((np.abs(got - want) / np.maximum(S, 1e-300)).max())
        print(name, key, {k: f"{v:.2e}" for k, v in ratio.items()}, f"|got - want| / S {tight:.2e} (bar {TIGHT:.2e});",
              f"largest |gradient| {np.abs(got).max():.3g}, most slots on one pixel {slots}")
        assert max(ratio.values()) <= R, ratio
        assert (np.abs(got - want) <= TIGHT * S).all()
        off = ~np.broadcast_to(w["on"][s][:, None], got.shape)
        assert not got[off].any()                                                   # untouched elements: exactly 0
        for b, v in enumerate(f["valid"]):
            if v != 1:
                assert not got[b].any()
    if name == "6_zero_dup_border":
        assert np.abs(ga.cpu().numpy()).max() > 1e5                                # the zero descriptor at a positive: v^ / eps


@pytest.mark.parametrize("name", GRAD_NAMES)
def test_dice_gradient_kernel_against_the_reference(name):
    from oryon_amd import ops
    f, g, w = load_grad(name)
    for key in "aq":
        logits = torch.from_numpy(f["logits_" + key][:, 0])
        gt = torch.from_numpy(fr.resize_nearest(f["gt_" + key], logits.shape[1:]).astype(np.int32))
        x, t = padded(logits, float("nan")), padded(gt, 1)
        sums, _, _ = ops.mask_dice_sums(x, t, 0.5)
        out, buf = guarded(x.shape)
        ops.mask_dice_grad(x, t, padded(sums, float("nan")), padded(torch.tensor([float(g["g_mask"])]), float("nan")), out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want, T = w["logits"][key], w["logit_terms"][key]
        ratio = {"restatement": worst_ratio(got, want, np.abs(want)), "golden": worst_ratio(got, g["grad_logits_" + key].astype(np.float64), T)}
        print(name, key, {k: f"{v:.2e}" for k, v in ratio.items()})
        assert tail_intact(buf, out.numel()) and np.isfinite(got).all() and max(ratio.values()) <= R, ratio
        # float64 inside: one fp32 rounding of the result (2^-24 |want|) and the float64 rounding of p, which 1 - p and the difference
        # of the two brackets carry over on the scale of the terms (a few 2^-53 T)
        assert (np.abs(got - want) <= 2.0 ** -24 * np.abs(want) + 2.0 ** -50 * T).all()


def test_one_negative_per_positive_on_the_positives_own_pixel():
    """pool_per_positive with a table that names each positive's own pixel: slots n and N + n land on one pixel and u = w.  Against the
    restatement only.  d(u, u) has no gradient, so in the rows the positive margin clamps both sides hold nothing but float64
    rounding noise of the size 2^-52 |u^| |beta| / |u|; the bar carries that floor as 1e-12 of the largest gradient."""
    f, g, w = load_grad("1_rescale")
    pix = w["r"]["pix"]
    own = np.stack([pix[..., 0] * 40 + pix[..., 1], pix[..., 2] * 40 + pix[..., 3]], axis=1)
    pool = padded(torch.from_numpy(own).to(torch.int32), 1 << 30)
    ga, gq, out = map_gradients(f, w["r"], [0.5, 0.25, 0.25], 0.2, 0.9, pool=pool, per_positive=True)
    idx = out["neg_idx"].cpu().numpy()
    assert f["valid"].tolist() == [1.0, 0.0, 1.0]
    assert np.array_equal(idx[[0, 2]], own[[0, 2]]) and not idx[1].any()             # the forward leaves an invalid pair at zero
    G, S, active = gr.map_grads(f["feat_a"], f["feat_q"], pix, f["valid"], own, (0.5, 0.25, 0.25))
    assert active[0, 1:].all()
    for s, got in enumerate((ga.cpu().numpy(), gq.cpu().numpy())):
        err = np.abs(got - G[s])
        print("own pixel", "aq"[s], f"largest |got - want| {err.max():.2e}, largest gradient {np.abs(G[s]).max():.2e}")
        assert np.isfinite(got).all() and (err <= TIGHT * S[s] + 1e-12 * np.abs(G[s]).max()).all()
        assert not got[1].any()


def test_bit_stability_across_runs_streams_and_batch_shapes():
    """Fixture 3 twice, on a second stream, and as four copies in one batch.  In the batch of four V is 4 x 2, so its upstream gradient is
    4 g: alpha = 4 g / (8 N) is g / (2 N) exactly (a power of two), and every copy must hold the bytes of the single run."""
    f, g, w = load_grad("3_pool")
    gh = g["g"].tolist()
    first = map_gradients(f, w["r"], gh, 0.2, 0.9)[:2]
    again = map_gradients(f, w["r"], gh, 0.2, 0.9)[:2]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = map_gradients(f, w["r"], gh, 0.2, 0.9)[:2]
    side.synchronize()
    four = map_gradients(f, w["r"], [4 * v for v in gh], 0.2, 0.9, copies=4)[:2]
    torch.cuda.synchronize()
    raw = lambda t: t.cpu().numpy().tobytes()
    B = len(f["valid"])
    for s in (0, 1):
        assert first[s].abs().max() > 0
        assert raw(first[s]) == raw(again[s]) == raw(other[s]), s
        for c in range(4):
            assert raw(four[s][c * B:(c + 1) * B]) == raw(first[s]), (s, c)


def _batch_of(f, requires_grad):
    B, _, IH, IW = (len(f["valid"]), 3) + f["image_hw"]
    batch = {"corrs": torch.from_numpy(f["corrs"]).long(), "valid": torch.from_numpy(f["valid"]),
             "anchor": {"rgb": torch.zeros(B, 3, IH, IW), "mask": torch.from_numpy(f["gt_a"])},
             "query": {"rgb": torch.zeros(B, 3, IH, IW), "mask": torch.from_numpy(f["gt_q"])}}
    outputs = {"featmap_a": torch.from_numpy(f["feat_a"]).to(DEV), "featmap_q": torch.from_numpy(f["feat_q"]).to(DEV),
               "mask_a": torch.from_numpy(f["logits_a"]).to(DEV), "mask_q": torch.from_numpy(f["logits_q"]).to(DEV)}
    for v in outputs.values():
        v.requires_grad_(requires_grad)
    return batch, outputs


def _direct(f, w, scale):
    """The gradients of scale * (1.0 mask + 0.5 pos + 0.5 neg) by direct kernel calls."""
    from oryon_amd import ops
    ga, gq, _ = map_gradients(f, w["r"], [0.5 * scale, 0.25 * scale, 0.25 * scale], 0.2, 0.9)
    gl = []
    for key in "aq":
        logits = torch.from_numpy(f["logits_" + key][:, 0]).to(DEV)
        gt = torch.from_numpy(fr.resize_nearest(f["gt_" + key], logits.shape[1:]).astype(np.int32)).to(DEV)
        sums, _, _ = ops.mask_dice_sums(logits, gt, 0.5)
        gl.append(ops.mask_dice_grad(logits, gt, sums, torch.tensor([0.5 * scale], device=DEV))[:, None])
    return ga, gq, gl[0], gl[1]


@pytest.mark.parametrize("name", ["1_rescale", "6_zero_dup_border", "7_none_valid"])
def test_feature_loss_autograd(name):
    """FeatureLoss.forward on maps and logits that require grad, then backward: the gradients of the direct kernel calls, byte for byte;
    under no_grad (and for inputs that do not require grad) the inference path, byte for byte; a non-unit upstream."""
    from oryon_amd.losses import FeatureLoss
    from oryon_amd.pipeline import Pipeline, default_args
    f, g, w = load_grad(name)
    args = default_args(**{"test.solver": "ransac"})
    pipe = Pipeline(args)
    keys = ("featmap_a", "featmap_q", "mask_a", "mask_q")

    def run(scale, requires_grad=True, no_grad=False):
        batch, outputs = _batch_of(f, requires_grad)
        with torch.no_grad() if no_grad else torch.enable_grad():
            losses, results = FeatureLoss(args, DEV).forward(batch, outputs)
            total, _ = pipe.reduce_losses(losses)
        if requires_grad and not no_grad:
            assert total.requires_grad and total.grad_fn is not None
            (scale * total).backward()
        return losses, results, outputs

    losses, results, outputs = run(1.0)
    assert all(not v.requires_grad for v in results.values())                       # the results stay detached
    want = _direct(f, w, 1.0)
    for k, d in zip(keys, want):
        got = outputs[k].grad if outputs[k].grad is not None else torch.zeros_like(outputs[k])
        assert got.shape == d.shape and torch.equal(got, d), k
    # the inference path: no_grad, and inputs that do not require grad
    for kw in (dict(no_grad=True), dict(requires_grad=False)):
        l0, r0, _ = run(1.0, **kw)
        assert all(v.grad_fn is None and not v.requires_grad for v in l0.values())
        for k in losses:
            assert l0[k].cpu().numpy().tobytes() == losses[k].detach().cpu().numpy().tobytes(), k
        for k in results:
            assert torch.equal(r0[k], results[k]) or bool(torch.isnan(r0[k]).any()), k
    # 3 x the loss: the kernel sees 3 g (exact), so the result is that of the direct call with 3 g, byte for byte; a row's margin test
    # does not see g, so the same elements are zero; against 3 x the unit result only the fp32 roundings differ (of the slots and their
    # sums for the maps: 3 TIGHT S; one per element for the logits)
    _, _, outputs3 = run(3.0)
    scales = (w["S"][0], w["S"][1], None, None)
    for k, d3, d1, S in zip(keys, _direct(f, w, 3.0), want, scales):
        got = outputs3[k].grad if outputs3[k].grad is not None else torch.zeros_like(outputs3[k])
        assert torch.equal(got, d3) and torch.equal(got == 0, d1 == 0), k
        err = (got.double() - 3.0 * d1.double()).abs().cpu().numpy()
        assert (err <= (3 * TIGHT * S if S is not None else 2.0 ** -22 * (3.0 * d1).abs().cpu().numpy())).all(), k
    # 4 x the loss: a power of two scales every float64 slot, its fp32 rounding and every fp32 sum exactly
    _, _, outputs4 = run(4.0)
    for k, d1 in zip(keys, want):
        got = outputs4[k].grad if outputs4[k].grad is not None else torch.zeros_like(outputs4[k])
        assert torch.equal(got, 4.0 * d1), k


def test_training_step_parameter_gradients_and_one_optimizer_step():
    """One training step on a small Oryon, B = 2: the parameter gradients through the HIP loss against the same step through the torch
    statement of the loss fed the HIP forward's negatives (param_ratio <= R_PARAM); the log; then one AdamW step: the frozen towers are
    byte-unchanged, every trainable tensor with a gradient has moved."""
    from oryon_amd.pipeline import Pipeline, default_args
    model, batch, pix = small_training_setup(DEV, 2)
    S = 192
    args = default_args(**{"test.solver": "ransac", "model.image_encoder.img_size": [S, S], "dataset.img_size": [S, S]})
    pipe = Pipeline(args, model=model)
    (optimizer,), (scheduler,) = pipe.configure_optimizers()
    assert isinstance(optimizer, torch.optim.AdamW) and isinstance(scheduler, torch.optim.lr_scheduler.CosineAnnealingLR)
    params = model.get_trainable_parameters()
    assert sum(p.numel() for g_ in optimizer.param_groups for p in g_["params"]) == sum(p.numel() for p in params)
    frozen = [p for p in list(model.vlm.parameters()) + list(model.guidance_backbone.parameters())]
    frozen_before = [p.detach().clone() for p in frozen]
    before = [p.detach().clone() for p in params]

    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    loss, log = pipe.training_step(batch, 0)
    assert set(log) == {"train/mask", "train/pos", "train/neg", "train/loss"} and loss.requires_grad and float(log["train/loss"]) == float(loss)
    assert all(np.isfinite(float(v)) and not v.requires_grad for v in log.values())
    assert set(pipe.train_evaluator.metrics) == {"Anchor IoU", "Query IoU", "Mean IoU", "IoU > .25", "IoU > .5", "IoU > .75"}
    assert all(len(v) == 2 for v in pipe.train_evaluator.metrics.values()) and pipe.train_evaluator.counts == {}
    loss.backward()
    hip = [p.grad.detach().clone() for p in params]
    assert all(p.grad is None for p in frozen)

    # the same step through the torch statement of the loss, with the negatives the HIP forward chose
    results = pipe.last_training["results"]
    neg_idx = torch.stack([results["neg_a"][..., 0] * S + results["neg_a"][..., 1], results["neg_q"][..., 0] * S + results["neg_q"][..., 1]], dim=1).long()
    optimizer.zero_grad(set_to_none=True)
    ref_loss = torch_total_loss(model.forward(batch), batch, pix, neg_idx)
    ref_loss.backward()
    ref = [p.grad.detach().clone() for p in params]
    r = param_ratio(hip, ref)
    print(f"training step: loss {float(loss):.6f} (torch statement {float(ref_loss):.6f}), parameter gradients worst ratio {r:.2e} (bar {R_PARAM:.1e})")
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 and r <= R_PARAM

    for p, gh in zip(params, hip):
        p.grad = gh
    optimizer.step()
    for p, p0 in zip(frozen, frozen_before):
        assert torch.equal(p, p0)
    # AdamW moves a tensor through its gradient or its decay: only one that is zero with a zero gradient stays
    stuck = [i for i, (p, p0, gh) in enumerate(zip(params, before, hip)) if torch.equal(p, p0) and (bool(gh.any()) or bool(p0.any()))]
    assert not stuck, f"trainable tensors {stuck} did not move"
    assert sum(not torch.equal(p, p0) for p, p0 in zip(params, before)) >= 0.9 * len(params)


def test_run_train_driver(tmp_path):
    sys.path.insert(0, ROOT)
    out_dir = tmp_path / "models"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), "--pairs", "4", "--batch", "2", "--epochs", "2", "--out", str(out_dir)],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(out["epochs"]) == 2 and out["checkpoints"][-1] == str(out_dir / "last.ckpt")
    for row in out["epochs"]:
        assert row["batches"] == 2 and all(np.isfinite(row[k]) for k in ("train/mask", "train/pos", "train/neg", "train/loss"))
    print("run_train:", [{k: row[k] for k in ("epoch", "lr", "train/loss")} for row in out["epochs"]])
    import run_test
    import run_train
    from oryon_amd.net import Oryon, default_model_args
    torch.manual_seed(1)
    fresh = Oryon(default_model_args(), DEV, clip_cfg=run_train.small_clip_config())
    blob = torch.load(out_dir / "last.ckpt", map_location="cpu")
    assert set(blob) >= {"state_dict"} and all(k.startswith("model.") for k in blob["state_dict"])
    stats = run_test.load_oryon_checkpoint(fresh, str(out_dir / "last.ckpt"))
    assert stats["missing"] == 0 and stats["unexpected"] == 0
    sd = fresh.state_dict()
    trainable = [k for k in sd if k.startswith(("fusion.", "decoder."))]
    assert len(trainable) >= len(fresh.get_trainable_parameters())
    for k in trainable:
        assert torch.equal(sd[k].cpu(), blob["state_dict"]["model." + k]), k
