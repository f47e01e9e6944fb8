"""CPU tests of the training step's ground truth: the float64 restatement of the loss gradients (tests/feature_loss_grad_restatement.py)
against what torch autograd gave the reference's FeatureLoss.forward (tests/golden/flossgrad_*.npz, written by tools/gen_goldens.py
gen_feature_loss_grad) and against torch float64 autograd of a torch statement of the same loss; the new C-ABI symbols on every layer.

The bar.  Per element, the error of a gradient is held against |want| + S, S = the sum of the magnitudes of the terms added into the
element (the restatement returns it): `ratio = |got - want| / (|want| + S)`.  R_REF is the largest ratio of the reference's own fp32
gradients against the float64 restatement over all eight fixtures, measured here (the test prints it per fixture and asserts that the
constant still covers it): 1.29e-3, in fixture 6 (8.5e-4 in fixture 3, 2.8e-4 in fixture 4, 1e-4 .. 2.4e-4 in 1 and 2, 9e-6 in 5).  It is
this large because S is taken after the subtraction v^_k - <u^,v^> u^_k: in a few of the 10^5 elements that difference all but
vanishes for one channel k, and fp32 errs on the scale of v^_k.  The GPU kernels are held to R = 4 R_REF = 5.2e-3 on the same ratio,
against the goldens and against the restatement (the factor the forward's 1e-6 bar was derived with).
Because that bar is wide, the kernel is ALSO held to the restatement alone on a bar that follows from its arithmetic (TIGHT): every
slot is evaluated in float64 and rounded once to fp32 (2^-24 relative), and the m slots of a pixel are added in fp32 (m - 1 additions of
2^-24 relative each); |slot| <= its share of S, so the error is at most m 2^-24 S.  No pixel of a fixture holds more than 8 slots:
TIGHT = 16 * 2^-24 = 9.5e-7, on |got - want| <= TIGHT * S.
Logit gradients: the kernel against the restatement on `ratio` with S = |want| and R.  The reference's recorded fp32 logit gradients
miss that form by 0.25 where the sigmoid saturates (its softmax backward forms p q (a - b) as p (a - (p a + q b))), so the goldens are
compared on the scale T of the four terms without the factor p q (feature_loss_grad_restatement.dice_grad): the reference's own
ratio |golden - want| / (|want| + T) is 3.6e-8 at most, and the same R_REF covers it.
Parameter gradients of one training step (small network): `param_ratio`, the same form with S = the step's largest gradient.
R_PARAM_REF = torch's fp32 autograd against float64 autograd of the same step on the CPU, measured here: 2.17e-4; the GPU step through
the HIP loss is held to R_PARAM = 4 R_PARAM_REF against the same step through the torch statement of the loss."""
import glob
import os

import numpy as np
import pytest
import torch

import feature_loss_grad_restatement as gr
import feature_loss_restatement as fr
from test_feature_loss_restatement import ROOT, load

GRAD_FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "flossgrad_*.npz")))
GRAD_NAMES = [os.path.basename(f)[len("flossgrad_"):-len(".npz")] for f in GRAD_FIXTURES]
R_REF = 1.3e-3
R = 4 * R_REF
TIGHT = 16 * 2.0 ** -24
_cache = {}


def load_grad(name):
    """-> (the forward fixture, the gradient fixture with dense map gradients, the restatement: forward r, G, S, active, logit gradients).
    Computed once, shared, never modified."""
    if name not in _cache:
        z = np.load(GRAD_FIXTURES[GRAD_NAMES.index(name)])
        g = {k: z[k] for k in z.files}
        f = load(os.path.join(ROOT, "tests", "golden", str(g["fixture"]) + ".npz"))
        B, C, FH, FW = f["feat_a"].shape
        for key in "aq":
            dense = np.zeros((B * FH * FW, C), np.float32)
            dense[g["pix_" + key]] = g["vec_" + key]
            g["grad_" + key] = np.ascontiguousarray(dense.reshape(B, FH, FW, C).transpose(0, 3, 1, 2))
        pm, nm = float(g["pos_margin"]), float(g["neg_margin"])
        r = fr.restate(f["feat_a"], f["feat_q"], f["corrs"], f["valid"], f["image_hw"], f["pool"], pm, nm)
        G, S, active = gr.map_grads(f["feat_a"], f["feat_q"], r["pix"], f["valid"], r["neg_idx"], g["g"].astype(np.float64), pm, nm)
        lg, lt = {}, {}
        for key in "aq":
            logits = f["logits_" + key][:, 0]
            lg[key], lt[key] = gr.dice_grad(logits, fr.resize_nearest(f["gt_" + key], logits.shape[1:]), float(g["g_mask"]))
        _cache[name] = (f, g, dict(r=r, G=G, S=S, active=active, logits=lg, logit_terms=lt, on=gr.touched(r["pix"], f["valid"], r["neg_idx"], (FH, FW))))
    return _cache[name]


def worst_ratio(got, want, S):
    return float((np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want) + S, 1e-300)).max())


def torch_losses(feat_a, feat_q, pix, valid, neg_idx, pos_margin=0.2, neg_margin=0.9):
    """The contrastive terms (pos, neg_a, neg_q) as differentiable torch expressions, per pair as the reference computes them
    (losses.py:91-111), with the negatives given: feat_* [B,C,FH,FW] tensors, pix [B,N,4] and neg_idx [B,2,N] long tensors."""
    F = torch.nn.functional
    B, C, FH, FW = feat_a.shape
    terms = []
    for b in range(B):
        if int(valid[b]) != 1:
            continue
        rows = (feat_a[b].reshape(C, -1).T, feat_q[b].reshape(C, -1).T)
        pos = (rows[0][pix[b, :, 0] * FW + pix[b, :, 1]], rows[1][pix[b, :, 2] * FW + pix[b, :, 3]])
        d_pos = 0.5 * (1 - F.cosine_similarity(pos[0], pos[1], dim=1))
        d_neg = [0.5 * (1 - F.cosine_similarity(pos[s], rows[s][neg_idx[b, s]], dim=1)) for s in (0, 1)]
        terms.append(torch.stack([F.relu(d_pos - pos_margin).mean(), F.relu(neg_margin - d_neg[0]).mean(), F.relu(neg_margin - d_neg[1]).mean()]))
    if not terms:
        return torch.zeros(3, dtype=feat_a.dtype, device=feat_a.device)
    return torch.stack(terms).mean(0)


def torch_dice(logits, gt):
    """DiceLoss(weight=[0.5, 0.5]) of logits [B,H,W] against gt [B,H,W] as a differentiable torch expression (dice.py:27-89)."""
    p = torch.sigmoid(2 * logits)
    t = (gt != 0).to(logits.dtype)
    ax = (1, 2)
    fg = 1 - ((p * t).sum(ax) + 1) / ((p * p).sum(ax) + t.sum(ax) + 1)
    bg = 1 - (((1 - p) * (1 - t)).sum(ax) + 1) / (((1 - p) ** 2).sum(ax) + (1 - t).sum(ax) + 1)
    return 0.25 * (fg.mean() + bg.mean())


def test_all_eight_gradient_fixtures_are_present():
    assert GRAD_NAMES == ["1_rescale", "1_rescale_m02", "2_nonsquare", "3_pool", "4_c256", "5_disc", "6_zero_dup_border", "7_none_valid"]
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "floss_*.npz")))
    for p in GRAD_FIXTURES:
        assert os.path.getsize(p) <= largest
        z = np.load(p)
        assert z["vec_a"].dtype == np.float32 and z["grad_logits_a"].dtype == np.float32


def test_gradient_fixtures_pin_what_they_are_for():
    for name in GRAD_NAMES:
        f, g, w = load_grad(name)
        keep = f["valid"] == 1
        if not keep.any():
            assert g["pix_a"].size == 0 and g["pix_q"].size == 0 and not w["G"].any()
            continue
        r = w["r"]
        pm, nm = float(g["pos_margin"]), float(g["neg_margin"])
        assert np.abs(r["d_pos"][keep] - pm).min() >= 1e-5 and np.abs(nm - r["d_neg"][keep]).min() >= 1e-5, name
        act = w["active"][keep]
        assert act[:, 0].any() and not act[:, 0].all(), name                      # active and clamped positive rows
        if name == "1_rescale_m02":
            assert act[:, 1:].any() and not act[:, 1:].all()                     # ... and, here only, clamped negative rows
        else:
            assert act[:, 1:].all()
    f, g, w = load_grad("6_zero_dup_border")
    assert np.abs(g["grad_a"]).max() > 1e5                                        # the zero descriptor at a positive: v^ / eps
    key = w["r"]["pix"][..., 0] * 24 + w["r"]["pix"][..., 1]
    counts = np.bincount(np.concatenate([key[0], w["r"]["neg_idx"][0, 0]]), minlength=576)
    assert counts.max() >= 3                                                      # several slots on one pixel


@pytest.mark.parametrize("name", GRAD_NAMES)
def test_restatement_reproduces_the_reference_gradients(name):
    f, g, w = load_grad(name)
    ratio = {"a": worst_ratio(g["grad_a"], w["G"][0], w["S"][0]), "q": worst_ratio(g["grad_q"], w["G"][1], w["S"][1])}
    for key in "aq":
        ratio["logits_" + key] = worst_ratio(g["grad_logits_" + key], w["logits"][key], w["logit_terms"][key])
    print(name, {k: f"{v:.2e}" for k, v in ratio.items()})
    assert max(ratio.values()) <= R_REF, ratio
    for s in (0, 1):                                                               # nothing outside the touched pixels, on either side
        assert not w["G"][s][~np.broadcast_to(w["on"][s][:, None], w["G"][s].shape)].any()
        assert not g["grad_" + "aq"[s]][~np.broadcast_to(w["on"][s][:, None], w["G"][s].shape)].any()
    for b, v in enumerate(f["valid"]):
        if v != 1:
            assert not w["G"][:, b].any() and not g["grad_a"][b].any() and not g["grad_q"][b].any()


@pytest.mark.parametrize("name", GRAD_NAMES)
def test_restatement_against_float64_autograd(name):
    f, g, w = load_grad(name)
    fa, fq = (torch.from_numpy(f[k]).double().requires_grad_() for k in ("feat_a", "feat_q"))
    pm, nm = float(g["pos_margin"]), float(g["neg_margin"])
    losses = torch_losses(fa, fq, torch.from_numpy(w["r"]["pix"]), f["valid"], torch.from_numpy(w["r"]["neg_idx"]), pm, nm)
    assert np.abs(losses.detach().numpy() - w["r"]["losses"]).max() < 1e-12
    if f["valid"].any():
        (torch.tensor(g["g"], dtype=torch.float64) * losses).sum().backward()
        for s, t in enumerate((fa, fq)):
            ratio = worst_ratio(t.grad.numpy(), w["G"][s], w["S"][s])
            print(name, "aq"[s], f"restatement vs float64 autograd: {ratio:.2e}")
            assert ratio < 1e-9
    for key in "aq":
        x = torch.from_numpy(f["logits_" + key][:, 0]).double().requires_grad_()
        gt = torch.from_numpy(fr.resize_nearest(f["gt_" + key], x.shape[1:]).astype(np.int64))
        (float(g["g_mask"]) * torch_dice(x, gt)).backward()
        assert worst_ratio(x.grad.numpy(), w["logits"][key], np.abs(w["logits"][key])) < 1e-10


def test_per_positive_table_that_names_the_positives_own_pixel():
    """Slots n and N + n on one pixel, u = w: d(u,u) = 0, its gradient vanishes with respect to both; what is left is the positive term."""
    f, g, w = load_grad("1_rescale")
    pix = w["r"]["pix"]
    own = np.stack([pix[..., 0] * 40 + pix[..., 1], pix[..., 2] * 40 + pix[..., 3]], axis=1)
    G, S, active = gr.map_grads(f["feat_a"], f["feat_q"], pix, f["valid"], own, (0.5, 0.25, 0.25))
    G0, _, _ = gr.map_grads(f["feat_a"], f["feat_q"], pix, f["valid"], np.full_like(own, -1), (0.5, 0.25, 0.25))
    assert active[0, 1:].all() and np.abs(G - G0).max() <= 1e-15 * S.max() + 1e-18 and S.max() > 0


def test_new_symbols():
    import re
    from oryon_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "oryon_hip.h")).read()
    L = _lib.lib()
    for name in ("oryon_feature_loss_grad_workspace_bytes", "oryon_feature_loss_grad", "oryon_mask_dice_grad"):
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\s*\(", hdr) and hasattr(L, name)
    assert hasattr(ops, "feature_loss_grad") and hasattr(ops, "mask_dice_grad")
    assert L.oryon_feature_loss_grad_workspace_bytes(32, 32, 500) == 32 * 2 * 32 * 1000 * 4
    assert L.oryon_feature_loss_grad_workspace_bytes(1, 257, 500) == 0 and L.oryon_feature_loss_grad_workspace_bytes(1, 32, 4097) == 0
    assert L.oryon_feature_loss_grad_workspace_bytes(0, 32, 500) == 0

    def rejected(code, why):
        msg = L.oryon_last_error().decode()
        assert code == -1 and why in msg, (code, msg)
    nul = [None] * 5
    rejected(L.oryon_feature_loss_grad(None, None, 1, 257, 8, 8, None, 4, *nul, 0.2, 0.9, None, 0, None, None, None), "exceeds 256 channels")
    rejected(L.oryon_feature_loss_grad(None, None, 1, 32, 8, 8, None, 4097, *nul, 0.2, 0.9, None, 0, None, None, None), "exceeds 4096 correspondences")
    rejected(L.oryon_feature_loss_grad(None, None, 1, 32, 8, 8, None, 4, *nul, 0.2, 0.9, None, 0, None, None, None), "feat_a && feat_q")
    rejected(L.oryon_mask_dice_grad(None, None, 1, 8, 8, None, None, None, None), "logits && gt")


# ---------------------------------------------------------------------------------------------- one training step of a small network
R_PARAM_REF = 2.2e-4       # measured by test_parameter_gradient_bar_fp32_against_float64_autograd: 2.17e-4
R_PARAM = 4 * R_PARAM_REF


def small_training_setup(dev, B, dtype=torch.float32, seed=0):
    """A small Oryon (run_train.small_clip_config: frozen random towers) in train mode and one synthetic training batch of B pairs on
    `dev`; -> (model, batch, pix [B,N,4] long = the correspondences in feature-map pixels)."""
    import sys
    sys.path.insert(0, ROOT)
    import run_test
    import run_train
    from oryon_amd.losses import batch_corrs, featmap_corrs
    from oryon_amd.net import Oryon, default_model_args
    torch.manual_seed(seed)
    model = Oryon(default_model_args(), dev, clip_cfg=run_train.small_clip_config()).to(dtype).train()
    batch = run_train.synthetic_train_batch(run_test, 0, B, dev, 500)
    for side in ("anchor", "query"):
        batch[side]["rgb"] = batch[side]["rgb"].to(dtype)
    S = run_train.SYNTH_SIZE
    pix = featmap_corrs(batch_corrs(batch), (S, S), (S, S))
    return model, batch, pix


def torch_total_loss(outputs, batch, pix, neg_idx, w=(1.0, 0.5, 0.5)):
    """w_mask mask + w_pos pos + w_neg neg of FeatureLoss.forward as differentiable torch expressions, with the negatives given."""
    dev = outputs["featmap_a"].device
    terms = torch_losses(outputs["featmap_a"], outputs["featmap_q"], pix.to(dev), batch["valid"], neg_idx.to(dev))
    mask = 0.5 * (torch_dice(outputs["mask_a"][:, 0], batch["anchor"]["mask"].to(dev)) + torch_dice(outputs["mask_q"][:, 0], batch["query"]["mask"].to(dev)))
    return w[0] * mask + w[1] * terms[0] + w[2] * 0.5 * (terms[1] + terms[2])


def param_ratio(got, want):
    """|got - want| / (|want| + S) over all elements of all parameter gradients, S = the largest |want| of the whole step.  An element
    of a parameter's gradient is a sum over some 10^5 pixels of terms of both signs, carried back through the network in fp32: it
    errs on the scale of the step's large gradients, not on its own - some tensors' gradients vanish identically (a key bias in
    front of a softmax) and hold nothing but rounding noise."""
    scale = max(float(w.abs().max()) for w in want)
    return max(float(((g.double() - w.double()).abs() / (w.double().abs() + scale)).max()) for g, w in zip(got, want))


def test_parameter_gradient_bar_fp32_against_float64_autograd():
    """Measures R_PARAM_REF: torch's fp32 autograd of one training step (small network, B = 1, the torch statement of the loss with given
    negatives) against the same step in float64, on the CPU, in `param_ratio`'s form."""
    grads = {}
    neg = torch.from_numpy(np.random.default_rng(0).integers(0, 192 * 192, (1, 2, 500)))
    for dtype in (torch.float32, torch.float64):
        model, batch, pix = small_training_setup("cpu", 1, dtype)
        loss = torch_total_loss(model.forward(batch), batch, pix, neg)
        loss.backward()
        grads[dtype] = [p.grad.clone() for p in model.get_trainable_parameters()]
        assert all(p.grad is None for p in model.vlm.parameters()) and all(p.grad is None for p in model.guidance_backbone.parameters())
    r = param_ratio(grads[torch.float32], grads[torch.float64])
    print(f"parameter gradients, fp32 against float64 autograd: worst ratio {r:.2e}")
    assert 0 < r <= R_PARAM_REF
