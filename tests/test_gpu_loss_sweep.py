"""GPU sweep of the loss kernels (csrc/feature_loss.hip, csrc/feature_loss_grad.hip) against their float64 statements
(tests/feature_loss_restatement.py, tests/feature_loss_grad_restatement.py) on the seeded cases of tests/loss_sweep_cases.py: the
channel counts, correspondence counts, batch sizes, chain lengths, pool tables and image sizes the recorded fixtures do not reach.
tests/test_loss_sweep_cases.py asserts the cases' premises (near-tie cap of 1 % of a case's rows, what each case is for) on the CPU.
Every case is run at each (pos_margin, neg_margin) of its `runs`, so that both margins have rows on each side.

Forward bars.  neg_idx equal to the restatement's on every row whose float64 top-2 cost gap is >= 1e-5 (in c1, whose costs are exact in
any arithmetic, on EVERY row: the first minimiser); on a near-tied row the kernel's index must name a candidate whose float64 cost is
within 1e-5 of the row's minimum, and d_neg is then evaluated at that index.  Distances, pair terms and batch losses within
BAR = 1e-6.  Invalid pairs exactly 0.  Everything finite, except a (pair, side) whose table names no pixel: NaN, pixel 0 on every row,
and that side's terms count it as 0.

Backward bars, against gr.map_grads called with the forward's own neg_idx, d_pos, d_neg (so the margin tests cannot disagree):
  * the wide R (|want| + S) of tests/test_feature_loss_grad_restatement.py;
  * the derived |got - want| <= max(16, K + 1) 2^-24 S per element, K = the number of slots on the element's pixel: every slot is a
    float64 value rounded once to fp32 (2^-24 of its magnitude, and the magnitudes add up to at most S), and the K slots are added by
    K - 1 fp32 additions of partial sums that never exceed S (1 + K 2^-24): K 2^-24 S to first order, the + 1 carries the second.  For
    K <= 15 this is the existing TIGHT = 16 * 2^-24.  No float64 cancellation floor is added: d(u, u) has no gradient, so the floor
    would be needed only where a negative is its positive's own pixel, and the test asserts that no row of a case is (the own pixel
    carries the full penalty 5e6 and every case has unpenalised candidates); a row without a candidate has no negative term at all;
  * the order of the sum: the restatement's float64 slots rounded to fp32 and added per pixel in ascending slot order reproduce the
    kernel's map; on the elements where the descending order gives another fp32 number, the kernel must hold the ascending one.  The
    kernel's float64 slot and the restatement's differ by a few float64 roundings of the slot's terms (about 2^-50 of them), which
    moves an fp32 rounding with a probability of about 2^-26 per slot: at most one element in a thousand is allowed to differ.
  * untouched elements and invalid pairs exactly 0, the guard tails intact.

What each of these mistakes would fail (reasoned from the code, not run):
  * summing a chain in descending slot order: the order check of n4096 (27 slots on a pixel), smooth (18) and the other noise cases
    (one_pixel cannot: its 300 slots are one number);
  * dropping the `i >= hi` re-scan of feature_loss_grad_scatter_kernel: the owner would follow links no thread of its block wrote;
    one_pixel (chains of 300 over three blocks) and n4096 (a chain with 26 slots past its owner's block) miss both bars;
  * counting V over the first 64 pairs only: b130 (V = 99 of 130, 50 of them among the first 64) is off by a factor of two
    in every gradient, and its batch means need the lane-strided loops' third trip;
  * breaking ties to the higher pool position: c1, where nearly every row is an exact tie of a hundred candidates.

Dice bars: tests/test_gpu_feature_loss.py (sums within 8 n u, n = H W, u = 2^-53, relative to the largest sum; the loss within BAR) and
tests/test_gpu_feature_loss_grad.py (2^-24 |want| + 2^-50 T per element)."""
import numpy as np
import pytest
import torch

import feature_loss_grad_restatement as gr
import feature_loss_restatement as fr
import loss_sweep_cases as sc
from test_feature_loss_grad_restatement import R, worst_ratio
from test_feature_loss_restatement import BAR
from test_gpu_feature_loss_grad import device_inputs, guarded, map_gradients, padded, tail_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = list(sc.CASES)
G_UP = [float(v) for v in np.array([0.7, 0.45, 0.3], dtype=np.float32)]       # the upstream gradient, fp32 numbers
U24 = 2.0 ** -24


def check_forward(tag, case, r, out, pm, nm, every_row=False):
    """out: numpy d_pos, d_neg, neg_idx, pair_terms and optionally losses -> the printed figures."""
    keep = case["valid"] == 1
    empty = np.zeros(r["d_neg"].shape, dtype=bool)
    if "empty" in case:
        empty[case["empty"]] = True
    idx = out["neg_idx"].astype(np.int64)
    assert np.isnan(out["d_neg"][empty]).all() and not idx[empty].any()                    # no candidate: NaN, pixel 0
    assert np.isfinite(out["d_neg"][~empty]).all() and np.isfinite(out["d_pos"]).all() and np.isfinite(out["pair_terms"]).all()
    for k in ("d_pos", "d_neg", "neg_idx", "pair_terms"):
        assert not out[k][~keep].any(), k                                                  # an invalid pair: zeros, exactly
    near = np.zeros(idx.shape, dtype=bool) if every_row else np.nan_to_num(r["gap"], nan=np.inf) < sc.NEAR_TIE
    differ = idx != r["neg_idx"]
    assert not (differ & ~near).any(), f"{int((differ & ~near).sum())} rows with another negative"
    want_d_neg = r["d_neg"].copy()
    excess = 0.0
    for b, side, n in np.argwhere(differ & near):
        assert (sc.candidates(case, b, side) == idx[b, side, n]).sum() == 1                # a candidate of this row's pool
        cost, want_d_neg[b, side, n] = sc.at_pixel(case, b, side, n, idx[b, side, n])
        excess = max(excess, cost - r["low"][b, side, n])
    assert excess <= sc.NEAR_TIE
    pair_terms, losses = fr.terms(r["d_pos"], want_d_neg, case["valid"], pm, nm)
    d = {"d_pos": np.abs(out["d_pos"] - r["d_pos"]).max(), "d_neg": np.abs(out["d_neg"] - want_d_neg)[~empty].max(),
         "pair_terms": np.abs(out["pair_terms"] - pair_terms).max()}
    if "losses" in out:
        assert np.isfinite(out["losses"]).all()
        d["losses"] = np.abs(out["losses"] - losses).max()
    print(tag, f"margins ({pm:.3f}, {nm:.3f}):", {k: f"{v:.2e}" for k, v in d.items()},
          f"near-tied rows {int(near.sum())}, of them with the other negative {int((differ & near).sum())} (cost excess {excess:.1e})")
    assert max(d.values()) <= BAR, d
    return losses


@pytest.mark.parametrize("name", NAMES)
def test_forward_kernel_against_the_restatement(name):
    from oryon_amd import ops
    case, r = sc.reference(name)
    for pm, nm in r["runs"]:
        out = {k: v.cpu().numpy() for k, v in ops.feature_loss(*device_inputs(case, r), pm, nm).items()}
        check_forward(name, case, r, out, pm, nm, every_row=name in sc.TIE_EXEMPT)


def chain_sums(slots, shape, descending=False):
    """The map of one side from the restatement's float64 slots: each rounded once to fp32, then added per pixel in fp32 in slot order."""
    B, C, FH, FW = shape
    out = np.zeros((B, FH * FW, C), dtype=np.float32)
    for (b, (keys, vals)) in slots.items():
        v32, first = vals.astype(np.float32), set()
        for i in (range(len(keys) - 1, -1, -1) if descending else range(len(keys))):
            if keys[i] >= 0:
                out[b, keys[i]] = out[b, keys[i]] + v32[i] if keys[i] in first else v32[i]
                first.add(keys[i])
    return out.transpose(0, 2, 1).reshape(shape)


def check_backward(tag, case, ga, gq, out, pm, nm):
    idx, dp, dn = (out[k].cpu().numpy() for k in ("neg_idx", "d_pos", "d_neg"))
    shape = case["feat_a"].shape
    FH, FW = shape[2:]
    keep = case["valid"] == 1
    own = np.stack([case["pix"][..., 0] * FW + case["pix"][..., 1], case["pix"][..., 2] * FW + case["pix"][..., 3]], axis=1)
    assert not ((idx == own) & np.isfinite(dn))[keep].any()                                # no u = w row: no cancellation floor
    slots = {}
    G, S, active = gr.map_grads(case["feat_a"], case["feat_q"], case["pix"], case["valid"], idx, G_UP, pm, nm, d_pos=dp, d_neg=dn, slots=slots)
    K = sc.slots_per_pixel(case, idx)
    on = gr.touched(case["pix"], case["valid"], idx, (FH, FW))
    for s, got in enumerate((ga.cpu().numpy(), gq.cpu().numpy())):
        want, Ss, Ks = G[s], S[s], K[s][:, None]
        assert np.isfinite(got).all()
        wide = worst_ratio(got, want, Ss)
        bar = np.maximum(16, Ks + 1) * U24 * Ss
        tight = float((np.abs(got - want) / np.maximum(bar, 1e-300)).max())
        side_slots = {b: v for (s_, b), v in slots.items() if s_ == s}
        up, down = chain_sums(side_slots, shape), chain_sums(side_slots, shape, descending=True)
        matters = up != down
        off_order = int((got != up).sum())
        print(tag, "aq"[s], f"margins ({pm:.3f}, {nm:.3f}): ratio {wide:.2e} (bar {R:.1e}), |got - want| / (max(16, K + 1) 2^-24 S) {tight:.2e} (bar 1),",
              f"most slots on one pixel {int(Ks.max())}, largest |gradient| {np.abs(got).max():.3g},",
              f"elements off the ascending fp32 sum {off_order} of {got.size} ({int(matters.sum())} where the order matters,"
              f" {int((got != up)[matters].sum())} of those off)")
        assert wide <= R
        assert (np.abs(got - want) <= bar).all()
        assert off_order <= 1e-3 * got.size and (got != up)[matters].sum() <= 1e-3 * max(int(matters.sum()), 1000)
        assert not got[~np.broadcast_to(on[s][:, None], got.shape)].any()                  # untouched elements: exactly 0
        assert not got[~keep].any()
    return G, S, active


@pytest.mark.parametrize("name", NAMES)
def test_backward_kernels_against_the_restatement(name):
    case, r = sc.reference(name)
    for i, (pm, nm) in enumerate(r["runs"]):
        ga, gq, out = map_gradients(case, r, G_UP, pm, nm)                                 # asserts the guard tails
        _, _, active = check_backward(name, case, ga, gq, out, pm, nm)
        keep = case["valid"] == 1
        if i == 1:
            assert active[keep][:, 1:].any() and not active[keep][:, 1:].all()             # the kernel's own d_neg: rows on both sides
        if name == "n4096" and i == 0:
            ga2, gq2, _ = map_gradients(case, r, G_UP, pm, nm)
            assert ga.cpu().numpy().tobytes() == ga2.cpu().numpy().tobytes() and gq.cpu().numpy().tobytes() == gq2.cpu().numpy().tobytes()
        if name == "pool_table" and i == 0:
            # the (pair, side) without a candidate: neg_margin - NaN > 0 is false, so nothing but the t_pos terms of its positives; and
            # its "negative", pixel 0, holds what a run whose negatives name no pixel at all puts there
            b, s = case["empty"]
            idx = out["neg_idx"].cpu().numpy().astype(np.int64)
            gone = idx.copy()
            gone[b, s] = -1
            dn = out["d_neg"].cpu().numpy()
            G, S, act = gr.map_grads(case["feat_a"], case["feat_q"], case["pix"], case["valid"], gone, [G_UP[0], 0.0, 0.0], pm, nm,
                                     d_pos=out["d_pos"].cpu().numpy(), d_neg=dn)
            got = (ga, gq)[s][b].cpu().numpy()
            assert np.isnan(dn[b, s]).all() and not act[b, 1 + s].any() and np.isfinite(got).all() and np.abs(got).max() > 0
            K = sc.slots_per_pixel(case, gone)[s][b]
            assert (np.abs(got - G[s][b]) <= np.maximum(16, K + 1) * U24 * S[s][b]).all()
            if (case["pix"][b, :, 2 * s:2 * s + 2] != 0).any(1).all():              # no positive of its own on pixel 0
                assert not got[:, 0, 0].any()


def test_argument_edges():
    """Past the documented limits both operators raise before any launch; an empty batch has zero losses."""
    from oryon_amd import _lib, ops
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
    i32 = torch.int32

    def grad(B, C, N):
        return ops.feature_loss_grad(z(B, C, 8, 8), z(B, C, 8, 8), z(B, N, 4, dtype=i32), torch.ones(B, dtype=i32, device=DEV), z(B, 2, N, dtype=i32),
                                     z(B, N), z(B, 2, N), z(3))

    def loss(B, C, N):
        return ops.feature_loss(z(B, C, 8, 8), z(B, C, 8, 8), z(B, N, 4, dtype=i32), torch.ones(B, dtype=i32, device=DEV))

    with pytest.raises(_lib.OryonError):
        grad(1, 4, 4097)
    with pytest.raises(_lib.OryonError):
        grad(1, 257, 8)
    with pytest.raises(_lib.OryonError):
        loss(1, 257, 8)
    out = loss(0, 4, 8)
    torch.cuda.synchronize()
    assert out["losses"].tolist() == [0.0, 0.0, 0.0] and out["d_pos"].shape == (0, 8)
    ga, gq = grad(0, 4, 8)
    assert ga.shape == (0, 4, 8, 8) and gq.shape == (0, 4, 8, 8)
    ga, gq = grad(1, 4, 8)                                                                 # the device is still in order
    torch.cuda.synchronize()
    assert torch.isfinite(ga).all()


@pytest.mark.parametrize("FH,FW", [(40, 50), (23, 87)])
def test_feature_loss_forward_on_both_sides_of_the_pool_switch(FH, FW):
    """FeatureLoss.draw_pool searches the whole map up to FH FW = 2000 (40 x 50) and a draw of 2000 pixels above (23 x 87 = 2001).  The
    table is obtained by calling draw_pool under the forward's seed; the forward's results equal the restatement with that table."""
    from oryon_amd.losses import POOL_SIZE, FeatureLoss
    from oryon_amd.pipeline import Pipeline, default_args
    rng = np.random.default_rng(FH * FW)
    B, C, N, HW = 2, 8, 32, FH * FW
    feat_a, feat_q = sc.noise_maps(rng, B, C, FH, FW)
    corrs = 2 * sc.noise_pix(rng, B, N, FH, FW) + 1                                        # image pixels: the image is twice the map
    valid = np.array([1.0, 0.0], dtype=np.float32)
    logits = {k: (3.0 * rng.standard_normal((B, 1, 24, 24))).astype(np.float32) for k in "aq"}
    gt = {k: rng.integers(0, 2, (B, 2 * FH, 2 * FW)).astype(np.int64) for k in "aq"}
    batch = {"corrs": torch.from_numpy(corrs).long(), "valid": torch.from_numpy(valid),
             "anchor": {"rgb": torch.zeros(B, 3, 2 * FH, 2 * FW), "mask": torch.from_numpy(gt["a"])},
             "query": {"rgb": torch.zeros(B, 3, 2 * FH, 2 * FW), "mask": torch.from_numpy(gt["q"])}}
    outputs = {"featmap_a": torch.from_numpy(feat_a).to(DEV), "featmap_q": torch.from_numpy(feat_q).to(DEV),
               "mask_a": torch.from_numpy(logits["a"]).to(DEV), "mask_q": torch.from_numpy(logits["q"]).to(DEV)}
    args = default_args(**{"test.solver": "ransac"})
    loss = FeatureLoss(args, DEV)

    def seed():
        torch.manual_seed(11)
        torch.cuda.manual_seed(11)

    seed()
    pool, per_positive = loss.draw_pool(outputs["featmap_a"], valid.tolist(), N)
    assert not per_positive
    if HW <= POOL_SIZE:
        assert pool is None
    else:
        assert tuple(pool.shape) == (B, 2, POOL_SIZE) and not pool[1].any()
        assert all(len(set(pool[0, s].tolist())) == POOL_SIZE and 0 <= int(pool[0, s].min()) and int(pool[0, s].max()) < HW for s in (0, 1))
    seed()
    losses, res = loss.forward(batch, outputs)
    after = torch.get_rng_state(), torch.cuda.get_rng_state()
    seed()
    assert Pipeline(args).feature_loss_rng_draws(batch, outputs) == (0 if HW <= POOL_SIZE else 2)
    assert torch.equal(torch.get_rng_state(), after[0]) and torch.equal(torch.cuda.get_rng_state(), after[1])

    pix = fr.feature_pixels(corrs, (2 * FH, 2 * FW), (FH, FW))
    assert pix[..., 1::2].max() == FH - 1 if FW > FH else True                             # the reference's second clamp, by FH - 1
    case = sc.make_case(f"{FH}x{FW}", (feat_a, feat_q), pix, valid=valid.astype(np.int32), pool=None if pool is None else pool.cpu().numpy().astype(np.int64))
    r = sc.restated(case)
    neg = torch.stack([res["neg_a"], res["neg_q"]], dim=1).cpu().numpy().astype(np.int64)
    out = {"d_pos": res["d_pos"].cpu().numpy(), "d_neg": torch.stack([res["d_neg_a"], res["d_neg_q"]], dim=1).cpu().numpy(),
           "neg_idx": neg[..., 0] * FW + neg[..., 1], "pair_terms": res["pair_terms"].cpu().numpy()}
    want = check_forward(case["name"], case, r, out, 0.2, 0.9)
    assert abs(float(losses["pos"]) - want[0]) <= BAR and abs(float(losses["neg"]) - 0.5 * (want[1] + want[2])) <= BAR
    mask = 0.5 * (fr.mask_terms(logits["a"], gt["a"], 0.5)[0] + fr.mask_terms(logits["q"], gt["q"], 0.5)[0])
    assert abs(float(losses["mask"]) - mask) <= BAR


@pytest.mark.parametrize("H,W", sc.DICE_SIZES)
def test_dice_kernels_against_the_restatement(H, W):
    from oryon_amd import ops
    x_host, gt_host = sc.dice_case(H, W)
    n, g = H * W, 0.5
    x, t = padded(torch.from_numpy(x_host), float("nan")), padded(torch.from_numpy(gt_host), 1)
    sums, mask, counts = ops.mask_dice_sums(x, t, 0.5)
    out, buf = guarded(x.shape)
    ops.mask_dice_grad(x, t, padded(sums, float("nan")), padded(torch.tensor([g]), float("nan")), out=out)
    torch.cuda.synchronize()
    assert tail_intact(buf, out.numel())
    with np.errstate(over="ignore"):
        want_sums = fr.dice_sums(x_host, gt_host)
        want_loss, want_mask, want_iou = fr.mask_terms(x_host, gt_host, 0.5)
        want_grad, T = gr.dice_grad(x_host, gt_host, g)
    got_sums, got = sums.cpu().numpy(), out.cpu().numpy()
    rel = float(np.abs(got_sums - want_sums).max() / want_sums.max())
    got_loss = fr.dice_loss(got_sums, n)
    err = np.abs(got - want_grad)
    bar = U24 * np.abs(want_grad) + 2.0 ** -50 * T
    print(f"dice {H} x {W}: sums rel {rel:.2e} (bound {8 * n * 2.0 ** -53:.2e}), loss {got_loss:.9f} vs restatement {want_loss:.9f},",
          f"gradient |got - want| / (2^-24 |want| + 2^-50 T) {float((err / np.maximum(bar, 1e-300)).max()):.2e} (bar 1), largest |gradient| {np.abs(got).max():.3g}")
    assert np.isfinite(got_sums).all() and rel <= 8 * n * 2.0 ** -53 and abs(got_loss - want_loss) <= BAR
    assert got_sums[0, 3] == 0 and got_sums[1, 3] == n                                     # all background, all object
    assert np.isfinite(got).all() and (err <= bar).all()
    assert not got[x_host == -200].any()                                                   # exp(400) = inf: p is exactly 0
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    on, obj = want_mask.reshape(3, -1) != 0, gt_host.reshape(3, -1) != 0
    assert np.array_equal(counts.cpu().numpy(), np.stack([(on & obj).sum(1), (on | obj).sum(1)], axis=1))
    with np.errstate(invalid="ignore"):
        iou = counts[:, 0].float().cpu().numpy() / counts[:, 1].float().cpu().numpy()
    assert np.array_equal(iou, want_iou, equal_nan=True)
