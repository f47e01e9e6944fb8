"""GPU tests of the training augmentations (csrc/augment.hip, K-1a): the fused rgb kernel against the numpy statement
tests/augment_restatement.py, the flip forms of the depth and mask resizes against the existing kernels on flipped input (bit for bit),
`DeviceCollate(augs=...)` end to end, and one training step on an augmented batch.

Tolerance of the colour path: with d = the largest difference between the statement as defined (float32 hue stage) and the statement with
a float64 hue stage - computed per case from the statement alone - the kernel may differ from the as-defined statement by at most
max(2^-23, 2 d): one fp32 output ulp at 1.0, or twice what the definition's own float32 hue stage costs against exact arithmetic.
Measured (MI355X): kernel error <= 2.98e-8 in every case (2^-25, the rounding of the fp32 output below 1.0: the colour chain itself agrees
with the statement), d between 0 (no hue op) and 8.2e-7; the largest pair is in DESIGN.md §7b.  Every test prints both per image."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_restatement as st  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(12, 20, 8, 8), (48, 64, 24, 24)]
JITTER = (1.1, 0.7, 1.4, 0.03)


def _params(apps, hflip=False, vflip=False):
    """apps: up to two (fn_idx, factors) applications (jitter, bright)."""
    from oryon_amd.augment import AugParams, ColorApplication
    apps = [None if a is None else ColorApplication(tuple(a[0]), tuple(a[1])) for a in list(apps) + [None, None]][:2]
    return AugParams(jitter=apps[0], bright=apps[1], hflip=hflip, vflip=vflip)


def _apps_of(p):
    return [(a.fn_idx, a.factors) for a in (p.jitter, p.bright) if a is not None]


def _random_images(seed, n, H, W):
    return np.random.default_rng(seed).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)


def _check_against_statement(rgb_u8, params, out_hw, label):
    """oryon_rgb_augment_resize on the batch against the statement, image by image, within max(2^-23, 2 d)."""
    from oryon_amd import augment, ops
    table = augment.build_table(params).to(DEV)
    got = ops.rgb_augment_resize(torch.from_numpy(rgb_u8).to(DEV), table, out_hw).cpu().numpy().astype(np.float64)
    worst = (0.0, 0.0)
    for i, p in enumerate(params):
        want = st.augment_resize(rgb_u8[i], _apps_of(p), p.hflip, p.vflip, out_hw)
        exact = st.augment_resize(rgb_u8[i], _apps_of(p), p.hflip, p.vflip, out_hw, hue_dtype=np.float64)
        d = float(np.abs(want - exact).max())
        err = float(np.abs(got[i] - want).max())
        print(f"{label} image {i}: kernel error {err:.3e}, d {d:.3e}, bound {max(2.0 ** -23, 2 * d):.3e}")
        assert got[i].min() >= 0.0 and got[i].max() <= 1.0
        assert err <= max(2.0 ** -23, 2 * d), (label, i, err, d)
        worst = max(worst, (err, d))
    return worst


COLOUR_CASES = {
    # contrast first, last and absent in the permutation (three different tables in one batch)
    "contrast_position": [_params([((1, 0, 2, 3), JITTER)]), _params([((0, 2, 3, 1), JITTER)], vflip=True),
                          _params([((2, 1, 3, 0), (1.1, None, 1.4, 0.03))], hflip=True)],
    # both applications live, only the second, none
    "applications": [_params([((3, 1, 0, 2), JITTER), ((2, 0, 1, 3), (0.8, None, None, None))], hflip=True, vflip=True),
                     _params([None, ((1, 3, 0, 2), (1.2, None, None, None))]), _params([])],
    # negative and positive hue alone, and a large shift behind a saturation change
    "hue_signs": [_params([((0, 1, 2, 3), (None, None, None, -0.05))]), _params([((0, 1, 2, 3), (None, None, None, 0.05))], hflip=True),
                  _params([((2, 3, 1, 0), (None, None, 0.5, 0.5))])],
    # factors at the ends of their ranges: clamping blends
    "range_ends": [_params([((0, 1, 2, 3), (1.125, 1.5, 1.5, 0.05)), ((0, 1, 2, 3), (1.25, None, None, None))]),
                   _params([((3, 2, 1, 0), (0.875, 0.5, 0.5, -0.05)), ((0, 1, 2, 3), (0.75, None, None, None))], vflip=True),
                   _params([((1, 2, 0, 3), (1.125, 1.5, 0.5, -0.05))])],
}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", sorted(COLOUR_CASES))
def test_colour_chain_against_the_statement(case, shape):
    HI, WI, HO, WO = shape
    _check_against_statement(_random_images(7, 3, HI, WI), COLOUR_CASES[case], (HO, WO), f"{case} {HI}x{WI}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_special_images(shape):
    """An all-gray image, one of saturated primaries and of pixels with r == g == maxc, and a white-heavy one under clamping factors
    (brightness 1.25 on 255), each through the whole chain."""
    HI, WI, HO, WO = shape
    rng = np.random.default_rng(11)
    g = rng.integers(0, 256, size=(HI, WI, 1), dtype=np.uint8)
    gray = np.repeat(g, 3, axis=2)
    palette = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (200, 200, 10), (37, 37, 36),
                        (90, 200, 200), (0, 0, 0), (255, 255, 255)], dtype=np.uint8)
    primaries = palette[rng.integers(0, len(palette), size=(HI, WI))]
    white = np.where(rng.random((HI, WI, 1)) < 0.7, np.uint8(255), rng.integers(0, 256, size=(HI, WI, 3), dtype=np.uint8)).astype(np.uint8)
    rgb = np.stack([gray, primaries, white])
    params = [_params([((3, 0, 1, 2), (1.05, 1.3, 0.6, -0.04))]),
              _params([((2, 3, 0, 1), (0.9, 1.2, 1.5, 0.05))], hflip=True),
              _params([((1, 0, 2, 3), (1.125, 1.5, 1.5, 0.02)), ((0, 1, 2, 3), (1.25, None, None, None))], vflip=True)]
    _check_against_statement(rgb, params, (HO, WO), f"special {HI}x{WI}")
    # a gray image stays gray through any chain
    from oryon_amd import augment, ops
    out = ops.rgb_augment_resize(torch.from_numpy(rgb[:1]).to(DEV), augment.build_table(params[:1]).to(DEV), (HO, WO))
    assert torch.equal(out[0, 0], out[0, 1]) and torch.equal(out[0, 0], out[0, 2])


def test_sensor_resolution():
    """480x640 -> 224x224, n = 2, both applications and both flips."""
    rgb = _random_images(5, 2, 480, 640)
    params = [_params([((2, 1, 3, 0), JITTER), ((0, 1, 2, 3), (0.8, None, None, None))], hflip=True),
              _params([((3, 0, 2, 1), (0.9, 1.4, 0.6, -0.05))], vflip=True)]
    _check_against_statement(rgb, params, (224, 224), "480x640")


@pytest.mark.parametrize("shape", SHAPES + [(480, 640, 224, 224)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_flips_and_identity_bit_for_bit(shape):
    """All-off table = ops.rgb_resize_bilinear; flip-only tables = the existing kernels on torch.flip'd input (rgb, depth with and
    without rounding, mask), a different flip per image."""
    from oryon_amd import augment, ops
    HI, WI, HO, WO = shape
    n = 4
    rng = np.random.default_rng(3)
    rgb = torch.from_numpy(_random_images(9, n, HI, WI)).to(DEV)
    depth = torch.from_numpy((rng.random((n, HI, WI)) * 2000).astype(np.float32)).to(DEV)
    depth_int = depth.round()
    mask = torch.from_numpy((rng.random((n, HI, WI)) < 0.4).astype(np.uint8) * rng.integers(1, 255, (n, HI, WI)).astype(np.uint8)).to(DEV)
    off = augment.build_table([_params([]) for _ in range(n)]).to(DEV)
    assert torch.equal(ops.rgb_augment_resize(rgb, off, (HO, WO)), ops.rgb_resize_bilinear(rgb, (HO, WO)))
    assert torch.equal(ops.resize_bilinear(depth, (HO, WO), flip_table=off), ops.resize_bilinear(depth, (HO, WO)))
    assert torch.equal(ops.mask_resize_nearest(mask, (HO, WO), flip_table=off), ops.mask_resize_nearest(mask, (HO, WO)))
    combos = [(False, False), (True, False), (False, True), (True, True)]
    table = augment.build_table([_params([], hflip=h, vflip=v) for h, v in combos]).to(DEV)

    def flipped(x):                                             # x[i] is [H,W] or [H,W,3]: x is axis 1, y is axis 0
        return torch.stack([torch.flip(x[i], ([1] if h else []) + ([0] if v else [])) for i, (h, v) in enumerate(combos)]).contiguous()
    assert torch.equal(ops.rgb_augment_resize(rgb, table, (HO, WO)), ops.rgb_resize_bilinear(flipped(rgb), (HO, WO)))
    assert torch.equal(ops.resize_bilinear(depth, (HO, WO), flip_table=table), ops.resize_bilinear(flipped(depth), (HO, WO)))
    assert torch.equal(ops.resize_bilinear(depth_int, (HO, WO), round_output=True, flip_table=table),
                       ops.resize_bilinear(flipped(depth_int), (HO, WO), round_output=True))
    assert torch.equal(ops.mask_resize_nearest(mask, (HO, WO), flip_table=table), ops.mask_resize_nearest(flipped(mask), (HO, WO)))


def test_two_runs_are_equal_and_images_are_independent():
    """Bit-stability of the mean reduction, and a table row reaches its own image only: image i of the batch equals the same image and
    row run alone."""
    from oryon_amd import augment, ops
    rgb = torch.from_numpy(_random_images(13, 3, 48, 64)).to(DEV)
    params = COLOUR_CASES["contrast_position"]
    table = augment.build_table(params).to(DEV)
    a = ops.rgb_augment_resize(rgb, table, (24, 24))
    b = ops.rgb_augment_resize(rgb, table, (24, 24))
    assert torch.equal(a, b)
    for i in range(3):
        assert torch.equal(ops.rgb_augment_resize(rgb[i:i + 1], table[i:i + 1].contiguous(), (24, 24))[0], a[i])
    big = torch.from_numpy(_random_images(14, 2, 480, 640)).to(DEV)
    t2 = augment.build_table([params[0], params[1]]).to(DEV)
    assert torch.equal(ops.rgb_augment_resize(big, t2, (224, 224)), ops.rgb_augment_resize(big, t2, (224, 224)))
    assert tuple(ops.rgb_augment_resize(rgb[:0], table[:0].contiguous(), (24, 24)).shape) == (0, 3, 24, 24)


def _tuples(n, size_in=(480, 640), corr_n=500):
    from oryon_amd import data
    H, W = size_in
    rng = np.random.default_rng(21)
    out = []
    for i in range(n):
        ia, iq = data.preprocess_item(data.make_raw_item(30 + i, H, W)), data.preprocess_item(data.make_raw_item(40 + i, H, W))
        c = torch.from_numpy(np.stack([rng.integers(0, H, corr_n), rng.integers(0, W, corr_n), rng.integers(0, H, corr_n),
                                       rng.integers(0, W, corr_n)], axis=1))
        out.append((ia, iq, ["mug"], c, c, np.eye(4), "mug", f"p{i}", True))
    return out


def test_device_collate_with_all_augmentations_and_one_training_step():
    """480x640 tuples through DeviceCollate(augs = all four): rgb within the bound of the statement run with the drawn parameters, mask and
    correspondences exact, depth bit-equal to flip-then-existing-kernel, orig_depth untouched; the plain collate's bytes with augs off;
    then Pipeline.training_step of a small Oryon on the augmented batch: finite loss, finite gradients."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_train
    from oryon_amd import data, ops
    from oryon_amd.net import Oryon, default_model_args
    from oryon_amd.pipeline import Pipeline, default_args
    S = run_train.SYNTH_SIZE
    H, W, B = 480, 640, 3
    tuples = _tuples(B)
    args = default_args(**{"test.solver": "ransac", "model.image_encoder.img_size": [S, S], "dataset.img_size": [S, S]})
    collate = data.DeviceCollate(500, (S, S), DEV, augs=args.augs)
    seed = 4
    random.seed(seed)
    torch.manual_seed(seed)
    params = collate.draw(B)                                    # what the call below draws, replayed from the same seed
    assert any(not p.identity for pair in params for p in pair) and any(p.hflip or p.vflip for pair in params for p in pair)
    random.seed(seed)
    torch.manual_seed(seed)
    batch = collate(tuples)
    plain = data.DeviceCollate(500, (S, S), DEV)(tuples)
    for s, side in enumerate(("anchor", "query")):
        b, items = batch[side], [t[s] for t in tuples]
        got = b["rgb"].cpu().numpy().astype(np.float64)
        for i, pair in enumerate(params):
            p = pair[s]
            want = st.augment_resize(items[i]["rgb"].numpy(), _apps_of(p), p.hflip, p.vflip, (S, S))
            exact = st.augment_resize(items[i]["rgb"].numpy(), _apps_of(p), p.hflip, p.vflip, (S, S), hue_dtype=np.float64)
            d, err = float(np.abs(want - exact).max()), float(np.abs(got[i] - want).max())
            print(f"collate {side} {i}: kernel error {err:.3e}, d {d:.3e}")
            assert err <= max(2.0 ** -23, 2 * d)
            m = torch.from_numpy(st.flip_image(items[i]["mask"].numpy(), p.hflip, p.vflip)).to(torch.uint8).to(DEV)
            assert torch.equal(b["mask"][i], ops.mask_resize_nearest(m, (S, S))[0].to(torch.uint8))
            dflip = torch.from_numpy(st.flip_image(items[i]["depth"].numpy(), p.hflip, p.vflip)).to(torch.float32).to(DEV)
            assert torch.equal(b["depth"][i], ops.resize_bilinear(dflip[None], (S, S), round_output=True)[0])
            assert torch.equal(b["orig_depth"][i].cpu(), items[i]["depth"].to(torch.float32)) and b["orig_rgb"][i] is items[i]["orig_rgb"]
            fb = st.flip_box(items[i]["metadata"]["boxes"].tolist(), H, W, p.hflip, p.vflip)
            assert torch.allclose(b["box"][i].double(), torch.tensor([fb[0] * S / H, fb[1] * S / W, fb[2] * S / H, fb[3] * S / W]).double(), rtol=1e-6)
            cols = slice(0, 2) if s == 0 else slice(2, 4)
            fc = st.flip_coords(tuples[i][3][:, cols].numpy(), H, W, p.hflip, p.vflip)
            _, want_c = data.resize_annotations(items[i], torch.from_numpy(fc), (S, S))
            assert torch.equal(batch["corrs"][i][:, cols], want_c.to(torch.long))
        assert torch.equal(b["camera"], plain[side]["camera"]) and torch.equal(b["sizes"], plain[side]["sizes"])
    off = data.DeviceCollate(500, (S, S), DEV, augs={"rgb": dict(jitter=False, bright=False, hflip=False, vflip=False)})(tuples)
    for side in ("anchor", "query"):
        for k in ("rgb", "mask", "depth", "box"):
            assert torch.equal(off[side][k], plain[side][k])
    assert torch.equal(off["corrs"], plain["corrs"])

    torch.manual_seed(0)
    model = Oryon(default_model_args(), DEV, clip_cfg=run_train.small_clip_config()).train()
    batch["prompt_tokens"] = run_train.synthetic_prompt_tokens(B)
    pipe = Pipeline(args, model=model)
    loss, log = pipe.training_step(batch, 0)
    loss.backward()
    assert np.isfinite(float(loss.detach())) and all(np.isfinite(float(v)) for v in log.values())
    grads = [p.grad for p in model.get_trainable_parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)


def test_run_train_real_asset_mode_with_augmentations(tmp_path):
    """run_train.py --data-root ... --augs all on the fabricated NOCS tree of test_datasets.py (random-init weights, hashed prompts): two
    epochs of one batch train with finite losses; the synthetic mode refuses to augment."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_train
    from test_datasets import make_nocs_tree
    make_nocs_tree(str(tmp_path), n_pairs=2)
    s = run_train.main(["--data-root", str(tmp_path), "--dataset", "nocs", "--split", "cross_scene_test", "--mask", "oracle", "--batch", "2",
                        "--pairs", "2", "--epochs", "2", "--hash-prompts", "--augs", "all", "--out", str(tmp_path / "models")])
    assert len(s["epochs"]) == 2
    for row in s["epochs"]:
        assert row["batches"] == 1 and all(np.isfinite(row[k]) for k in ("train/mask", "train/pos", "train/neg", "train/loss"))
    with pytest.raises(SystemExit, match="synthetic mode"):
        run_train.main(["--pairs", "2", "--augs", "hflip"])
