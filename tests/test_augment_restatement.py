"""CPU tests of the training augmentations: the numpy statement (tests/augment_restatement.py) against the properties its definition
implies, and the host half of the feature - the draws, the table, the flips of boxes and correspondences in `DeviceCollate` - against
the statement and against a hand-written replay of the reference's call list (utils/augmentations.py:17-127, torchvision ColorJitter)."""
import itertools
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_restatement as st  # noqa: E402

from oryon_amd import augment  # noqa: E402
from oryon_amd.data import DeviceCollate, box_from_mask, make_raw_item, preprocess_item  # noqa: E402


def _image(seed, H=12, W=20):
    return np.random.default_rng(seed).integers(0, 256, size=(3, H, W)).astype(np.float64) / 255.0


def test_unit_factors_return_the_input_exactly():
    x = _image(0)
    for fn_idx in itertools.permutations(range(4)):
        assert np.array_equal(st.colour_jitter(x, fn_idx, (1.0, 1.0, 1.0, None)), x)


def test_hue_third_sends_red_to_green():
    x = np.zeros((3, 2, 2))
    x[0] = 1.0
    y = st.colour_jitter(x, (0, 1, 2, 3), (None, None, None, 1.0 / 3.0))
    assert np.array_equal(y[1], np.ones((2, 2))) and np.array_equal(y[0], np.zeros((2, 2))) and np.array_equal(y[2], np.zeros((2, 2)))
    y64 = st.colour_jitter(x, (0, 1, 2, 3), (None, None, None, 1.0 / 3.0), hue_dtype=np.float64)
    assert np.abs(y64 - y).max() < 1e-12


@pytest.mark.parametrize("f", [-0.5, -0.05, -1e-3, 0.0, 0.02, 0.05, 1.0 / 3.0, 0.5])
def test_gray_pixels_survive_any_hue_factor(f):
    g = np.arange(256, dtype=np.float64).reshape(16, 16) / 255.0
    x = np.stack([g, g, g])
    y = st.colour_jitter(x, (3, 0, 1, 2), (None, None, None, f))
    assert np.array_equal(y, x.astype(np.float32).astype(np.float64))          # the fp32 stage rounds the value once, the hue never enters


def test_hue_stage_costs_about_one_fp32_ulp():
    x = _image(3, 48, 64)
    for f in (-0.05, 0.05):
        d = np.abs(st.adjust_hue(x, f) - st.adjust_hue(x, f, np.float64)).max()
        assert 0 < d < 4e-6, d


def test_double_flip_is_the_identity():
    x = _image(1)
    mask = (np.random.default_rng(2).random((12, 20)) < 0.3)
    box, coords = [3, 4, 5, 6], np.array([[0, 0], [11, 19], [5, 7]])
    for h, v in ((1, 0), (0, 1), (1, 1)):
        assert np.array_equal(st.flip_image(st.flip_image(x, h, v), h, v), x)
        assert np.array_equal(st.flip_image(st.flip_image(mask, h, v), h, v), mask)
        assert st.flip_box(st.flip_box(box, 12, 20, h, v), 12, 20, h, v) == box
        assert np.array_equal(st.flip_coords(st.flip_coords(coords, 12, 20, h, v), 12, 20, h, v), coords)
        # and the package's host functions say the same as the statement
        assert augment.flip_box(torch.tensor(box), (12, 20), h, v).tolist() == st.flip_box(box, 12, 20, h, v)
        assert np.array_equal(augment.flip_coords(torch.tensor(coords), (12, 20), h, v).numpy(), st.flip_coords(coords, 12, 20, h, v))


def test_coords_follow_their_pixels():
    x = np.arange(12 * 20, dtype=np.float64).reshape(1, 12, 20)
    coords = np.array([[0, 0], [11, 19], [5, 7], [3, 19]])
    for h, v in ((1, 0), (0, 1), (1, 1)):
        fx, fc = st.flip_image(x, h, v), st.flip_coords(coords, 12, 20, h, v)
        assert np.array_equal(fx[0, fc[:, 0], fc[:, 1]], x[0, coords[:, 0], coords[:, 1]])


def test_flipped_box_still_bounds_the_flipped_mask():
    """The reference's box is [y1, x1, y2 - y1, x2 - x1] over INCLUSIVE pixel bounds (utils/data/common.py:71-73) and its flip is
    [y, W - w - x, h, w] (utils/augmentations.py:65, 103), where the pixel mirror is W - 1 - x: the flipped box keeps its extent and sits
    one pixel past the box of the flipped mask on the flipped axis.  'Bounds' is therefore checked as the reference's formula gives it:
    same extent, origin exactly one pixel up, i.e. every mask pixel within [origin - 1, origin + extent]."""
    H, W = 12, 20
    mask = np.zeros((H, W), dtype=np.uint8)
    mask[2:7, 5:14] = 1
    mask[4, 3] = 1
    y1, x1, y2, x2 = box_from_mask(mask, 1)
    box = [y1, x1, y2 - y1, x2 - x1]
    for h, v in ((1, 0), (0, 1), (1, 1)):
        fy, fx, fh, fw = st.flip_box(box, H, W, h, v)
        ys, xs = np.nonzero(st.flip_image(mask, h, v))
        assert (fh, fw) == (ys.max() - ys.min(), xs.max() - xs.min())
        assert fy == ys.min() + (1 if v else 0) and fx == xs.min() + (1 if h else 0)
        assert ys.min() >= fy - 1 and ys.max() <= fy + fh and xs.min() >= fx - 1 and xs.max() <= fx + fw


def _augs(jitter, bright, hflip, vflip):
    return SimpleNamespace(rgb=SimpleNamespace(jitter=jitter, bright=bright, hflip=hflip, vflip=vflip))


def _replay(flags):
    """The call list of the reference for one pair, written out: transforms in the order jitter, bright, hflip, vflip; inside one, the
    anchor's gate and draws, then the query's.  Returns what was drawn, as plain tuples."""
    jitter_ranges = ((0.875, 1.125), (0.5, 1.5), (0.5, 1.5), (-0.05, 0.05))
    out = [dict(jitter=None, bright=None, hflip=False, vflip=False) for _ in range(2)]
    if flags[0]:
        for side in out:
            if random.random() < 0.5:
                perm = torch.randperm(4).tolist()
                side["jitter"] = (perm, [float(torch.empty(1).uniform_(lo, hi)) for lo, hi in jitter_ranges])
    if flags[1]:
        for side in out:
            if random.random() < 0.5:
                perm = torch.randperm(4).tolist()
                side["bright"] = (perm, [float(torch.empty(1).uniform_(0.75, 1.25)), None, None, None])
    if flags[2]:
        for side in out:
            if random.random() < 0.5:
                side["hflip"] = True
    if flags[3]:
        for side in out:
            if random.random() < 0.5:
                side["vflip"] = True
    return out


@pytest.mark.parametrize("flags", list(itertools.product((False, True), repeat=4)))
def test_draw_order_is_the_reference_call_list(flags):
    gates_seen = set()
    for seed in range(40):
        random.seed(seed)
        torch.manual_seed(seed)
        want = [_replay(flags) for _ in range(3)]                 # three pairs in a row: the state carries over
        want_state = (random.getstate(), torch.get_rng_state())
        random.seed(seed)
        torch.manual_seed(seed)
        got = [augment.draw_pair_params(_augs(*flags)) for _ in range(3)]
        assert random.getstate() == want_state[0] and torch.equal(torch.get_rng_state(), want_state[1])
        for pair_w, pair_g in zip(want, got):
            for w, g in zip(pair_w, pair_g):
                assert (g.hflip, g.vflip) == (w["hflip"], w["vflip"])
                for name in ("jitter", "bright"):
                    app = getattr(g, name)
                    assert (app is None) == (w[name] is None)
                    if app is not None:
                        assert list(app.fn_idx) == w[name][0] and list(app.factors) == w[name][1]
                gates_seen.add((g.jitter is not None, g.bright is not None, g.hflip, g.vflip))
    assert all((not a or flags[0]) and (not b or flags[1]) and (not c or flags[2]) and (not d or flags[3]) for a, b, c, d in gates_seen)
    assert len(gates_seen) == 2 ** sum(flags)                    # every gate combination the flags allow showed up


def test_factor_ranges():
    random.seed(0)
    torch.manual_seed(0)
    for _ in range(200):
        for p in augment.draw_pair_params(_augs(True, True, False, False)):
            if p.jitter is not None:
                for f, (lo, hi) in zip(p.jitter.factors, ((0.875, 1.125), (0.5, 1.5), (0.5, 1.5), (-0.05, 0.05))):
                    assert lo <= f <= hi
            if p.bright is not None:
                assert 0.75 <= p.bright.factors[0] <= 1.25 and p.bright.factors[1:] == (None, None, None)


def test_table_layout():
    a = augment.AugParams(jitter=augment.ColorApplication((2, 1, 3, 0), (1.1, 0.7, 1.3, -0.02)),
                          bright=augment.ColorApplication((1, 0, 3, 2), (0.8, None, None, None)), hflip=False, vflip=True)
    t = augment.build_table([augment.AugParams(), a, augment.AugParams(hflip=True, vflip=True)])
    assert t.dtype == torch.float64 and tuple(t.shape) == (3, 18)
    assert t[0].tolist() == [0.0, 0.0] + [-1.0, 0.0] * 8
    assert t[1].tolist() == [2.0, 0.0, 2.0, 1.3, 1.0, 0.7, 3.0, -0.02, 0.0, 1.1, 0.0, 0.8] + [-1.0, 0.0] * 3
    assert t[2].tolist() == [3.0, 0.0] + [-1.0, 0.0] * 8
    assert a.ops() == [(2, 1.3), (1, 0.7), (3, -0.02), (0, 1.1), (0, 0.8)]


def test_all_off_means_no_augmentation_and_no_draws():
    for augs in (None, _augs(False, False, False, False), {"rgb": {"jitter": False, "bright": False, "hflip": False, "vflip": False}}):
        c = DeviceCollate(8, (24, 24), "cuda", augs=augs)
        random.seed(5)
        torch.manual_seed(5)
        state = (random.getstate(), torch.get_rng_state())
        assert c.augs is None and c.draw(4) is None
        assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])
    assert DeviceCollate(8, (24, 24), "cuda", augs={"rgb": {"jitter": False, "bright": False, "hflip": True, "vflip": False}}).augs is not None


def test_pipeline_default_args_carry_the_reference_augs():
    from oryon_amd.pipeline import default_args
    assert augment.enabled(default_args().augs) == (True, True, True, True)


def test_collate_host_half_against_the_statement():
    """Boxes and sampled correspondences of DeviceCollate(augs=...) = the statement's flips at sensor resolution, then the plain
    resize bookkeeping (what the collate does without augmentations, on the flipped annotations)."""
    H, W, size = 96, 128, (24, 24)
    items = [preprocess_item(make_raw_item(i, H, W)) for i in range(4)]
    plain = DeviceCollate(8, size, "cuda")
    c = DeviceCollate(8, size, "cuda", augs=_augs(False, False, True, True))
    rng = np.random.default_rng(0)
    corrs = torch.tensor(np.stack([rng.integers(0, H, 8), rng.integers(0, W, 8), rng.integers(0, H, 8), rng.integers(0, W, 8)], axis=1))
    combos = [(False, False), (True, False), (False, True), (True, True)]
    params = [augment.AugParams(hflip=h, vflip=v) for h, v in combos]
    boxes = c.side_boxes(items, params)
    for it, (h, v), box in zip(items, combos, boxes):
        flipped = dict(it, metadata=dict(it["metadata"], boxes=torch.tensor(st.flip_box(it["metadata"]["boxes"].tolist(), H, W, h, v))))
        assert torch.equal(box, plain.side_boxes([flipped])[0])
        y, x, bh, bw = st.flip_box(it["metadata"]["boxes"].tolist(), H, W, h, v)
        assert torch.allclose(box.double(), torch.tensor([y * 24 / H, x * 24 / W, bh * 24 / H, bw * 24 / W]).double(), rtol=1e-6, atol=0)
    assert all(torch.equal(a, b) for a, b in zip(c.side_boxes(items, None), plain.side_boxes(items)))
    for pa, pq in itertools.product(params, params):
        got = c.pair_corrs(items[0], items[1], corrs, (pa, pq))
        fa = st.flip_coords(corrs[:, :2].numpy(), H, W, pa.hflip, pa.vflip)
        fq = st.flip_coords(corrs[:, 2:].numpy(), H, W, pq.hflip, pq.vflip)
        want = plain.pair_corrs(items[0], items[1], torch.tensor(np.concatenate([fa, fq], axis=1)))
        assert torch.equal(got, want)
    assert torch.equal(items[0]["metadata"]["boxes"], preprocess_item(make_raw_item(0, H, W))["metadata"]["boxes"])      # nothing mutated


def test_new_entry_points_validate_without_a_gpu():
    from oryon_amd import _lib
    L = _lib.lib()
    assert L.oryon_rgb_augment_workspace_bytes(3) == 3 * 64 * 8 and L.oryon_rgb_augment_workspace_bytes(0) == 0
    assert L.oryon_rgb_augment_resize(None, None, 0, 4, 4, 2, 2, None, 0, None, None) == 0          # n == 0: nothing to do
    assert L.oryon_rgb_augment_resize(None, None, 1, 4, 4, 2, 2, None, 0, None, None) == -1
    assert b"invalid argument" in L.oryon_last_error()
    assert L.oryon_rgb_augment_resize(8, 8, 1, 4, 4, 2, 2, 8, 0, 8, None) == -3                      # ORYON_ERR_WORKSPACE, no launch
    assert L.oryon_rgb_augment_resize(8, 8, 1, 1 << 15, 1 << 15, 2, 2, 8, 512, 8, None) == -1
    assert L.oryon_resize_bilinear_f32_flip(None, None, 0, 4, 4, 2, 2, 0, None, None) == 0
    assert L.oryon_resize_bilinear_f32_flip(None, None, 1, 4, 4, 2, 2, 0, None, None) == -1
    assert L.oryon_mask_resize_nearest_flip(None, None, 0, 4, 4, 2, 2, None, None) == 0
    assert L.oryon_mask_resize_nearest_flip(8, 12, 1, 4, 4, 2, 2, 8, None) == -1                     # table not 8-byte aligned
