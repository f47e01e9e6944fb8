"""GPU tests of mask clean-up (csrc/mask_clean.hip, ops.mask_clean, masks.clean_mask, Pipeline test.mask_clean) against the plain
restatement of its definition (tests/mask_clean_restatement.py).

Bars.  Everything is an integer and the label of a component is the smallest linear index among its pixels - a property of the
partition, not of the schedule: out, labels and stats are compared EXACTLY, on the LDS route and on the global route, and a call's bytes
must not change between runs or streams.  The restatement of a (map, fill) pair is computed once and shared."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_clean_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROUTES = ("lds", "global")
MODES = ("all", "largest", "area")
# (mode, frac, fill_holes): modes 0 and 1 with and without filling, mode 2 at every fraction of R.FRACS with and without
CONFIGS = [(m, 0.25, f) for m in ("all", "largest") for f in (False, True)] + [("area", fr, f) for fr in R.FRACS for f in (False, True)]
CASES = R.cases()
BIG = {}


def big(name):
    """The maps too large to rebuild per test, made on first use."""
    if name not in BIG:
        if name == "cap":                                      # exactly ORYON_MASK_CLEAN_LDS_PIXELS pixels: 256 x 256
            m = R.blobs(256, 256, 7, n=10)
            m[64:192, 100] = 1
            R.ring(m, 10, 10, 120, 120)
            R.ring(m, 130, 130, 250, 250)
        elif name == "above_cap":                              # 272 x 272: route 'auto' must go global
            m = R.blobs(272, 272, 8, n=10)
            R.ring(m, 5, 5, 266, 266)
        elif name == "serpentine_blobs":                       # the longest chains next to random blobs, 224 x 224
            m = R.serpentine(224, 224)
            m[:, 100:140] = 0
            m[R.blobs(224, 224, 9, n=12) == 1] = 1
            m[150:180, 10:90] = 0
            R.ring(m, 152, 12, 178, 88)
        BIG[name] = m
    return BIG[name]


@functools.lru_cache(maxsize=None)
def _restated(name, mode, fq16, fill):
    m = CASES[name] if name in CASES else (R.batch5() if name == "batch5" else big(name))
    return R.clean(m, R.MODES[mode], fq16, fill)


def restated(name, mode, frac, fill):
    return _restated(name, mode, R.frac_q16(frac) if mode == "area" else 0, fill)


def run(mask, mode, frac, fill, route, **kw):
    from oryon_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    return ops.mask_clean(t, mode=mode, frac=frac, fill_holes=fill, route=route, **kw)


def check(name, mask, route, configs=CONFIGS):
    for mode, frac, fill in configs:
        out, labels, stats = (t.cpu().numpy() for t in run(mask, mode, frac, fill, route, want_labels=True, want_stats=True))
        want = restated(name, mode, frac, fill)
        tag = (name, route, mode, frac, fill)
        assert out.dtype == labels.dtype == stats.dtype == np.int32 and out.shape == labels.shape == mask.shape
        assert np.array_equal(stats, want[2]), (tag, stats.tolist(), want[2].tolist())
        assert np.array_equal(labels, want[1]), tag
        assert np.array_equal(out, want[0]), tag


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_equals_the_restatement(name, route):
    check(name, CASES[name], route)


@pytest.mark.parametrize("route", ROUTES)
def test_five_different_maps_in_one_call(route):
    check("batch5", R.batch5(), route)


def test_a_map_of_exactly_the_lds_cap_on_the_lds_route():
    from oryon_amd import ops
    m = big("cap")
    assert m.size == ops.MASK_CLEAN_LDS_PIXELS
    check("cap", m, "lds", [("largest", 0.25, True), ("area", 0.25, False), ("all", 0.25, False)])
    with pytest.raises(Exception, match="ORYON_MASK_CLEAN_LDS_PIXELS|not supported"):
        run(np.zeros((256, 257), np.int32), "largest", 0.25, False, "lds")


def test_a_map_above_the_cap_takes_the_global_route():
    from oryon_amd import ops
    L = ops.lib()
    m = big("above_cap")
    assert m.size > ops.MASK_CLEAN_LDS_PIXELS
    assert L.oryon_mask_clean_workspace_bytes(1, 272, 272, 0) == L.oryon_mask_clean_workspace_bytes(1, 272, 272, 2) > 3 * 4 * m.size
    assert L.oryon_mask_clean_workspace_bytes(1, 256, 256, 0) == L.oryon_mask_clean_workspace_bytes(1, 256, 256, 1) == 256
    check("above_cap", m, "auto", [("largest", 0.25, True), ("area", 0.25, False)])


@pytest.mark.parametrize("route", ROUTES)
def test_serpentine_plus_random_blobs(route):
    check("serpentine_blobs", big("serpentine_blobs"), route, [("largest", 0.25, True), ("area", 0.5, False), ("all", 0.25, True)])


def test_auto_is_the_lds_route_below_the_cap_and_routes_agree():
    m = R.batch5()
    for mode, frac, fill in (("largest", 0.25, True), ("area", 0.5, False)):
        a, b, c = (run(m, mode, frac, fill, r, want_labels=True, want_stats=True) for r in ("auto", "lds", "global"))
        for x, y, z in zip(a, b, c):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() == z.cpu().numpy().tobytes()


@pytest.mark.parametrize("route", ROUTES)
def test_the_same_call_twice_and_on_a_second_stream_gives_identical_bytes(route):
    m = np.stack([big("serpentine_blobs")] * 3)
    m[1] = np.roll(m[1], 5, axis=1)
    first = [t.cpu().numpy().tobytes() for t in run(m, "area", 0.25, True, route, want_labels=True, want_stats=True)]
    again = [t.cpu().numpy().tobytes() for t in run(m, "area", 0.25, True, route, want_labels=True, want_stats=True)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = run(m, "area", 0.25, True, route, want_labels=True, want_stats=True)
    s.synchronize()
    assert first == again == [t.cpu().numpy().tobytes() for t in other]


@pytest.mark.parametrize("route", ROUTES)
def test_labels_and_stats_may_be_null_and_shapes_follow_the_input(route):
    m = CASES["nested_rings"]
    want = restated("nested_rings", "largest", 0.25, True)
    out = run(m, "largest", 0.25, True, route)
    assert isinstance(out, torch.Tensor) and out.shape == m.shape and np.array_equal(out.cpu().numpy(), want[0])
    out, stats = run(m, "largest", 0.25, True, route, want_stats=True)
    assert stats.shape == (6,) and np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(stats.cpu().numpy(), want[2])
    out, labels = run(m[None], "largest", 0.25, True, route, want_labels=True)
    assert labels.shape == (1,) + m.shape and np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(labels[0].cpu().numpy(), want[1])
    src = torch.from_numpy(m).cuda()
    keep = src.clone()
    from oryon_amd import ops
    ops.mask_clean(src, route=route)
    assert torch.equal(src, keep)                              # the input is not written


def test_clean_mask_round_trips_numpy_and_torch():
    from oryon_amd import masks
    m = CASES["w70"]
    want = restated("w70", "largest", 0.25, False)[0]
    got = masks.clean_mask(m)
    assert isinstance(got, np.ndarray) and got.dtype == m.dtype and got.shape == m.shape and np.array_equal(got, want)
    got = masks.clean_mask((m == 1).astype(np.uint8))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    got = masks.clean_mask(m == 1, mode="area", frac=0.5, fill_holes=True)
    assert got.dtype == np.bool_ and np.array_equal(got, restated("w70", "area", 0.5, True)[0].astype(bool))
    t = torch.from_numpy(m).to(torch.int64)
    got = masks.clean_mask(t)
    assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    got = masks.clean_mask(t.cuda().to(torch.uint8)[None].repeat(2, 1, 1), mode="all", fill_holes=True)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (2,) + m.shape
    assert np.array_equal(got[1].cpu().numpy(), restated("w70", "all", 0.25, True)[0])
    with pytest.raises(TypeError):
        masks.clean_mask(m.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ Pipeline
H, C, IDX = 64, 32, (3, 4, 5, 6)


def _island_spot(m):
    """The first 2 x 2 block in raster order whose 4 x 4 surroundings hold no foreground: an island there joins nothing."""
    for y in range(1, m.shape[0] - 2):
        for x in range(1, m.shape[1] - 2):
            if not m[y - 1:y + 3, x - 1:x + 3].any():
                return y, x
    raise AssertionError("no room for an island")


@pytest.fixture(scope="module")
def scene():
    """4 synthetic pairs at 64 x 64, C = 32; the masks with a 2 x 2 island each, and the restatement's clean-up of them."""
    from oryon_amd.synth import make_pair
    pairs = [make_pair(i, H, H, C) for i in IDX]
    st = lambda k: torch.stack([p[k] for p in pairs])
    raw, clean, removed = {}, {}, 0
    for k in ("mask_a", "mask_q"):
        m = st(k).numpy().astype(np.int32).copy()
        for b in range(len(pairs)):
            y, x = _island_spot(m[b])
            m[b, y:y + 2, x:x + 2] = 1
        raw[k] = m
        clean[k], _, stats = R.clean(m, R.MODES["largest"], 0, False)
        removed += int(stats[:, 4].sum())
        assert (stats[:, 4] >= 4).all() and (stats[:, 0] >= 2).all()
    anchor_pose = torch.eye(4).repeat(len(pairs), 1, 1)
    anchor_pose[:, :3, 3] = torch.tensor([0.01, -0.02, 0.8])

    def batch(masks):
        logits = lambda m: (torch.from_numpy(m).float() * 8.0 - 4.0)[:, None].cuda()          # thresholds back to m at 0.5
        return {"featmap_a": st("feat_a").cuda(), "featmap_q": st("feat_q").cuda(), "mask_a": logits(masks["mask_a"]), "mask_q": logits(masks["mask_q"]),
                "anchor": {"mask": torch.from_numpy(masks["mask_a"]).to(torch.uint8), "orig_depth": [p["depth_a"] for p in pairs],
                           "camera": st("camera"), "pose": anchor_pose, "instance_id": [f"s {i} a" for i in IDX]},
                "query": {"mask": torch.from_numpy(masks["mask_q"]).to(torch.uint8), "orig_depth": [p["depth_q"] for p in pairs],
                          "camera": st("camera"), "pose": st("pose").float(), "instance_id": [f"s {i} q" for i in IDX]},
                "instance_id": [f"s {i}" for i in IDX], "cls_id": [1] * len(pairs)}
    return dict(raw=raw, clean=clean, removed=removed, island=batch(raw), cleaned=batch(clean))


def _seed():
    """The per-sample route draws from torch's generator (the matcher's samples) and from numpy's global one (RANSAC's rows)."""
    torch.manual_seed(1)
    np.random.seed(1)


def _pipeline(**test_flags):
    from oryon_amd.pipeline import Pipeline, default_args
    args = default_args(**{"test.solver": "ransac", "model.image_encoder.img_size": [H, H], "dataset.img_size": [H, H]})
    for k, v in test_flags.items():
        setattr(args.test, k, v)
    return Pipeline(args)


def test_batched_step_with_clean_up_equals_the_step_on_cleaned_masks(scene):
    on, off = _pipeline(mask_clean="largest"), _pipeline()
    a, b = on.test_step_batched(scene["island"]), off.test_step_batched(scene["cleaned"])
    assert a["status"].cpu().tolist() == b["status"].cpu().tolist() == [0, 0, 0, 0]
    for k in ("pose", "pred_q", "status"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    res = on.mask_results(scene["island"], on.model.forward(scene["island"]))
    for k in ("a", "q"):
        assert np.array_equal(res[f"mask_{k}_raw"].cpu().numpy(), scene["raw"][f"mask_{k}"])              # still holds the island
        assert np.array_equal(res[f"mask_{k}"].cpu().numpy(), scene["clean"][f"mask_{k}"])
        kept, given = scene["clean"][f"mask_{k}"].sum(axis=(1, 2)), scene["raw"][f"mask_{k}"].sum(axis=(1, 2))
        want_iou = kept.astype(np.float32) / given.astype(np.float32)          # the cleaned mask against the batch's own (with its island)
        assert np.array_equal(a[f"iou_{k}"].cpu().numpy(), want_iou) and (want_iou < 1).all()
    assert sorted(on.last_mask_clean) == ["a", "q"] and all(v.is_cuda and tuple(v.shape) == (4, 6) for v in on.last_mask_clean.values())
    s = on.mask_clean_summary()
    assert s["mask_clean"] == "largest" and s["mask_clean_masks"] == 16                                   # two steps' worth: 2 x (4 + 4)
    assert s["mask_clean_removed_pixels_mean"] * 8 == scene["removed"] and s["mask_clean_filled_pixels_mean"] == 0.0
    assert off.mask_clean_summary() == {} and off.last_mask_clean is None and "mask_a_raw" not in off.mask_results(scene["island"], off.model.forward(scene["island"]))


def test_per_sample_step_with_clean_up_equals_the_step_on_cleaned_masks(scene):
    on, off = _pipeline(mask_clean="largest"), _pipeline()
    _seed()
    a = on.test_step(scene["island"], 0)
    _seed()
    b = off.test_step(scene["cleaned"], 0)
    assert [r["status"] for r in a] == [r["status"] for r in b] == [0, 0, 0, 0]
    for x, y in zip(a, b):
        assert x["pred_pose_rel"].numpy().tobytes() == y["pred_pose_rel"].numpy().tobytes()
    pose_of = lambda lines: [l.split(",")[:3] for l in lines]             # ids and pose; the IoU columns rate each batch's own masks
    assert pose_of(on.pred_lines) == pose_of(off.pred_lines) and len(on.pred_lines) == 4
    s = on.mask_clean_summary()
    assert s["mask_clean_masks"] == 8 and s["mask_clean_removed_pixels_mean"] * 8 == scene["removed"]


def test_external_masks_go_through_the_same_helper(scene):
    on, off = _pipeline(mask="oracle", mask_clean="largest", mask_fill_holes=True), _pipeline(mask="oracle")
    filled = {k: R.clean(scene["raw"][k], R.MODES["largest"], 0, True)[0] for k in ("mask_a", "mask_q")}
    batch = dict(scene["island"])
    ext = dict(batch, anchor=dict(batch["anchor"], mask=torch.from_numpy(filled["mask_a"]).to(torch.uint8)),
               query=dict(batch["query"], mask=torch.from_numpy(filled["mask_q"]).to(torch.uint8)))
    a, b = on.test_step_batched(batch), off.test_step_batched(ext)
    for k in ("pose", "status"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    s = on.mask_clean_summary()
    assert s["mask_clean_masks"] == 8 and s["mask_fill_holes"] is True and s["mask_clean_filled_pixels_mean"] > 0
    _seed()
    ra = on.test_step(batch, 0)
    _seed()
    rb = off.test_step(ext, 0)
    for x, y in zip(ra, rb):
        assert x["status"] == y["status"] and x["pred_pose_rel"].numpy().tobytes() == y["pred_pose_rel"].numpy().tobytes()


def test_run_pose_sets_the_default_and_records_the_flags_and_means(tmp_path, capsys):
    """run_pose.py --mask-clean: the flags become the process-wide default that the pipelines run_test.py builds read, run_test.py's own
    --mask goes through untouched, and the last JSON line carries the flags and the summary's means; without them it is run_test.py's."""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_pose
    from oryon_amd import engine, pipeline
    common = ["--solver", "ransac", "--pairs", "4", "--batch", "2", "--size", "64", "--channels", "32", "--mask", "oracle", "--out", str(tmp_path / "pred.csv")]
    try:
        s = run_pose.main(common + ["--mask-clean", "largest", "--fill-holes"])
        assert pipeline.default_mask_clean() == ("largest", 0.25, True) and s["pairs"] == 4
        assert (s["mask_clean"], s["mask_clean_frac"], s["mask_fill_holes"]) == ("largest", 0.25, True)
        assert s["mask_clean_masks"] >= 8 and s["mask_clean_components_mean"] >= 1.0 and s["mask_clean_kept_components_mean"] == 1.0
        assert s["mask_clean_filled_pixels_mean"] > 0                                  # the synthetic query masks have holes
        last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert last["mask_clean"] == "largest" and last["mask_clean_masks"] == s["mask_clean_masks"]
        s0 = run_pose.main(common)
        assert pipeline.default_mask_clean() == ("none", 0.25, False) and not any(k.startswith("mask_") for k in s0) and s0["pairs"] == 4
    finally:
        pipeline.set_default_mask_clean("none")
        engine.set_default_solver("pointdsc")
