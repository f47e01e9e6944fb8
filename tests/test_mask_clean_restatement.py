"""CPU tests of mask clean-up (h1): the plain restatement of its definition (tests/mask_clean_restatement.py) against outputs written
out by hand and, where scipy imports, against scipy.ndimage.label's partitions on every case; the C ABI of csrc/mask_clean.hip (symbols,
the cap, the workspace size and every argument check, which runs before any HIP call: 0x1000 stands for a non-NULL pointer that is never
dereferenced) and the flags of the layers above.  No GPU is touched."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_clean_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PIXELS = 65536


def A(text):
    """A map drawn with '#' (1), '.' (0) and '2' (a value that is not foreground)."""
    rows = [r.strip() for r in text.strip().splitlines()]
    return np.array([[{"#": 1, ".": 0, "2": 2}[c] for c in r] for r in rows], dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_two_blobs_and_a_pixel_by_hand():
    m = A("""
        ##....
        ##..#.
        ....#.
        .2..#.
        #.....""")
    lab = np.array([[0, 0, -1, -1, -1, -1], [0, 0, -1, -1, 10, -1], [-1, -1, -1, -1, 10, -1], [-1, -1, -1, -1, 10, -1], [24, -1, -1, -1, -1, -1]])
    out, labels, stats = R.clean(m, 0, 0, False)
    assert np.array_equal(out, (m == 1).astype(np.int32)) and np.array_equal(labels, lab) and stats.tolist() == [3, 4, 3, 8, 0, 0]
    out, labels, stats = R.clean(m, 1, 0, False)
    assert np.array_equal(out, (lab == 0).astype(np.int32)) and np.array_equal(labels, lab) and stats.tolist() == [3, 4, 1, 4, 4, 0]
    out, _, stats = R.clean(m, 2, R.frac_q16(0.75), False)                     # 3 * 65536 >= 49152 * 4: exactly on the threshold
    assert np.array_equal(out, ((lab == 0) | (lab == 10)).astype(np.int32)) and stats.tolist() == [3, 4, 2, 7, 1, 0]
    out, _, stats = R.clean(m, 2, R.frac_q16(0.75) + 1, False)
    assert np.array_equal(out, (lab == 0).astype(np.int32)) and stats.tolist() == [3, 4, 1, 4, 4, 0]


def test_a_two_way_area_tie_goes_to_the_smaller_label_by_hand():
    m = A("""
        ....##
        ....##
        ##....
        ##....""")
    out, labels, stats = R.clean(m, 1, 0, False)
    assert np.array_equal(out, A("""
        ....##
        ....##
        ......
        ......""")) and stats.tolist() == [2, 4, 1, 4, 4, 0]
    assert labels[0, 4] == 4 and labels[2, 0] == 12
    out, _, stats = R.clean(m, 2, 65536, False)                                # frac 1: both are as large as the largest
    assert np.array_equal(out, m) and stats.tolist() == [2, 4, 2, 8, 0, 0]


def test_a_diagonal_touch_joins_the_foreground_but_not_the_holes_by_hand():
    m = A("""
        ##...
        ##...
        ..##.
        ..##.""")
    out, labels, stats = R.clean(m, 1, 0, False)
    assert np.array_equal(out, m) and stats.tolist() == [1, 8, 1, 8, 0, 0] and set(labels[m == 1].tolist()) == {0}
    m = A("""
        ######
        #.####
        ##.###
        ###..#
        ######""")                                                             # (1,1), (2,2) and (3,3)-(3,4) touch diagonally only: three holes
    out, labels, stats = R.clean(m, 0, 0, True)
    assert out.all() and stats.tolist() == [1, 30, 1, 30, 0, 4] and (labels == 0).all()
    m[4, 3] = 0                                                                # the last hole opens to the border: it stays, the other two fill
    out, _, stats = R.clean(m, 0, 0, True)
    assert stats.tolist() == [1, 26 + 1, 1, 27, 0, 2] and out[3, 3] == 0 and out[3, 4] == 0 and out[4, 3] == 0 and out[1, 1] == 1 and out[2, 2] == 1


def test_ring_hole_inside_hole_and_island_by_hand():
    m = A("""
        .......
        .#####.
        .#...#.
        .#.#.#.
        .#...#.
        .#####.
        ......2""")
    out, labels, stats = R.clean(m, 1, 0, False)                               # the ring (16) beats the island (1)
    assert stats.tolist() == [2, 16, 1, 16, 1, 0] and out[3, 3] == 0 and labels[3, 3] == 24 and labels[1, 1] == 8
    out, labels, stats = R.clean(m, 1, 0, True)                                # the hole fills: ring, hole and island are one blob
    assert stats.tolist() == [1, 25, 1, 25, 0, 8] and np.array_equal(out[1:6, 1:6], np.ones((5, 5), np.int32)) and out.sum() == 25
    assert (labels[1:6, 1:6] == 8).all() and labels[6, 6] == -1


def test_empty_and_single_row_by_hand():
    out, labels, stats = R.clean(np.zeros((3, 4), np.int32), 1, 0, True)
    assert not out.any() and (labels == -1).all() and stats.tolist() == [0] * 6
    m = A("#.##.###.")
    out, labels, stats = R.clean(m, 1, 0, True)                                # every gap of a single row touches the border
    assert np.array_equal(out, A(".....###.")) and labels.tolist() == [[0, -1, 2, 2, -1, 5, 5, 5, -1]]
    assert stats.tolist() == [3, 3, 1, 3, 3, 0]


def test_frac_q16_is_one_rounding_clamped():
    assert [R.frac_q16(f) for f in (0.0, 0.25, 0.5, 1.0, -1.0, 2.0)] == [0, 16384, 32768, 65536, 0, 65536]
    assert R.frac_q16(0.5 + 1.0 / 65536.0) == 32769
    from oryon_amd import ops
    for f in (0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.5 + 1.0 / 65536.0, 0.999999, 1.0):
        assert ops.mask_clean_frac_q16(f) == R.frac_q16(f)


ALL_MAPS = dict(R.cases(), **{f"batch{i}": m for i, m in enumerate(R.batch5())})


@pytest.mark.parametrize("name", sorted(ALL_MAPS))
def test_partitions_equal_scipys(name):
    ndi = pytest.importorskip("scipy.ndimage")
    m = ALL_MAPS[name]
    fg = m == 1
    for member, nb, structure in ((fg, R.N8, np.ones((3, 3), int)), (~fg, R.N4, [[0, 1, 0], [1, 1, 1], [0, 1, 0]])):
        lab, areas = R.components(member, nb)
        want, n = ndi.label(member, structure=structure)
        assert n == len(areas) and np.array_equal(lab >= 0, member)
        pairs = set(zip(lab[member].tolist(), want[member].tolist()))          # a bijection between the two labellings
        assert len(pairs) == n == len({a for a, _ in pairs}) == len({b for _, b in pairs})
        idx = np.arange(m.size).reshape(m.shape)
        for l, a in areas.items():
            assert a == int((lab == l).sum()) and l == int(idx[lab == l].min())
    filled = ndi.binary_fill_holes(fg, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    assert np.array_equal(R.holes(fg), filled & ~fg)


def test_cases_hold_what_their_names_say():
    c = R.cases()
    st = lambda name, mode=1, f=16384, fill=False: R.clean(c[name], mode, f, fill)[2].tolist()
    assert st("empty") == [0] * 6 and st("full") == [1, 63, 1, 63, 0, 0] and st("single") == [1, 1, 1, 1, 0, 0]
    assert c["row"].shape == (1, 150) and c["column"].shape == (150, 1) and c["w70"].shape == (9, 70) and set(np.unique(c["w70"])) == {-1, 0, 1, 2}
    assert st("diagonal")[0] == 1 and st("diagonal_holes", 0, 0, True)[5] == 8 and st("diagonal_leak", 0, 0, True)[5] == 4
    assert st("checkerboard")[0] == 1 and st("checkerboard", 0, 0, True)[5] == int((c["checkerboard"][1:-1, 1:-1] == 0).sum())
    assert st("u")[0] == 1 and st("serpentine")[:2] == [1, 32 * 64 + 32]
    assert st("ring", 0, 0, True)[5] == 15 and st("ring_at_border", 0, 0, True)[5] == 0 and st("nested_rings")[0] == 4
    assert st("nested_rings", 0, 0, True)[:2] == [1, 19 * 21]
    assert st("tie") == [3, 6, 1, 6, 10, 0] and R.clean(c["tie"], 1, 0, False)[0][1, 1] == 1 and st("tie3") == [3, 4, 1, 4, 8, 0]
    assert R.clean(c["tie3"], 1, 0, False)[0][1, 5] == 1
    kept = [R.clean(c["thresholds"], 2, R.frac_q16(f), False)[2][2] for f in R.FRACS]
    assert kept == [3, 3, 2, 1, 1]


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def Pt(v=0x1000):
    return ctypes.c_void_p(v)


def _lib():
    from oryon_amd import _lib
    return _lib.lib()


def _ok():
    return dict(mask=Pt(), n_maps=2, H=48, W=40, mode=1, frac_q16=16384, fill_holes=1, route=0, out=Pt(0x2000), labels=None, stats=None,
                workspace=Pt(0x3000), workspace_bytes=1 << 30, stream=None)


def _call(**change):
    L = _lib()
    rc = L.oryon_mask_clean(*dict(_ok(), **change).values())
    return rc, L.oryon_last_error().decode()


def test_symbols_header_and_makefile():
    from oryon_amd import _lib, masks, ops
    for name in ("oryon_mask_clean_workspace_bytes", "oryon_mask_clean"):
        assert name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(_lib.lib(), name)
    assert callable(ops.mask_clean) and callable(masks.clean_mask)
    assert ops.MASK_CLEAN_MODES == ("all", "largest", "area") and ops.MASK_CLEAN_STATS == R.STATS and ops.MASK_CLEAN_LDS_PIXELS == LDS_PIXELS
    assert LDS_PIXELS >= 224 * 224
    header = open(os.path.join(ROOT, "include", "oryon_hip.h")).read()
    for line in ("#define ORYON_MASK_CLEAN_STATS 6", f"#define ORYON_MASK_CLEAN_LDS_PIXELS {LDS_PIXELS}",
                 "size_t oryon_mask_clean_workspace_bytes(int n_maps, int H, int W, int route);", "int oryon_mask_clean("):
        assert line in header
    assert "mask_clean.hip" in open(os.path.join(ROOT, "oryon_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("key", ["mask", "out", "workspace"])
def test_null_pointers_are_rejected(key):
    rc, err = _call(**{key: None})
    assert rc == -1 and "oryon_mask_clean: invalid argument" in err and key in err


@pytest.mark.parametrize("change,names", [
    (dict(out=Pt()), "out != mask"),
    (dict(n_maps=-1), "n_maps >= 0"), (dict(n_maps=65536), "n_maps <= 65535"),
    (dict(H=0), "H >= 1"), (dict(W=0), "W >= 1"), (dict(H=1 << 16, W=1 << 15), "H * W"),
    (dict(mode=-1), "mode >= 0"), (dict(mode=3), "mode <= 2"),
    (dict(frac_q16=-1), "frac_q16 >= 0"), (dict(frac_q16=65537), "frac_q16 <= 65536"),
    (dict(route=-1), "route >= 0"), (dict(route=3), "route <= 2"),
    (dict(route=1, H=256, W=257), "ORYON_MASK_CLEAN_LDS_PIXELS"), (dict(route=1, H=1, W=LDS_PIXELS + 1), "ORYON_MASK_CLEAN_LDS_PIXELS"),
    (dict(workspace=Pt(0x3010)), "workspace"),
    (dict(workspace_bytes=0), "workspace_bytes"), (dict(workspace_bytes=16), "workspace_bytes"),
    (dict(route=2, workspace_bytes=3 * 2 * 48 * 40 * 4), "workspace_bytes"),
])
def test_bad_values_are_rejected_with_the_checks_text(change, names):
    rc, err = _call(**change)
    assert rc == -1 and "oryon_mask_clean: invalid argument" in err and names in err, err


def test_nothing_to_do_returns_ok_before_any_launch():
    for change in (dict(), dict(route=1), dict(route=2), dict(H=(1 << 16) - 1, W=1 << 15), dict(route=1, H=256, W=256),
                   dict(mode=0, frac_q16=0, fill_holes=0), dict(mode=2, frac_q16=65536, labels=Pt(0x4000), stats=Pt(0x5000))):
        rc, err = _call(n_maps=0, **change)
        assert rc == 0, (change, err)


def test_workspace_bytes_is_monotone_in_n_maps_and_zero_safe():
    L = _lib()
    a256 = lambda x: (x + 255) // 256 * 256
    for H, W in ((1, 1), (48, 40), (224, 224), (256, 256), (272, 272), (384, 384)):
        for route in (0, 1, 2):
            if route == 1 and H * W > LDS_PIXELS:
                assert L.oryon_mask_clean_workspace_bytes(4, H, W, route) == 0
                continue
            sizes = [L.oryon_mask_clean_workspace_bytes(n, H, W, route) for n in (0, 1, 2, 3, 5, 64, 128, 65535)]
            assert sizes[0] > 0 and all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
            lds = route == 1 or (route == 0 and H * W <= LDS_PIXELS)
            for n, s in zip((0, 1, 2, 3, 5, 64, 128, 65535), sizes):
                m = max(n, 1)
                assert s == a256(64 * m) + (0 if lds else 3 * a256(4 * n * H * W)), (H, W, route, n)
    for args in ((-1, 8, 8, 0), (65536, 8, 8, 0), (1, 0, 8, 0), (1, 8, 0, 0), (1, 1 << 16, 1 << 15, 0), (1, 8, 8, -1), (1, 8, 8, 3)):
        assert L.oryon_mask_clean_workspace_bytes(*args) == 0, args
    o = _ok()
    for route in (0, 2):
        need = L.oryon_mask_clean_workspace_bytes(o["n_maps"], o["H"], o["W"], route)
        rc, err = _call(route=route, workspace_bytes=need - 1)
        assert rc == -1 and "workspace_bytes" in err


def test_python_wrapper_checks_its_arguments_without_a_gpu():
    import torch
    from oryon_amd import ops
    m = torch.zeros(4, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="mode 'biggest'"):
        ops.mask_clean(m, mode="biggest")
    with pytest.raises(ValueError, match="route 'shared'"):
        ops.mask_clean(m, route="shared")
    with pytest.raises(ValueError, match="frac"):
        ops.mask_clean(m, frac=1.5)
    with pytest.raises(ValueError, match="mask is a tensor"):
        ops.mask_clean(torch.zeros(4, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------ flags
def test_pipeline_flags_and_their_process_wide_default():
    from oryon_amd import pipeline
    from oryon_amd.pipeline import Pipeline, default_args
    assert pipeline.MASK_CLEAN_MODES == ("none", "largest", "area") and pipeline.MASK_CLEAN_FRAC == 0.25
    assert pipeline.default_mask_clean() == ("none", 0.25, False)
    t = default_args().test
    assert (t.mask_clean, t.mask_clean_frac, t.mask_fill_holes) == ("none", 0.25, False)
    pl = Pipeline(default_args(**{"test.solver": "ransac"}))
    assert not pl.mask_clean_active() and pl.mask_clean_summary() == {} and pl.last_mask_clean is None
    try:
        pipeline.set_default_mask_clean("area", 0.5, True)
        a = default_args(**{"test.solver": "ransac"})
        assert (a.test.mask_clean, a.test.mask_clean_frac, a.test.mask_fill_holes) == ("area", 0.5, True)
        assert Pipeline(a).mask_clean_cfg() == ("area", 0.5, True)
        del a.test.mask_clean, a.test.mask_clean_frac, a.test.mask_fill_holes          # arg objects without the flags: the default
        assert Pipeline(a).mask_clean_cfg() == ("area", 0.5, True) and Pipeline(a).mask_clean_active()
    finally:
        pipeline.set_default_mask_clean("none")
    assert pipeline.default_mask_clean() == ("none", 0.25, False)
    a = default_args(**{"test.solver": "ransac"})
    del a.test.mask_clean, a.test.mask_clean_frac, a.test.mask_fill_holes
    assert not Pipeline(a).mask_clean_active()
    assert Pipeline(default_args(**{"test.solver": "ransac", "test.mask_fill_holes": True})).mask_clean_active()      # 'none' + fill: mode all
    with pytest.raises(ValueError, match="Mask clean-up biggest not implemented"):
        Pipeline(default_args(**{"test.solver": "ransac", "test.mask_clean": "biggest"}))
    for frac in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="mask_clean_frac"):
            Pipeline(default_args(**{"test.solver": "ransac", "test.mask_clean": "area", "test.mask_clean_frac": frac}))
    with pytest.raises(ValueError):
        pipeline.set_default_mask_clean("largest", 2.0)
    with pytest.raises(ValueError):
        pipeline.set_default_mask_clean("all")
    assert pipeline.default_mask_clean() == ("none", 0.25, False)


def test_mask_clean_summary_of_the_pipeline_and_of_the_process():
    import torch
    from oryon_amd import pipeline
    from oryon_amd.pipeline import Pipeline, default_args
    pipeline.set_default_mask_clean("none")
    assert pipeline.mask_clean_summary() == {}
    Pipeline(default_args(**{"test.solver": "ransac"}))
    assert pipeline.mask_clean_summary() == {}                                          # a pipeline that does not clean leaves no trace
    pl = Pipeline(default_args(**{"test.solver": "ransac", "test.mask_clean": "largest", "test.mask_fill_holes": True}))
    s = pl.mask_clean_summary()
    assert s == pipeline.mask_clean_summary() and s["mask_clean_masks"] == 0 and s["mask_clean_removed_pixels_mean"] is None
    assert (s["mask_clean"], s["mask_clean_frac"], s["mask_fill_holes"]) == ("largest", 0.25, True)
    pl._mask_clean_log.append(torch.tensor([[3, 10, 1, 10, 6, 2], [1, 20, 1, 20, 0, 0]], dtype=torch.int32))      # filled by hand, on the host
    pl._mask_clean_log.append(torch.tensor([[2, 5, 1, 5, 3, 1]], dtype=torch.int32))
    s = pl.mask_clean_summary()
    assert s == pipeline.mask_clean_summary() and s["mask_clean_masks"] == 3
    assert s["mask_clean_components_mean"] == 2.0 and s["mask_clean_removed_pixels_mean"] == 3.0 and s["mask_clean_filled_pixels_mean"] == 1.0
    assert s["mask_clean_kept_pixels_mean"] == 35 / 3 and s["mask_clean_kept_components_mean"] == 1.0
    pipeline.set_default_mask_clean("none")                                             # a driver's new run starts empty
    assert pipeline.mask_clean_summary() == {} and pl.mask_clean_summary() == s


def test_match_pose_config_does_not_carry_the_flags():
    import dataclasses
    from oryon_amd.engine import MatchPoseConfig
    assert not any("mask_clean" in f.name or "fill_holes" in f.name for f in dataclasses.fields(MatchPoseConfig))
    assert not any("mask_clean" in n for n, _ in __import__("oryon_amd._lib", fromlist=["EngineConfig"]).EngineConfig._fields_)


def test_inactive_pipeline_never_calls_mask_clean_and_returns_todays_keys(monkeypatch):
    import torch
    from oryon_amd import ops
    from oryon_amd.pipeline import Pipeline, default_args

    def boom(*a, **k):
        raise AssertionError("ops.mask_clean called with clean-up inactive")
    monkeypatch.setattr(ops, "mask_clean", boom)
    monkeypatch.setattr(ops, "mask_from_logits", lambda logits, th: (torch.sigmoid(logits) > th).to(torch.int32))     # the CPU stand-in
    logits = torch.full((2, 1, 6, 6), -4.0)
    logits[:, :, 1:3, 1:3] = 4.0
    logits[:, :, 5, 5] = 4.0                                                            # an island
    batch = {"anchor": {"mask": (logits[:, 0] > 0).to(torch.uint8)}, "query": {}}
    for args in (default_args(**{"test.solver": "ransac"}), default_args(**{"test.solver": "ransac", "test.mask_clean": "none"})):
        pl = Pipeline(args)
        res = pl.mask_results(batch, {"mask_a": logits, "mask_q": logits})
        assert sorted(res) == ["iou_a", "iou_q", "mask_a", "mask_q"] and int(res["mask_a"].sum()) == 10 and res["iou_a"].tolist() == [1.0, 1.0]
        assert pl.clean_masks(res["mask_a"]) is res["mask_a"] and pl.last_mask_clean is None and pl.mask_clean_summary() == {}
    # active: the helper is the one way in, the thresholded masks stay beside the cleaned ones and the IoU rates the cleaned mask
    calls = []

    def fake(mask, mode, frac, fill_holes, want_stats):
        calls.append((mode, frac, fill_holes, want_stats))
        out = mask.clone()
        out[:, 5, 5] = 0
        return out, torch.tensor([[2, 4, 1, 4, 1, 0]] * mask.shape[0], dtype=torch.int32)
    monkeypatch.setattr(ops, "mask_clean", fake)
    pl = Pipeline(default_args(**{"test.solver": "ransac", "test.mask_fill_holes": True}))
    res = pl.mask_results(batch, {"mask_a": logits, "mask_q": logits})
    assert sorted(res) == ["iou_a", "iou_q", "mask_a", "mask_a_raw", "mask_q", "mask_q_raw"] and calls == [("all", 0.25, True, True)] * 2
    assert int(res["mask_a_raw"].sum()) == 10 and int(res["mask_a"].sum()) == 8 and res["iou_a"].tolist() == pytest.approx([0.8, 0.8])
    assert sorted(pl.last_mask_clean) == ["a", "q"] and pl.mask_clean_summary()["mask_clean_masks"] == 4


def test_run_pose_takes_the_flags_out():
    sys.path.insert(0, ROOT)
    import run_pose
    p = run_pose.parse(["--mask-clean", "area", "--mask-clean-frac", "0.5", "--fill-holes", "--solver", "ransac", "--pairs", "4"])
    assert p == ("ransac", ["--pairs", "4"]) and (p.mask_clean, p.mask_clean_frac, p.mask_fill_holes) == ("area", 0.5, True)
    p = run_pose.parse(["--mask-clean", "largest", "--pairs", "4", "--batch", "2"])
    assert p == ("pointdsc", ["--pairs", "4", "--batch", "2"]) and (p.mask_clean, p.mask_clean_frac, p.mask_fill_holes) == ("largest", 0.25, False)
    p = run_pose.parse([])
    assert (p.mask_clean, p.mask_clean_frac, p.mask_fill_holes) == ("none", 0.25, False) and p.verify == "none" and not p.mutual
    assert tuple(run_pose.Parsed("ransac", ["x"], False)) == ("ransac", ["x"]) and run_pose.Parsed("ransac", [], False).mask_clean == "none"
    p = run_pose.parse(["--mask", "oracle", "--mask-clean", "largest", "--solver", "ransac"])      # run_test.py's --mask is a prefix of the flag
    assert p == ("ransac", ["--mask", "oracle"]) and p.mask_clean == "largest"
    p = run_pose.parse(["--mask=oracle", "--fill-holes"])
    assert p == ("pointdsc", ["--mask=oracle"]) and p.mask_fill_holes and p.mask_clean == "none"
    with pytest.raises(SystemExit):
        run_pose.parse(["--mask-clean", "biggest"])
    with pytest.raises(SystemExit, match="mask-clean-frac"):
        run_pose.main(["--mask-clean", "area", "--mask-clean-frac", "1.5", "--solver", "ransac"])
