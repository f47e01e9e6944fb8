"""The statements of tests/plumbing_restatement.py against independent references, and the premises of tests/plumbing_cases.py, on the
CPU.  The references: torch's own bilinear (float64) and nearest interpolation, the recorded outputs of the reference project's data
path (g8_data.npz), lift (g2_lift_*.npz) and metrics (g7_metrics.npz), oryon_amd.evaluation's numpy transform, plain python loops."""
import glob
import os

import numpy as np
import pytest
import torch

import plumbing_cases as pc
import plumbing_restatement as pr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_SHAPES = {**pc.RESIZE, **pc.DYADIC}


def _depth(name):
    return pc.dyadic_depth(name) if name in pc.DYADIC else pc.depth_int(name)


@pytest.mark.parametrize("name", list(ALL_SHAPES))
def test_bilinear_statement_against_torch_float64(name):
    """<= 1e-9 absolute on values <= 3000 (measured 2e-11 at 480x640 -> 224x224: the two evaluation orders in float64)."""
    _, out_hw, _, _ = ALL_SHAPES[name]
    x = _depth(name).astype(np.float64)
    assert np.abs(x).max() <= 4096
    ref = torch.nn.functional.interpolate(torch.from_numpy(x)[:, None], size=out_hw, mode="bilinear", align_corners=False)[:, 0].numpy()
    got = pr.bilinear64(x, out_hw)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-9


@pytest.mark.parametrize("name", list(pc.RESIZE))
def test_nearest_statement_against_torch(name):
    _, out_hw, _, _ = pc.RESIZE[name]
    m = pc.masks(name)
    assert set(np.unique(m)) <= {0, 1, 2, 255}
    ref = torch.nn.functional.interpolate(torch.from_numpy(m.astype(np.float32))[:, None], size=out_hw, mode="nearest")[:, 0].numpy()
    got = pr.nearest(m, out_hw)
    assert got.dtype == np.int32 and np.array_equal(got, ref.astype(np.int32))


def test_taps_float32_and_float64_name_the_same_cells_up_to_a_crossing():
    """The float32 tap may sit one cell beside the float64 one only where src is within 3e*in of an integer; then the pair (i0, l1) still
    names a position within 3e*in of the exact one."""
    for name, ((HI, WI), (HO, WO), _, _) in ALL_SHAPES.items():
        for o, i in ((HO, HI), (WO, WI)):
            a0, a1, al0, al1 = pr.taps(o, i, np.float32)
            b0, b1, bl0, bl1 = pr.taps(o, i, np.float64)
            assert al1.dtype == np.float32 and (a1 - a0 == (a0 < i - 1)).all() and (b1 - b0 == (b0 < i - 1)).all()
            assert np.abs((a0 + al1.astype(np.float64)) - (b0 + bl1)).max() <= 3 * pr.U24 * i, name
            assert al0.dtype == np.float32 and (al0 == np.float32(1) - al1).all() and np.abs(bl0 + bl1 - 1).max() <= 2.0 ** -52


def _raw_sides():
    from oryon_amd import data
    g = dict(np.load(os.path.join(GOLD, "g8_data.npz")))
    H, W = (int(v) for v in g["hw"])
    items = [data.preprocess_item(data.make_raw_item(k, H, W)) for k in range(4)]
    return g, {"anchor": items[0::2], "query": items[1::2]}


def test_resize_statements_against_the_recorded_data_path():
    """g8_data.npz (the reference's preprocess / resize / collate at 96x128 -> 56x56): rgb within the 1.2e-7 of the device test, the mask
    equal, the rounded depth within its '<= 1 on < 1 % of the pixels'."""
    g, sides = _raw_sides()
    size = tuple(int(v) for v in g["size"])
    for side, items in sides.items():
        rgb = pr.rgb64(np.stack([it["rgb"].numpy() for it in items]), size).astype(np.float32)
        np.testing.assert_allclose(rgb, g[f"{side}_rgb"], rtol=0, atol=1.2e-7)
        mask = pr.nearest(np.stack([it["mask"].numpy() for it in items]).astype(np.uint8), size)
        np.testing.assert_array_equal(mask, g[f"{side}_mask"])
        d = np.abs(np.rint(pr.bilinear64(np.stack([it["depth"].numpy() for it in items]), size)) - g[f"{side}_depth"])
        assert d.max() <= 1.0 and (d > 0).mean() < 1e-2


def test_rgb_statement_channel_order_and_constants():
    u8 = np.zeros((1, 4, 5, 3), dtype=np.uint8)
    u8[..., 1], u8[..., 2] = 51, 255
    out = pr.rgb64(u8, (7, 3))
    assert out.shape == (1, 3, 7, 3) and (out[0, 0] == 0).all() and np.abs(out[0, 1] - 0.2).max() <= 1e-15 and np.abs(out[0, 2] - 1.0).max() <= 1e-15


@pytest.mark.parametrize("name", list(pc.RESIZE))
def test_rounded_depth_cases_keep_the_near_tie_cap(name):
    """The cap is a condition of the case, from the statement alone: at most 5 % of the pixels within the bar of a rounding tie."""
    _, out_hw, _, _ = pc.RESIZE[name]
    x = pc.depth_int(name)
    assert np.array_equal(x, np.rint(x)) and (x == 0).any() and x.max() < 3000
    want, tol = pr.bilinear64(x, out_hw), pr.depth_bar(x, out_hw)
    share = pc.band(want, tol).mean()
    print(name, f"band share {100 * share:.2f} %, largest bar {tol.max():.3g}")
    assert share <= pc.BAND_CAP
    xf = pc.depth_float(name)
    assert (xf != np.rint(xf)).mean() > 0.9 and len({float(v) for v in xf[:, 0, 0]}) == xf.shape[0]


def test_depth_bar_is_the_stated_window():
    """S_x, S_y and M by plain loops at two small shapes."""
    for (HI, WI), out_hw in (((5, 3), (9, 8)), ((1, 7), (3, 2)), ((6, 1), (4, 5))):
        x = np.random.default_rng(3).uniform(0, 100, size=(2, HI, WI))
        y0, y1, _, _ = pr.taps(out_hw[0], HI)
        x0, x1, _, _ = pr.taps(out_hw[1], WI)
        want = np.zeros((2,) + out_hw)
        for n in range(2):
            for oy in range(out_hw[0]):
                for ox in range(out_hw[1]):
                    rows = range(max(y0[oy] - 1, 0), min(y1[oy] + 1, HI - 1) + 1)
                    cols = range(max(x0[ox] - 1, 0), min(x1[ox] + 1, WI - 1) + 1)
                    sx = max([abs(x[n, r, c + 1] - x[n, r, c]) for r in rows for c in cols if c + 1 in cols] or [0.0])
                    sy = max([abs(x[n, r + 1, c] - x[n, r, c]) for r in rows for c in cols if r + 1 in rows] or [0.0])
                    m = max(abs(x[n, r, c]) for r in (y0[oy], y1[oy]) for c in (x0[ox], x1[ox]))
                    want[n, oy, ox] = 4 * pr.U24 * (WI * sx + HI * sy + m)
        np.testing.assert_allclose(pr.depth_bar(x, out_hw), want, rtol=1e-14)


@pytest.mark.parametrize("name", list(pc.DYADIC))
def test_dyadic_cases_hold_ties_at_even_and_odd(name):
    (HI, WI), out_hw, _, _ = pc.DYADIC[name]
    x = pc.dyadic_depth(name)
    assert np.array_equal(x, np.rint(x)) and x.min() >= 0 and x.max() < 4096
    want = pr.bilinear64(x, out_hw)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)             # every value is a float32 number
    for o, i in zip(out_hw, (HI, WI)):                                                   # and so is every tap, identically
        for a, b in zip(pr.taps(o, i, np.float32), pr.taps(o, i, np.float64)):
            assert np.array_equal(a.astype(np.float64), b)
    tie = want - np.floor(want) == 0.5
    k = np.floor(want[tie]).astype(np.int64)
    print(name, "ties:", int(tie.sum()), "at even k:", int((k % 2 == 0).sum()), "at odd k:", int((k % 2 == 1).sum()))
    assert (k % 2 == 0).sum() >= 3 and (k % 2 == 1).sum() >= 3


def test_compact_statement_and_cases():
    for name, (H, W, _) in pc.COMPACT.items():
        m = pc.compact_masks(name)
        assert m.shape == (5, H, W) and m.dtype == np.int32
        lists = pr.compact(m)
        flat = m.reshape(5, -1)
        assert len(lists[0]) == H * W and len(lists[1]) == 0 and list(lists[2]) == [H * W - 1]
        for i in range(5):
            assert list(lists[i]) == [p for p in range(H * W) if flat[i, p] == 1]
        if H * W > 64:
            assert 0.3 < len(lists[3]) / (H * W) < 0.7 and set(np.unique(m[4])) == {-1, 0, 1, 2, 255}
    assert {h * w for h, w, _ in pc.COMPACT.values()} >= {1, 7, 8, 9, 1147, 8190, 8192, 8193, 8196, 50176}


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "g2_lift_*.npz"))), ids=os.path.basename)
def test_lift_statement_bit_equal_to_the_recorded_lift(path):
    g = np.load(path)
    da, dq = g["depth_a"].astype(np.float32), g["depth_q"].astype(np.float32)
    ca, cq = g["cam_a"].astype(np.float32), g["cam_q"].astype(np.float32)
    pa, pq, keep = pr.lift_pairs(g["corrs"].astype(np.int32), tuple(int(v) for v in g["feat_hw"]), da, dq, ca, cq)
    assert np.array_equal(keep, g["valid"])
    assert pa.dtype == np.float32 and np.array_equal(pa, g["pcd_a"]) and np.array_equal(pq, g["pcd_q"])
    pix = g["pix_a"].astype(np.int64)
    pts = pr.lift_points(da, ca, pix[:, 1], pix[:, 0])
    assert pts.dtype == np.float32 and np.array_equal(pts / np.float32(1000), g["pcd_a"])


@pytest.mark.parametrize("name", list(pc.LIFT))
def test_lift_cases_premises(name):
    grid, cap, kind = pc.LIFT[name]
    (FH, FW), hwa, hwq = pc.LIFT_GRIDS[grid]
    c, want, s = pc.lift_corrs(name), pc.lift_want(name), pc.lift_scene(grid)
    assert c.shape == (pc.LIFT_B, cap, 4) and c.dtype == np.int32
    keep = np.stack([w[2] for w in want])
    inside = (c[..., 0] >= 0) & (c[..., 0] < FH) & (c[..., 2] >= 0) & (c[..., 2] < FH) & (c[..., 1] >= 0) & (c[..., 1] < FW) & \
        (c[..., 3] >= 0) & (c[..., 3] < FW)
    assert np.array_equal(keep, inside)                          # the float32 scale test agrees with the integer one at these grids
    dropped = 1.0 - keep.mean()
    if kind == "mixed":
        assert 0.10 <= dropped <= 0.60, dropped
        if cap >= 4:
            for p in range(pc.LIFT_B):
                assert c[p, 1, 0] == FH and c[p, 2, 3] == FW and c[p, 3, 2] == -1 and not keep[p, 1:4].any()
                assert (c[p] < -1).any() and (c[p][:, 0] > FH).any() | (c[p][:, 1] > FW).any() | (c[p][:, 2] > FH).any() | (c[p][:, 3] > FW).any()
    else:
        assert dropped == 0.0
    if cap >= 4:
        assert keep[:, 0].all() and (c[:, 0] == (FH - 1, FW - 1, FH - 1, FW - 1)).all()
        if grid == "gid":                                        # scale 1: the kept row on the grid's last cell reads the map's last pixel
            assert (FH - 1, FW - 1) == (hwa[0] - 1, hwa[1] - 1)
            z = s["depth_a"][:, -1, -1] / np.float32(1000)
            assert all(want[p][0][0, 2] == z[p] for p in range(pc.LIFT_B))
    assert len({float(v) for v in s["cam_a"][:, 0]}) == pc.LIFT_B and (s["depth_a"][:2] == 0).any() and (s["depth_a"][2:] % 1 != 0).any()
    for n_corr, status in pc.lift_counts(cap):
        assert n_corr.max() <= cap and n_corr.min() >= 0
    assert set(pc.lift_counts(cap)[0][0]) == {cap, cap // 2, min(1, cap), 0} and pc.lift_counts(cap)[1][1][2] != 0


def test_half_transform_bit_equal_to_the_numpy_dot():
    from oryon_amd import evaluation
    pred, gt = pc.pose_pairs()
    pts = pc.model(3000)
    for P in list(pred) + list(gt):
        a = pr.transform_f16(pts, P[:3, :3], P[:3, 3])
        b = evaluation.transform_points_f16(pts, P[:3, :3].astype(np.float64), P[:3, 3].astype(np.float64))
        assert a.dtype == np.float16 and b.dtype == np.float16 and np.array_equal(a, b)


def test_pose_statement_against_the_recorded_metrics():
    """g7_metrics.npz within the bars of test_pose_metrics_on_device_match_reference_golden."""
    from oryon_amd import evaluation
    g = np.load(os.path.join(GOLD, "g7_metrics.npz"))
    pred, gt = g["pred"].astype(np.float32).astype(np.float64), g["gt"].astype(np.float32).astype(np.float64)
    st = np.array([pr.pose_stats(g["pcd"], pred[i], gt[i]) for i in range(pred.shape[0])])
    np.testing.assert_allclose(st[:, 0], g["add"].astype(np.float64), rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(st[:, 1], g["adds"], rtol=1e-5, atol=1e-7)
    theta, shift = evaluation.compute_RT_distances(pred, gt)
    np.testing.assert_allclose(theta, g["theta"], rtol=0, atol=2e-3)
    np.testing.assert_allclose(shift, g["shift"], rtol=1e-5, atol=1e-4)


def test_nearest_distance_against_a_plain_loop():
    r = np.random.default_rng(0)
    a, b = r.normal(size=(300, 3)), r.normal(size=(41, 3))
    want = [min(np.sqrt(((p - q) ** 2).sum()) for q in b) for p in a]
    np.testing.assert_allclose(pr.nearest_distance(a, b, chunk=64), want, rtol=1e-14)


def test_pose_cases_premises():
    pred, gt = pc.pose_pairs()
    theta, shift = pc.rt_want()
    floor = np.arccos(1 - 1e-12) * 180 / np.pi
    i = {k: n for n, k in enumerate(pc.POSE_PAIRS)}
    assert np.array_equal(pred[i["equal"]], gt[i["equal"]]) and theta[i["equal"]] == floor and shift[i["equal"]] == 0.0
    assert 7e-5 < floor < 9e-5
    assert abs(theta[i["small"]] - 2.0) < 1e-3 and abs(shift[i["small"]] - 0.5) < 1e-4
    assert abs(theta[i["deg170"]] - 170.0) < 1e-3
    assert theta[i["deg180"]] == np.arccos(-1 + 1e-12) * 180 / np.pi and np.array_equal(pred[i["deg180"], :3, :3], np.diag([1, -1, -1]))
    assert abs(np.cbrt(np.linalg.det(pred[i["scaled"], :3, :3].astype(np.float64))) - 1.3) < 1e-6 and abs(theta[i["scaled"]] - 10.0) < 1e-3
    assert theta[i["shift"]] == floor and abs(shift[i["shift"]] - 100 * np.sqrt(0.0014)) < 1e-4
    for M in (1, 257):
        w = pc.pose_want(M)
        assert (w[i["equal"]] == 0).all() and (w[1:] > 0).all() and (w[:, 1] <= w[:, 0] * (1 + 2.0 ** -9)).all()      # ADD rounds a - b to half
    assert pc.POSE_M == (1, 255, 256, 257, 1023, 1024, 1025, 2500) and pc.MULTI_SIZES == (2500, 1, 300, 0)
    assert set(pc.MULTI_MODEL_OF_PAIR) == {0, 1, 2, 3}
