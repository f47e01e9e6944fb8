"""GPU tests of point-to-plane ICP on the depth map (csrc/icp_plane.hip, ops.icp_plane_refine, geo6d.icp_point_to_plane, Pipeline
test.refine = icp_plane) against the numpy restatement of its definition (tests/icp_plane_restatement.py).

Bars.  Pixels (idx), kept-row counts and iteration counts: exact - every case asserts FIRST, on the restatement alone, the margins that
make them independent of rounding (u + .5 and v + .5 from an integer, dist from max_dist, a depth step from normal_jump, |prev - mean|
from the tolerance, a pivot ratio from 1e-12, each >= 1e-9 in its own unit).  T64: 1e-7 absolute, derived, not measured: sums of
<= 8192 float64 terms in any order (<= 1e-12 relative) times cond(A) <= 1e4 (asserted) times |x| <= 0.2 times 20 iterations = 4e-8, with
2.5 x headroom.  mean_err: 3e-7 m, |r| being 1-Lipschitz in the moved points.  Measured gaps: DESIGN.md "Point-to-plane ICP on the
depth map".

A batch shares one map size, so the fixtures' maps (48 x 48, 40 x 56, 56 x 40) are laid into the top-left corner of a 56 x 60 canvas
(depth 0, mask 0 elsewhere: pixel coordinates and intrinsics are unchanged) and the restatement is given the same canvas; the maps'
own shapes run as single-pair calls."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_plane_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

POSE_BAR, MEAN_BAR, MARGIN = 1e-7, 3e-7, 1e-9
CANVAS = (56, 60)
CAP = 320                                   # above every n_s (<= 300): rows beyond the counts hold NaN


def on_canvas(f, HW=CANVAS, **change):
    depth, mask = np.zeros(HW, dtype=np.float32), np.zeros(HW, dtype=np.int32)
    depth[:f["H"], :f["W"]], mask[:f["H"], :f["W"]] = f["depth"], f["mask"]
    return dict(f, depth=depth, mask=mask, **change)


def batch_pairs():
    """The five fixtures, a pair with a failure status between them and a pair whose mask is empty."""
    pairs = [on_canvas(R.fixture(k)) for k in sorted(R.FIXTURES)]
    pairs.insert(2, on_canvas(R.fixture(2), name="failed", status=2))
    pairs.append(on_canvas(R.fixture(3), name="empty_mask"))
    pairs[-1]["mask"] = np.zeros_like(pairs[-1]["mask"])
    return pairs


def pack(pairs, cap=None, dev="cuda"):
    B = len(pairs)
    cap = cap or max(p["src"].shape[0] for p in pairs)
    src = np.full((B, cap, 3), np.nan)
    for b, p in enumerate(pairs):
        src[b, :p["src"].shape[0]] = p["src"]
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    return dict(src=t(src, torch.float64), n_src=t(np.array([p["src"].shape[0] for p in pairs]), torch.int32),
                depth=t(np.stack([p["depth"] for p in pairs]), torch.float32), mask=t(np.stack([p["mask"] for p in pairs]), torch.int32),
                cam9=t(np.stack([p["cam9"] for p in pairs]), torch.float64), T_init=t(np.stack([p["T0"] for p in pairs]), torch.float32),
                status=t(np.array([p.get("status", 0) for p in pairs]), torch.int32))


def run(pk, **kw):
    from oryon_amd import ops
    out = ops.icp_plane_refine(pk["src"], pk["n_src"], pk["depth"], pk["mask"], pk["cam9"], pk["T_init"], status=pk["status"], want_idx=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


_restated = {}


def restate(pairs, max_iter=20, tolerance=1e-5):
    """The restatement of every pair (computed once per configuration and shared), with its margins asserted: the precondition of the
    exact comparisons.  At tolerance 0 the convergence test is false for every float and has no margin."""
    rs = []
    for p in pairs:
        key = (p["name"], p["depth"].shape, max_iter, tolerance)
        if key not in _restated:
            _restated[key] = R.icp_plane(p["src"], p["depth"], p["mask"], p["cam9"], p["T0"], max_iter, tolerance, status_in=p.get("status", 0))
        r = _restated[key]
        for g in ("frac_gap", "dist_gap", "jump_gap", "pivot_gap", "rows_gap") + (("conv_gap",) if tolerance > 0 else ()):
            assert r[g] >= MARGIN or (g == "rows_gap" and r["n_kept"] == 0), (p["name"], g, r[g])
        assert r["cond"] <= 1e4 and all(np.abs(x).max() <= 0.2 for x in r["x_seq"])
        rs.append(r)
    return rs


def compare(out, pairs, rs, what):
    """-> the largest pose gap.  Prints every figure before asserting it."""
    worst = 0.0
    for b, (p, r) in enumerate(zip(pairs, rs)):
        n_s = p["src"].shape[0]
        gap = float(np.abs(out["T64"][b] - r["T"]).max())
        mgap = abs(float(out["mean_err"][b]) - r["mean_err"])
        print(f"{what}[{b}] {p['name']}: n {n_s}, iters {out['iters'][b]} / {r['iters']}, kept {out['n_kept'][b]} / {r['n_kept']}, "
              f"|T64 - restatement| {gap:.2e}, mean_err {r['mean_err']:.3e} off by {mgap:.2e}")
        assert out["iters"][b] == r["iters"] and out["n_kept"][b] == r["n_kept"]
        assert np.array_equal(out["idx"][b, :n_s], r["idx"]) and (out["idx"][b, n_s:] == -1).all()
        assert gap <= POSE_BAR and mgap <= MEAN_BAR
        assert np.array_equal(out["T"][b, :3].view(np.uint32), out["T64"][b].astype(np.float32).view(np.uint32))       # T == float32(T64) bitwise
        assert np.array_equal(out["T"][b, 3], p["T0"][3]) and out["status"][b] == p.get("status", 0)
        worst = max(worst, gap)
    return worst


@pytest.mark.parametrize("max_iter,tolerance", [(20, 1e-5), (20, 0.0), (3, 1e-5)], ids=["tolerance_1e-5", "tolerance_0", "max_iter_3"])
def test_the_fixtures_in_one_batch_beside_pairs_that_do_not_start(max_iter, tolerance):
    pairs = batch_pairs()
    pk = pack(pairs, cap=CAP)
    out = run(pk, max_iter=max_iter, tolerance=tolerance)
    rs = restate(pairs, max_iter, tolerance)
    worst = compare(out, pairs, rs, "batch")
    print(f"batch at max_iter {max_iter}, tolerance {tolerance:g}: |T64 - restatement| <= {worst:.2e}")
    started = [b for b, p in enumerate(pairs) if p["name"] in ("pair1", "pair2", "pair3", "pair4")]
    if tolerance == 0.0:
        assert all(out["iters"][b] == 20 for b in started)
    elif max_iter == 3:
        assert all(out["iters"][b] == 3 for b in started)
    else:
        assert all(2 <= out["iters"][b] < 20 for b in started) and len({int(out["iters"][b]) for b in started}) > 1
        for b in started:                                                  # and the device's own result is the converged pose
            a0, t0 = R.pose_error(pairs[b]["T0"], pairs[b]["T_gt"], pairs[b]["centre"])
            a1, t1 = R.pose_error(out["T64"][b], pairs[b]["T_gt"], pairs[b]["centre"])
            assert a1 <= a0 / 10 and t1 <= t0 / 10
    # pairs that never start: five rows, a failure status.  T_init comes back, nothing ran
    for b, p in enumerate(pairs):
        if p["name"] in ("pair5", "failed"):
            assert np.array_equal(out["T"][b], p["T0"]) and np.array_equal(out["T64"][b], p["T0"][:3].astype(np.float64))
            assert out["iters"][b] == 0 and out["n_kept"][b] == 0 and out["mean_err"][b] == 0.0 and (out["idx"][b] == -1).all()
        if p["name"] == "empty_mask":                                      # starts, keeps no row, ends: T_init as well
            assert np.array_equal(out["T"][b], p["T0"]) and out["iters"][b] == 0 and out["n_kept"][b] == 0 and (out["idx"][b] == -1).all()


@pytest.mark.parametrize("k", [2, 3, 1])
def test_each_map_at_its_own_shape_and_cap_equal_to_n(k):
    """40 x 56 and 56 x 40: a swapped H and W, or a row stride that is not W, shows here.  cap_src = n_s exactly (257: two blocks, the
    second holding one row; 256: one full block)."""
    p = R.fixture(k)
    out = run(pack([p]))
    compare(out, [p], restate([p]), "own shape")


def test_two_maps_of_480_by_640():
    """The size the pipeline runs at, on the inputs of tools/time_icp.py --mode plane: the second pair's map starts 307 200 pixels
    into the buffer (and lies 5 mm further away than the first, so reading the first in its place shows), rows land all over it."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import time_icp
    src, depth, mask, cam9, T0 = (x.numpy() for x in time_icp.plane_inputs(2, 300, "cpu"))
    depth[1] += np.float32(5.0)
    pairs = [dict(name=f"vga{b}", src=src[b], depth=depth[b], mask=mask[b], cam9=cam9[b], T0=T0[b]) for b in range(2)]
    rs = restate(pairs, 6, 0.0)
    assert all(r["iters"] == 6 and r["n_kept"] >= 250 for r in rs) and abs(rs[0]["T"][2, 3] - rs[1]["T"][2, 3]) > 2e-3
    assert max(int(r["idx"].max()) for r in rs) > 300 * 640          # rows below the 300th line of the map
    compare(run(pack(pairs), max_iter=6, tolerance=0.0), pairs, rs, "480x640")


def test_bit_stable_across_runs_streams_and_batch_position():
    from oryon_amd import ops
    pk = pack(batch_pairs(), cap=CAP)
    keys = ("T", "T64", "iters", "mean_err", "n_kept", "idx", "status")
    first = run(pk, tolerance=0.0)
    again = run(pk, tolerance=0.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.icp_plane_refine(pk["src"], pk["n_src"], pk["depth"], pk["mask"], pk["cam9"], pk["T_init"], tolerance=0.0, status=pk["status"],
                                     want_idx=True)
    side.synchronize()
    other = {k: v.cpu().numpy() for k, v in other.items()}
    flipped = run({k: v.flip(0).contiguous() for k, v in pk.items()}, tolerance=0.0)
    for k in keys:
        assert first[k].tobytes() == again[k].tobytes(), k
        assert first[k].tobytes() == other[k].tobytes(), k
        assert first[k].tobytes() == flipped[k][::-1].tobytes(), k


def test_a_ragged_batch_equals_single_pair_calls_byte_for_byte():
    pairs = batch_pairs()
    out = run(pack(pairs, cap=CAP))
    for b, p in enumerate(pairs):
        one = run(pack([p]))                                               # cap_src = the pair's own n_s
        n_s = p["src"].shape[0]
        for k in ("T", "T64", "iters", "mean_err", "n_kept", "status"):
            assert one[k][0].tobytes() == out[k][b].tobytes(), (p["name"], k)
        assert np.array_equal(one["idx"][0], out["idx"][b, :n_s])


def test_geo6d_facade_and_optional_outputs():
    from oryon_amd import geo6d, ops
    p = R.fixture(2)
    K = p["cam9"].reshape(3, 3)
    T = geo6d.icp_point_to_plane(p["src"], p["depth"], p["mask"], K, init_pose=p["T0"])
    r = restate([p])[0]
    assert T.shape == (3, 4) and T.dtype == np.float64 and np.abs(T - r["T"]).max() <= POSE_BAR
    few = geo6d.icp_point_to_plane(p["src"][:5], p["depth"], p["mask"], K, init_pose=p["T0"])
    assert np.array_equal(few, p["T0"][:3].astype(np.float64))
    pk = pack([p])
    out = ops.icp_plane_refine(pk["src"], pk["n_src"], pk["depth"], pk["mask"], pk["cam9"], pk["T_init"])          # no status, no idx
    assert out["idx"] is None and int(out["status"][0]) == 0 and np.abs(out["T64"][0].cpu().numpy() - r["T"]).max() <= POSE_BAR


def test_icp_plane_refine_rejects_tensors_it_would_have_to_convert():
    from oryon_amd import ops
    pk = pack([R.fixture(4)])
    names = ("src", "n_src", "depth", "mask", "cam9", "T_init")
    args = lambda **kw: [dict(pk, **kw)[k] for k in names]
    wide = torch.zeros(1, 64, 6, dtype=torch.float64, device="cuda")
    for change, name in ((dict(src=pk["src"].float()), r"src\.dtype == float64"), (dict(src=wide[:, :, :3]), r"src\.is_contiguous"),
                         (dict(n_src=pk["n_src"].long()), "n_src is"), (dict(depth=pk["depth"].double()), r"depth\.dtype == float32"),
                         (dict(depth=pk["depth"][0]), r"depth\.shape"), (dict(depth=pk["depth"].transpose(1, 2)), r"depth\.is_contiguous"),
                         (dict(mask=pk["mask"].bool()), r"mask\.dtype == int32"), (dict(mask=pk["mask"][:, :-1].contiguous()), r"mask\.shape"),
                         (dict(cam9=pk["cam9"].float()), r"cam9\.dtype == float64"), (dict(cam9=pk["cam9"].reshape(1, 3, 3)), r"cam9\.shape"),
                         (dict(T_init=pk["T_init"].double()), r"T_init\.dtype == float32"), (dict(T_init=pk["T_init"][:, :3]), r"T_init\.shape"),
                         (dict(T_init=pk["T_init"].transpose(1, 2)), r"T_init\.is_contiguous"), (dict(src=pk["src"].cpu()), r"src\.is_cuda"),
                         (dict(depth=pk["depth"][:, :2].contiguous(), mask=pk["mask"][:, :2].contiguous()), "H, W >= 3")):
        with pytest.raises(ValueError, match="icp_plane_refine: " + name):
            ops.icp_plane_refine(*args(**change))
    for kw, name in ((dict(max_iter=0), "max_iter"), (dict(tolerance=-1.0), "tolerance >= 0"), (dict(max_dist=float("nan")), "max_dist >= 0"),
                     (dict(normal_jump=-0.1), "normal_jump >= 0"), (dict(status=pk["status"].long()), "status is")):
        with pytest.raises(ValueError, match="icp_plane_refine: .*" + name):
            ops.icp_plane_refine(*args(), **kw)
    with pytest.raises(ValueError, match="cap_src <= 8192"):
        ops.icp_plane_refine(*args(src=torch.zeros(1, 8193, 3, dtype=torch.float64, device="cuda")))


# ------------------------------------------------------------------------------------------------------------------ Pipeline
def _solver(L=2, C=32):
    from oracle import oryon_oracle as orc
    from oryon_amd.pointdsc import PointDSC
    m = PointDSC(in_dim=6, num_layers=L, num_channels=C, num_iterations=10, ratio=0.1, sigma_d=0.1, k=40, nms_radius=0.1)
    m.load_state_dict(orc.analytic_pointdsc_params(L, C), strict=True)
    return m.cuda().eval()


def _batch(idx, H=48, C=32, dev="cuda"):
    """The synthetic pairs of tests/test_gpu_pipeline.py at its smallest configuration."""
    from oryon_amd.synth import make_pair
    pairs = [make_pair(i, H, H, C) for i in idx]
    B = len(pairs)
    st = lambda k: torch.stack([p[k] for p in pairs])
    anchor_pose = torch.eye(4).repeat(B, 1, 1)
    anchor_pose[:, :3, 3] = torch.tensor([0.01, -0.02, 0.8])
    return {
        "featmap_a": st("feat_a").to(dev), "featmap_q": st("feat_q").to(dev),
        "anchor": {"mask": st("mask_a").to(torch.uint8), "orig_depth": [p["depth_a"] for p in pairs], "camera": st("camera"),
                   "pose": anchor_pose, "instance_id": [f"s {i} a" for i in idx], "sizes": torch.tensor([[H, H]] * B)},
        "query": {"mask": st("mask_q").to(torch.uint8), "orig_depth": [p["depth_q"] for p in pairs], "camera": st("camera"),
                  "pose": st("pose").float(), "instance_id": [f"s {i} q" for i in idx], "sizes": torch.tensor([[H, H]] * B)},
        "instance_id": [f"s {i}" for i in idx], "cls_id": [1] * B,
    }


def _pipeline(H=48, **test_flags):
    from oryon_amd.pipeline import Pipeline, default_args
    args = default_args(**{"test.mask": "oracle", "model.image_encoder.img_size": [H, H], "dataset.img_size": [H, H]})
    for k, v in test_flags.items():
        setattr(args.test, k, v)
    return Pipeline(args, pointdsc_solver=_solver())


def test_refine_icp_plane_per_sample_is_icp_plane_refine_by_hand(monkeypatch):
    """get_pose with test.refine = icp_plane against ops.icp_plane_refine called by hand on the source cloud refine_clouds builds for
    the anchor and a target put together here with torch alone - with the mode's default flags, and with flags of its own."""
    import oryon_amd.pipeline as pipeline_module
    from oryon_amd import ops
    batch = _batch([3, 4])
    base = _pipeline()
    torch.manual_seed(1)
    starts = [r["pred_pose_rel"] for r in base.test_step(batch, 0)]
    for flags, kw in ((dict(), dict(max_iter=20, tolerance=1e-5, max_dist=0.02, normal_jump=0.02)),
                      (dict(refine_max_iter=4, refine_tolerance=0.0, refine_max_dist=0.01, refine_normal_jump=0.012),
                       dict(max_iter=4, tolerance=0.0, max_dist=0.01, normal_jump=0.012))):
        pl = _pipeline(refine="icp_plane", refine_points=512, **flags)
        given = iter([s.double() for s in starts])
        monkeypatch.setattr(pipeline_module, "get_pointdsc_pose", lambda *a, **k: next(given))
        torch.manual_seed(1)
        recs = pl.test_step(batch, 0)
        for b, rec in enumerate(recs):
            assert rec["status"] == 0
            depth_a = batch["anchor"]["orig_depth"][b].squeeze().to("cuda", torch.float32)[None].contiguous()
            depth_q = batch["query"]["orig_depth"][b].squeeze().to("cuda", torch.float32)[None].contiguous()
            cam = batch["query"]["camera"][b:b + 1].cuda()
            c = pl.refine_clouds(batch["anchor"]["mask"][b:b + 1].cuda(), batch["query"]["mask"][b:b + 1].cuda(), depth_a, depth_q,
                                 batch["anchor"]["camera"][b:b + 1].cuda(), cam, torch.tensor([b], dtype=torch.int64, device="cuda"))
            assert int(c["n_src"][0]) == 512                                                           # the subsample took place
            mask = ((batch["query"]["mask"][b:b + 1].cuda() == 1) & (depth_q > 0)).to(torch.int32).contiguous()
            cam9 = cam.to(torch.float32).to(torch.float64).reshape(1, 9).contiguous()
            hand = ops.icp_plane_refine(c["src"], c["n_src"], depth_q, mask, cam9, starts[b][None].cuda().contiguous(), **kw)
            print(f"pair {b} {flags}: iters {int(hand['iters'][0])}, kept {int(hand['n_kept'][0])}, mean |r| {float(hand['mean_err'][0]):.2e}")
            assert int(hand["iters"][0]) >= 1 and rec["refine_iters"] == int(hand["iters"][0])
            assert hand["T"][0].cpu().numpy().tobytes() == rec["pred_pose_rel"].numpy().tobytes()
            assert not torch.equal(rec["pred_pose_rel"], starts[b])
            np.testing.assert_allclose(rec["pred_pose"].numpy(), rec["pred_pose_rel"].numpy() @ batch["anchor"]["pose"][b].numpy(), atol=1e-6)
        if "refine_max_iter" in flags:
            assert all(r["refine_iters"] == 4 for r in recs)


def test_refine_icp_plane_batched_agrees_with_per_sample_and_leaves_failed_pairs_alone(monkeypatch):
    """The batched step against the per-sample loop, both with test.refine = icp_plane, from the SAME solver pose (the per-sample
    loop's solver call is answered with the engine's unrefined pose of the same pair, as tests/test_gpu_icp.py does and for its
    reason: the two routes' matchers draw from different generators): same iteration counts, poses within 1e-6."""
    import oryon_amd.pipeline as pipeline_module
    batch = _batch([3, 4, 5, 6])
    batch["anchor"]["mask"][2] = 0                       # NO_MASK
    pl = _pipeline(refine="icp_plane", refine_points=512)
    out = pl.test_step_batched(batch)
    iters = out["refine_iters"].cpu().tolist()
    assert out["status"].cpu().tolist() == [0, 0, 1, 0]
    assert torch.equal(out["pose"][2].cpu(), torch.eye(4)) and iters[2] == 0 and torch.equal(out["pose_unrefined"][2].cpu(), torch.eye(4))
    starts = iter([out["pose_unrefined"][b].cpu().double() for b in (0, 1, 3)])
    monkeypatch.setattr(pipeline_module, "get_pointdsc_pose", lambda *a, **k: next(starts))
    torch.manual_seed(1)
    recs = pl.test_step(batch, 0)
    assert [r["status"] for r in recs] == [0, 0, 1, 0]
    assert torch.equal(recs[2]["pred_pose_rel"], torch.eye(4)) and "refine_iters" not in recs[2]
    for b in (0, 1, 3):
        gap = float((recs[b]["pred_pose_rel"] - out["pose"][b].cpu()).abs().max())
        print(f"pair {b}, same start: iters per-sample {recs[b]['refine_iters']} / batched {iters[b]}, |pose difference| {gap:.2e}")
        assert recs[b]["refine_iters"] == iters[b] >= 1
        assert gap <= 1e-6
        assert not torch.equal(out["pose"][b], out["pose_unrefined"][b])
    np.testing.assert_allclose(out["pred_q"][0].cpu().numpy(), out["pose"][0].cpu().numpy() @ batch["anchor"]["pose"][0].numpy(), atol=1e-6)


def test_refine_icp_is_untouched_by_the_new_mode():
    """refine_clouds returns what it did: both sides, the anchor's the cloud refine_inputs hands to icp_plane."""
    batch = _batch([3])
    pl_icp, pl_plane = _pipeline(refine="icp", refine_points=512), _pipeline(refine="icp_plane", refine_points=512)
    args = (batch["anchor"]["mask"].cuda(), batch["query"]["mask"].cuda(),
            batch["anchor"]["orig_depth"][0].squeeze().to("cuda", torch.float32)[None].contiguous(),
            batch["query"]["orig_depth"][0].squeeze().to("cuda", torch.float32)[None].contiguous(),
            batch["anchor"]["camera"].cuda(), batch["query"]["camera"].cuda(), torch.tensor([0], dtype=torch.int64, device="cuda"))
    c = pl_icp.refine_clouds(*args)
    assert set(c) == {"src", "dst", "n_src", "n_dst"} and set(pl_icp.refine_inputs(*args)) == set(c)
    t = pl_plane.refine_inputs(*args)
    assert set(t) == {"src", "n_src", "depth", "mask", "cam9"}
    assert torch.equal(t["n_src"], c["n_src"]) and t["src"].cpu().numpy().tobytes() == c["src"].cpu().numpy().tobytes()
    assert t["mask"].dtype == torch.int32 and t["cam9"].dtype == torch.float64 and tuple(t["cam9"].shape) == (1, 9)
    assert min(int(t["mask"].sum()), 512) == int(c["n_dst"][0])                # the same object pixels as the icp mode's target cloud
    assert t["depth"].data_ptr() == args[3].data_ptr()                         # the depth map as it is: no copy
