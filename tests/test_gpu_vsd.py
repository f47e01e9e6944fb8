"""The VSD kernels (csrc/vsd.hip) on the device: the rasteriser against its numpy statement bit for bit, batching and streams, the
counts against what the reference's vsd computed (tests/golden/g11_vsd.npz), and evaluate_batch(device='cuda') with compute_vsd
against the reference's Evaluator(compute_vsd=True)."""
import numpy as np
import pytest
import torch

from oryon_amd import evaluation as ev
from tests import vsd_fixture as vf

pytestmark = pytest.mark.gpu

MESHES = ("ico2", "box", "twopart")


def _view_pose(i):
    """A closed-form pose (millimetres) that shows the object at about 0.4 m, tilted, a little off-centre."""
    c, s = np.cos(0.4 + 0.3 * i), np.sin(0.4 + 0.3 * i)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) @ np.array([[1.0, 0.0, 0.0], [0.0, 0.8, -0.6], [0.0, 0.6, 0.8]])
    P = np.eye(4, dtype=np.float32)
    P[:3, :3], P[:3, 3] = R, (3.0 - 2.0 * i, -2.0 + i, 400.0 + 25.0 * i)
    return P


def _render(P, K, o, H, W, **kw):
    from oryon_amd import ops
    return ops.render_depth(torch.from_numpy(P)[None].cuda(), torch.from_numpy(K)[None].cuda(), torch.from_numpy(o["pts"]),
                            torch.from_numpy(o["faces"]), H, W, **kw)


def _expected_routes(P, K, o, H, W):
    """(triangles drawn one wave each, triangles drawn one thread each) by the documented rule: a triangle that draws at all goes to
    its set-up thread when its clipped pixel box is at most 8 x 8, else to the queue.  For poses in front of the camera."""
    f32 = np.float32
    P, Kc, v = np.asarray(P, f32), np.asarray(K, f32), o["pts"].astype(f32)
    X, Y, Z = (((P[k, 0] * v[:, 0] + P[k, 1] * v[:, 1]) + P[k, 2] * v[:, 2]) + P[k, 3] for k in range(3))
    sx = np.rint((Kc[0, 0] * (X / Z) + Kc[0, 2]) * f32(256)).astype(np.int64)
    sy = np.rint((Kc[1, 1] * (Y / Z) + Kc[1, 2]) * f32(256)).astype(np.int64)
    large = small = 0
    for a, b, c in o["faces"]:
        xs, ys = sx[[a, b, c]], sy[[a, b, c]]
        if (xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0]) == 0:
            continue
        cmin, cmax = max((xs.min() + 127) >> 8, 0), min((xs.max() - 128) >> 8, W - 1)
        rmin, rmax = max((ys.min() + 127) >> 8, 0), min((ys.max() - 128) >> 8, H - 1)
        if cmin <= cmax and rmin <= rmax:
            if cmax - cmin < 8 and rmax - rmin < 8:
                small += 1
            else:
                large += 1
    return large, small


def _assert_same_image(dev, ref):
    """coverage and the fp32 depth, bit for bit"""
    dev = dev.cpu().numpy()
    assert np.array_equal(dev > 0, ref > 0), f"coverage differs at {int(((dev > 0) != (ref > 0)).sum())} pixels"
    assert np.array_equal(dev.view(np.uint32), ref.view(np.uint32)), \
        f"{int((dev != ref).sum())} depths differ, max |d| {np.abs(dev - ref).max():.3e} mm"


@pytest.mark.parametrize("hw", [(48, 64), (60, 80)])
@pytest.mark.parametrize("name", MESHES)
def test_render_equals_numpy_statement(name, hw):
    H, W = hw
    o, K, P = vf.objects()[name], vf.small_camera(H, W), _view_pose(MESHES.index(name))
    ref = ev.rasterize_depth(P, K, o["pts"], o["faces"], H, W)
    assert (ref > 0).sum() > 100
    depth, (large, small) = _render(P, K, o, H, W, return_route_counts=True)
    _assert_same_image(depth[0], ref)
    # the work distribution: pixel-sized triangles are drawn by their set-up thread, the box's faces by one wave each, and the
    # plate-and-post mesh uses both routes (the post's end caps are a few pixels across)
    assert (large, small) == _expected_routes(P, K, o, H, W)
    if name == "ico2":
        assert large == 0 and small > 100
    if name == "box":
        assert small == 0 and 1 <= large <= 12
    if name == "twopart":
        assert large >= 12 and small >= 1 and large + small <= 24


def test_render_equals_numpy_statement_640x480():
    g, o = vf.golden(), vf.objects()["ico3"]
    P = vf.pose_mm(g["gt"][1])
    depth, (large, small) = _render(P, g["K"], o, 480, 640, return_route_counts=True)
    _assert_same_image(depth[0], ev.rasterize_depth(P, g["K"], o["pts"], o["faces"], 480, 640))
    assert large == 0 and small > 1000 and (large, small) == _expected_routes(P, g["K"], o, 480, 640)     # the thread route at full size
    r0, c0 = g["crop_gt_1_origin"]
    assert np.array_equal(depth[0, r0:r0 + 48, c0:c0 + 64].cpu().numpy(), g["crop_gt_1"])


def _batch():
    objs, H, W = vf.objects(), 60, 80
    names = ["ico2", "box", "twopart"]
    verts = torch.from_numpy(np.concatenate([objs[k]["pts"] for k in names]))
    faces = torch.from_numpy(np.concatenate([objs[k]["faces"] for k in names]))
    vo = torch.tensor(np.concatenate(([0], np.cumsum([objs[k]["pts"].shape[0] for k in names]))), dtype=torch.int32)
    fo = torch.tensor(np.concatenate(([0], np.cumsum([objs[k]["faces"].shape[0] for k in names]))), dtype=torch.int32)
    which = [0, 2, 1, 0, 2]
    P = np.stack([_view_pose(i) for i in range(5)])
    P[3, 2, 3] = -400.0                                        # behind the camera
    K = np.stack([vf.small_camera(H, W) + np.array([[2.0 * i, 0, 0.5 * i], [0, 3.0 * i, -0.25 * i], [0, 0, 0]]) for i in range(5)])
    return objs, names, verts, faces, vo, fo, which, P, K, H, W


def test_batch_of_mixed_models_equals_single_calls():
    from oryon_amd import ops
    objs, names, verts, faces, vo, fo, which, P, K, H, W = _batch()
    out = ops.render_depth(torch.from_numpy(P).cuda(), torch.from_numpy(K).cuda(), verts, faces, H, W, vert_offset=vo, face_offset=fo,
                           model_of_image=torch.tensor(which, dtype=torch.int32))
    assert out.shape == (5, H, W)
    for i in range(5):
        single = _render(P[i], K[i], objs[names[which[i]]], H, W)
        assert torch.equal(out[i], single[0]), i
        _assert_same_image(out[i], ev.rasterize_depth(P[i], K[i], objs[names[which[i]]]["pts"], objs[names[which[i]]]["faces"], H, W))
    assert int((out[3] != 0).sum()) == 0 and int((out[0] > 0).sum()) > 100


def test_two_streams_give_identical_images():
    from oryon_amd import ops
    objs, names, verts, faces, vo, fo, which, P, K, H, W = _batch()
    args = (torch.from_numpy(P).cuda(), torch.from_numpy(K).cuda(), verts.cuda(), faces.cuda(), H, W)
    kw = dict(vert_offset=vo, face_offset=fo, model_of_image=torch.tensor(which, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = ops.render_depth(*args, **kw)
    with torch.cuda.stream(s2):
        b = ops.render_depth(*args, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and int((a > 0).sum()) > 100


def test_vsd_counts_equal_reference_at_640x480():
    from oryon_amd import ops
    g, objs = vf.golden(), vf.objects()
    names, cls = list(objs), g["cls"].tolist()
    n = len(cls)
    counts = ops.vsd_counts(torch.from_numpy(g["pred"]).cuda(), torch.from_numpy(g["gt"]).cuda(), torch.from_numpy(np.tile(g["K"], (n, 1, 1))).cuda(),
                            torch.from_numpy(vf.test_depths()).cuda(), torch.from_numpy(np.concatenate([objs[k]["pts"] for k in names])),
                            torch.from_numpy(np.concatenate([objs[k]["faces"] for k in names])), torch.from_numpy(g["diameters"]),
                            vert_offset=torch.tensor(np.concatenate(([0], np.cumsum([objs[k]["pts"].shape[0] for k in names]))), dtype=torch.int32),
                            face_offset=torch.tensor(np.concatenate(([0], np.cumsum([objs[k]["faces"].shape[0] for k in names]))), dtype=torch.int32),
                            model_of_pair=torch.tensor([names.index(c) for c in cls], dtype=torch.int32), delta=float(g["delta"]),
                            taus=g["taus"]).cpu().numpy()
    assert counts.dtype == np.int32 and np.array_equal(counts, g["counts"]), (counts, g["counts"])
    assert np.array_equal(ev.vsd_errors(counts), g["errors"])


def test_device_evaluation_with_vsd_matches_reference_evaluator():
    g, objs = vf.golden(), vf.objects()
    n = len(g["cls"])
    status = [2 if i in g["failures"].tolist() else 0 for i in range(n)]
    E = ev.Evaluator("g11", compute_vsd=True)
    ev.evaluate_batch(E, pred_pose_rel=g["pred"], anchor_pose=np.tile(np.eye(4), (n, 1, 1)), gt_pose=g["gt"], K=np.tile(g["K"], (n, 1, 1)),
                      status=status, cls_ids=g["cls"].tolist(), instance_ids=[f"inst{i}" for i in range(n)], objects=objs,
                      iou_a=g["iou_a"], iou_q=g["iou_q"], device="cuda", depth=list(vf.test_depths()))
    for k in ("VSD", "AR", "MSSD", "MSPD"):
        assert np.array_equal(np.asarray(E.metrics[k], dtype=np.float64), g[f"metric_{k}"]), k
    assert E.get_latex_str() == str(g["latex"])


def test_object_off_screen_in_both_poses_scores_one():
    from oryon_amd import ops
    o, K, H, W = vf.objects()["box"], vf.small_camera(48, 64), 48, 64
    pose = np.eye(4)
    pose[:3, 3] = (5.0, 0.0, 0.4)                              # metres: five metres to the right of a 64-pixel image
    depth = torch.full((1, H, W), 700.0)
    counts = ops.vsd_counts(torch.from_numpy(pose)[None].cuda(), torch.from_numpy(pose)[None].cuda(), torch.from_numpy(K)[None].cuda(),
                            depth.cuda(), torch.from_numpy(o["pts"]), torch.from_numpy(o["faces"]), torch.tensor([o["diameter"]])).cpu().numpy()
    assert not counts.any()
    assert np.array_equal(ev.vsd_errors(counts), np.ones((1, 10)))


def test_run_pose_vsd_scores_the_runs_csv_on_the_device(tmp_path, monkeypatch, capsys):
    """`run_pose.py --vsd`: what it adds to run_test.py's summary - the CSV scored by compute_metrics.py on the device - on a fabricated
    NOCS tree.  run_test.main is stood in for by a stub that writes the CSV and returns a summary, so the test is about the VSD path
    and not about the network; the device result must equal the numpy path's (integer counts: VSD exactly)."""
    import json
    import compute_metrics
    import run_pose
    import run_test
    from oryon_amd import synth
    from tests.test_datasets import make_nocs_tree
    base = make_nocs_tree(str(tmp_path))
    _, f = synth.icosphere(1)
    for name in ("mug_a_norm", "can_b_norm"):
        with open(f"{base}/obj_models/real_test/{name}.obj", "w") as fh:
            fh.write("".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f.tolist()))
    csv = str(tmp_path / "preds.csv")
    rel = np.eye(4)
    rel[:3, 3] = (0.01, -0.02, 0.03)

    def stub(argv):
        with open(csv, "w") as fh:
            for i in range(3):
                obj = "mug_a_norm" if i != 1 else "can_b_norm"
                fh.write(ev.format_pred_line(f"1 {10 + i} {obj}", f"2 {20 + i} {obj}", 0.5, 0.75, rel))
        return {"pairs": 3, "csv": csv, "MSSD": 0.0, "not_computed": "VSD / AR", "latex_row": "x & - & - &"}
    monkeypatch.setattr(run_test, "main", stub)
    s = run_pose.main(["--vsd", "--data-root", str(tmp_path), "--dataset", "nocs", "--mask", "oracle", "--out", csv])
    last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "not_computed" not in s and last["VSD"] == s["VSD"] and last["AR"] == s["AR"] and " & - & - & " not in s["latex_row"]
    dev = json.load(open(s["metrics_json"]))
    cpu = compute_metrics.main([csv, "--data-root", str(tmp_path), "--mask", "oracle", "--device", "cpu"])
    ref = json.load(open(cpu["metrics_json"]))
    assert len(dev["VSD"]) == 3 and dev["VSD"] == ref["VSD"] and dev["MSSD"] == ref["MSSD"] and dev["MSPD"] == ref["MSPD"]
    assert dev["AR"] == ref["AR"] and s["VSD"] == cpu["VSD"] and 0.0 <= s["VSD"] <= 1.0
    with pytest.raises(SystemExit):
        run_pose.main(["--vsd", "--pairs", "2"])
