"""VSD on the CPU: the numpy rasteriser (evaluation.rasterize_depth) against its definition and against analytic depths, the counts
and errors against what the reference's vsd / Evaluator(compute_vsd=True) produced (tests/golden/g11_vsd.npz, written by
`tools/gen_goldens.py vsd`), and the mesh face readers."""
import struct

import numpy as np
import pytest

from oryon_amd import datasets, synth
from oryon_amd import evaluation as ev
from tests import vsd_fixture as vf

EPS = float(np.finfo(np.float32).eps)


def _eye_mm(tz):
    P = np.eye(4, dtype=np.float32)
    P[2, 3] = tz
    return P


# ---------------------------------------------------------------------------------------------- the rasteriser against its definition
def test_quad_on_pixel_centres_covers_the_half_open_block():
    """Corners that project exactly onto sample points (a + 0.5, b + 0.5): the top-left rule keeps the samples on the left and top
    edges and drops those on the right and bottom ones, and the shared diagonal is drawn once."""
    H, W, Z, f = 24, 32, 512.0, 256.0                       # X = (u - cx) Z / f: exact in fp32 for these powers of two
    K = np.array([[f, 0, 16.0], [0, f, 12.0], [0, 0, 1]])
    a, a2, b, b2 = 5, 19, 3, 14
    corners = [(a, b), (a2, b), (a2, b2), (a, b2)]
    verts = np.array([[(c + 0.5 - 16.0) * Z / f, (r + 0.5 - 12.0) * Z / f, 0.0] for c, r in corners])
    for faces in ([[0, 1, 2], [0, 2, 3]], [[1, 2, 3], [1, 3, 0]], [[0, 2, 1], [0, 3, 2]]):
        d = ev.rasterize_depth(_eye_mm(Z), K, verts, np.array(faces), H, W)
        want = np.zeros((H, W), bool)
        want[b:b2, a:a2] = True
        assert np.array_equal(d > 0, want)
        assert (d[want] == np.float32(Z)).all()               # constant Z, a power of two: 1 / (1 / Z) is exact
    assert d.dtype == np.float32


def test_box_face_on_is_piecewise_planar():
    """The box seen along its z axis: the front face is the plane Z = tz - 30 = 370, exact in the vertex stage; on a plane of
    constant Z the interpolation returns iz itself, so the only roundings are those of iz = 1 / Z and of depth = 1 / iz: half an ulp
    each, |depth - Z| <= eps * Z."""
    o, H, W = vf.objects()["box"], 60, 80
    K = vf.small_camera(H, W)
    d = ev.rasterize_depth(_eye_mm(400.0), K, o["pts"], o["faces"], H, W)
    Zf = 400.0 - 30.0
    u, v = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    x, y = (u - K[0, 2]) * Zf / K[0, 0], (v - K[1, 2]) * Zf / K[1, 1]
    snap = Zf / K[0, 0] / 256.0                             # a vertex moves by at most half of 1/256 pixel
    inside = (np.abs(x) < 60.0 - snap) & (np.abs(y) < 45.0 - snap)
    outside = (np.abs(x) > 60.0 + snap) | (np.abs(y) > 45.0 + snap)
    assert inside.sum() > 300 and (d[inside] > 0).all() and (d[outside] == 0).all()
    assert np.abs(d[inside] - Zf).max() <= EPS * Zf


def _ray_sphere(K, H, W, centre, radius):
    """Nearest depth (Z) at which the ray through each sample point meets the sphere; NaN where it misses."""
    u, v = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1)
    dd, dc = (d * d).sum(-1), d @ centre
    disc = dc * dc - dd * (centre @ centre - radius * radius)
    with np.errstate(invalid="ignore"):
        return (dc - np.sqrt(disc)) / dd


@pytest.mark.parametrize("name", ["ico2", "ico3"])
def test_icosphere_lies_between_its_two_spheres(name):
    """The mesh lies between the sphere through its vertices and the sphere that touches its nearest face plane, so does every
    rendered depth - up to the snap of the vertices to 1/256 pixel, which moves the surface sideways by at most
    sqrt(2)/512 pixel = sqrt(2)/512 * Z / f millimetres, and the fp32 rounding of the interpolation (a few ulp of Z)."""
    o, H, W = vf.objects()[name], 60, 80
    K = vf.small_camera(H, W)
    P = _eye_mm(400.0)
    P[0, 3], P[1, 3] = 7.0, -4.0
    centre = P[:3, 3].astype(np.float64)
    v, f = o["pts"], o["faces"]
    r_out = np.linalg.norm(v, axis=1).max()
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    r_in = np.abs((n * v[f[:, 0]]).sum(1) / np.linalg.norm(n, axis=1)).min()
    assert 0.9 * r_out < r_in < r_out
    slack = np.sqrt(2.0) / 512.0 * (400.0 + r_out) / K[0, 0] + 8 * EPS * 500.0
    near, far = _ray_sphere(K, H, W, centre, r_out + slack), _ray_sphere(K, H, W, centre, r_in - slack)
    d = ev.rasterize_depth(P, K, v, f, H, W)
    assert (d[~np.isnan(far)] > 0).all() and (d[np.isnan(near)] == 0).all() and (~np.isnan(far)).sum() > 300
    cov = d > 0
    assert (d[cov] >= near[cov]).all()
    both = cov & ~np.isnan(far)
    assert (d[both] <= far[both]).all()


def test_windings_degenerate_behind_and_cropped():
    o, H, W = vf.objects()["twopart"], 48, 64
    K = vf.small_camera(H, W)
    P = _eye_mm(420.0)
    P[:3, :3] = np.array([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]]) @ np.array([[1, 0, 0], [0, 0.6, -0.8], [0, 0.8, 0.6]])
    d = ev.rasterize_depth(P, K, o["pts"], o["faces"], H, W)
    assert (d > 0).sum() > 150
    assert np.array_equal(d, ev.rasterize_depth(P, K, o["pts"], o["faces"][:, [0, 2, 1]], H, W))        # both windings are drawn
    # a triangle without area, and one with a vertex behind the camera, draw nothing
    tri = np.array([[-30.0, -20.0, 0.0], [30.0, -20.0, 0.0], [0.0, 25.0, 0.0]])
    one = np.array([[0, 1, 2]])
    assert (ev.rasterize_depth(_eye_mm(300.0), K, tri, one, H, W) > 0).sum() > 50        # about 74 pixels of area
    assert not ev.rasterize_depth(_eye_mm(300.0), K, np.array([[-30.0, 0, 0], [0.0, 0, 0], [30.0, 0, 0]]), one, H, W).any()
    assert not ev.rasterize_depth(_eye_mm(300.0), K, tri, np.array([[0, 1, 1]]), H, W).any()
    behind = tri.copy()
    behind[2, 2] = -400.0
    assert not ev.rasterize_depth(_eye_mm(300.0), K, behind, one, H, W).any()
    assert not ev.rasterize_depth(_eye_mm(-300.0), K, tri, one, H, W).any()
    # half off the screen: cropped, the visible part unchanged
    shift = _eye_mm(300.0)
    shift[0, 3] = 128.0                                       # 128 mm * 70.4 / 300 mm = 30.04 pixels to the right
    full = ev.rasterize_depth(shift, K, tri, one, H, 2 * W)
    crop = ev.rasterize_depth(shift, K, tri, one, H, W)
    assert (full[:, W:] > 0).any() and (crop > 0).sum() > 20 and np.array_equal(crop, full[:, :W])


def test_golden_crops_of_the_640x480_renders():
    g, objs = vf.golden(), vf.objects()
    for key, i, which in (("crop_gt_1", 1, "gt"), ("crop_est_3", 3, "pred")):
        o = objs[str(g["cls"][i])]
        d = ev.rasterize_depth(vf.pose_mm(g[which][i]), g["K"], o["pts"], o["faces"], 480, 640)
        r0, c0 = g[key + "_origin"]
        assert (g[key] > 0).sum() > 500 and np.array_equal(d[r0:r0 + 48, c0:c0 + 64], g[key])


# ---------------------------------------------------------------------------------------------- counts, errors, the evaluator
def test_synth_poses_are_the_goldens():
    g = vf.golden()
    gt, pred = synth.vsd_poses()
    np.testing.assert_allclose(gt, g["gt"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(pred, g["pred"], rtol=0, atol=1e-12)
    assert g["cls"].tolist() == list(synth.VSD_CLS) and g["failures"].tolist() == list(synth.VSD_FAILURES)


@pytest.fixture(scope="module")
def counts():
    g, objs = vf.golden(), vf.objects()
    depth = vf.test_depths()
    return np.stack([ev.vsd_counts_np(g["pred"][i], g["gt"][i], g["K"], depth[i], objs[c]["pts"], objs[c]["faces"], objs[c]["diameter"],
                                      float(g["delta"]), g["taus"]) for i, c in enumerate(g["cls"].tolist())])


def test_counts_and_errors_equal_the_reference(counts):
    g = vf.golden()
    assert counts.dtype == np.int32 and np.array_equal(counts, g["counts"])
    assert np.array_equal(ev.vsd_errors(counts), g["errors"])
    assert (g["errors"][0] == 0).all() and (g["errors"][5] == 1).all()              # exact pose; pose behind the camera
    assert np.array_equal(ev.vsd_errors(np.zeros((2, 12), np.int32)), np.ones((2, 10)))     # empty union


def _registered(E, g, vsd_errs):
    n = len(g["cls"])
    objs = vf.objects()
    for i in range(n):
        cls = str(g["cls"][i])
        if i in g["failures"].tolist():
            E.register_test_failure(cls_id=cls, instance_id=f"inst{i}", iou_a=g["iou_a"][i], iou_q=g["iou_q"][i])
            continue
        o = objs[cls]
        th, sh = ev.compute_RT_distances(g["pred"][i].astype(np.float32), g["gt"][i])      # the pipeline hands fp32 poses over
        kw = dict(vsd_errs=vsd_errs[i]) if vsd_errs is not None else {}
        E.register_test(pred_pose_rel=g["pred"][i].astype(np.float32), rot_deg=float(th[0]), trans_cm=float(sh[0]),
                        add_s=ev.compute_add(o["pts"] / 1000.0, g["pred"][i].astype(np.float32), g["gt"][i]),
                        add_diam=ev.extent_diameter(o["pts"]) / 1000.0,
                        mssd_mm=ev.mssd_error(g["pred"][i].astype(np.float32), g["gt"][i], o["pts"], o["syms"]),
                        mspd_px=ev.mspd_error(g["pred"][i].astype(np.float32), g["gt"][i], g["K"], o["pts"], o["syms"]),
                        bop_diam_mm=o["diameter"], cls_id=cls, instance_id=f"inst{i}", iou_a=g["iou_a"][i], iou_q=g["iou_q"][i], **kw)
    return E


def test_evaluator_with_vsd_reproduces_the_reference(counts):
    g = vf.golden()
    E = _registered(ev.Evaluator("g11", compute_vsd=True), g, ev.vsd_errors(counts))
    for k in ("VSD", "AR", "MSSD", "MSPD", "ADD(S)-0.1d"):
        assert np.array_equal(np.asarray(E.metrics[k], dtype=np.float64), g[f"metric_{k}"]), k
    assert g["metric_VSD"][6] == 0 and g["metric_AR"][6] == 0 and 0 < g["metric_VSD"][1] < 1          # the failure; a partial score
    means = E.get_means()
    assert list(means) == g["mean_names"].tolist()
    np.testing.assert_allclose([means[k] for k in means], g["mean_values"], rtol=1e-6)       # R / T errors are fp32 in the reference
    assert means["VSD"] == g["mean_values"][g["mean_names"].tolist().index("VSD")]
    assert means["AR"] == g["mean_values"][g["mean_names"].tolist().index("AR")]
    assert E.get_latex_str() == str(g["latex"])
    with pytest.raises(ValueError):
        _registered(ev.Evaluator("g11", compute_vsd=True), g, None)


def test_evaluator_default_still_prints_the_row_without_vsd():
    g = vf.golden()
    E = _registered(ev.Evaluator("g11"), g, None)
    assert "VSD" not in E.metrics and "AR" not in E.metrics
    assert E.get_latex_str() == str(g["latex_no_vsd"]) and " & - & - & " in E.get_latex_str()


def test_evaluate_batch_numpy_path_with_vsd():
    g, objs = vf.golden(), vf.objects()
    n = len(g["cls"])
    status = [2 if i in g["failures"].tolist() else 0 for i in range(n)]
    E = ev.Evaluator("g11", compute_vsd=True)
    args = dict(pred_pose_rel=g["pred"], anchor_pose=np.tile(np.eye(4), (n, 1, 1)), gt_pose=g["gt"], K=np.tile(g["K"], (n, 1, 1)),
                status=status, cls_ids=g["cls"].tolist(), instance_ids=[f"inst{i}" for i in range(n)], objects=objs, iou_a=g["iou_a"],
                iou_q=g["iou_q"])
    ev.evaluate_batch(E, depth=list(vf.test_depths()), **args)
    for k in ("VSD", "AR"):
        assert np.array_equal(np.asarray(E.metrics[k], dtype=np.float64), g[f"metric_{k}"]), k
    assert E.get_latex_str() == str(g["latex"])
    with pytest.raises(ValueError):
        ev.evaluate_batch(ev.Evaluator("g11", compute_vsd=True), **args)


# ---------------------------------------------------------------------------------------------- face readers
def _write_ply(path, verts, faces, binary, list_name="vertex_indices", count_t="uchar", index_t="int", extra_face_prop=False):
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", "comment test", f"element vertex {len(verts)}",
            "property float x", "property float y", "property float z", "property uchar red", f"element face {len(faces)}"]
    if extra_face_prop:
        head.append("property uchar flags")
    head += [f"property list {count_t} {index_t} {list_name}", "end_header"]
    code = datasets._PLY_CODE
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        for v in verts:
            f.write(struct.pack("<3fB", *v, 7) if binary else (" ".join(repr(float(x)) for x in v) + " 7\n").encode())
        for fc in faces:
            if binary:
                f.write((struct.pack("<B", 1) if extra_face_prop else b"") + struct.pack("<" + code[count_t], len(fc)) +
                        struct.pack(f"<{len(fc)}" + code[index_t], *fc))
            else:
                f.write((("1 " if extra_face_prop else "") + f"{len(fc)} " + " ".join(str(i) for i in fc) + "\n").encode())


@pytest.mark.parametrize("binary", [False, True])
def test_read_ply_faces(tmp_path, binary):
    v, f = synth.box_mesh(10.0, 20.0, 30.0)
    p = str(tmp_path / "a.ply")
    _write_ply(p, v, f.tolist(), binary)
    out = datasets.read_ply_faces(p)
    assert out.dtype == np.int32 and np.array_equal(out, f)
    np.testing.assert_allclose(datasets.read_ply_vertices(p), v)
    _write_ply(p, v, f.tolist(), binary, list_name="vertex_index", count_t="ushort", index_t="uint", extra_face_prop=True)
    assert np.array_equal(datasets.read_ply_faces(p), f)
    _write_ply(p, v, f.tolist()[:3] + [[0, 1, 3, 2]], binary)
    with pytest.raises(ValueError, match="only triangles"):
        datasets.read_ply_faces(p)


def test_read_obj_faces_converts_to_zero_based_and_checks_the_range(tmp_path):
    v, f = synth.box_mesh(10.0, 20.0, 30.0)
    p = str(tmp_path / "a.obj")
    with open(p, "w") as fh:
        fh.write("# test\n" + "".join(f"v {x} {y} {z}\n" for x, y, z in v) + "vn 0 0 1\n")
        fh.write("".join(f"f {a + 1}/{a + 1}/1 {b + 1}//1 {c + 1}\n" for a, b, c in f.tolist()))
    out = datasets.read_obj_faces(p, 8)
    assert out.dtype == np.int32 and np.array_equal(out, f)
    with pytest.raises(ValueError, match="outside"):
        datasets.read_obj_faces(p, 7)                         # index 8 of 7 vertices: what the reference would read out of range
    with open(p, "a") as fh:
        fh.write("f 1 2 3 4\n")
    with pytest.raises(ValueError, match="only triangles"):
        datasets.read_obj_faces(p, 8)


def test_object_info_loads_faces_only_on_request(tmp_path):
    from tests.test_datasets import make_nocs_tree, make_toyl_tree
    base = make_nocs_tree(str(tmp_path))
    with open(f"{base}/obj_models/real_test/mug_a_norm.obj", "w") as fh:
        fh.write("f 1/1/1 2/2/2 64/3/3\nf 3 2 1\n")
    ds = datasets.FixedSplit("nocs", str(tmp_path), "nocs", "cross_scene_test", "all")
    plain = ds.object_info("mug_a_norm")
    assert set(plain) == {"pts", "diameter", "syms", "symmetric"}
    full = ds.object_info("mug_a_norm", faces=True)
    assert np.array_equal(full["faces"], [[0, 1, 63], [2, 1, 0]]) and full["pts"] is plain["pts"]
    assert ds.object_info("mug_a_norm") is plain and "faces" not in plain          # today's call and its dict stay as they are
    with pytest.raises(FileNotFoundError):
        ds.object_info("can_b_norm", faces=True)                                    # no .obj in the tree: an error, not an empty mesh
    make_toyl_tree(str(tmp_path))
    dt = datasets.FixedSplit("toyl", str(tmp_path), "toyl", "cross_scene_test", "all")
    assert dt.object_info(3, faces=True)["faces"].shape == (0, 3)                  # the fabricated BOP model has an empty face element
    with pytest.raises(ValueError, match="no face element"):
        dt.object_info(7, faces=True)


def test_compute_metrics_scores_a_prediction_csv_with_vsd(tmp_path, capsys):
    """compute_metrics.py on a fabricated NOCS tree with the numpy path: every pair of the split is registered, VSD and AR are
    reported and AR is the mean of (VSD + MSSD + MSPD) / 3 per pair."""
    import json
    import compute_metrics
    from tests.test_datasets import make_nocs_tree
    base = make_nocs_tree(str(tmp_path))
    v, f = synth.icosphere(1, radius=0.05)                     # 42 of the models' 64 vertices carry the faces
    for name in ("mug_a_norm", "can_b_norm"):
        with open(f"{base}/obj_models/real_test/{name}.obj", "w") as fh:
            fh.write("".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f.tolist()))
    csv = tmp_path / "preds.csv"
    rel = np.eye(4)
    rel[:3, 3] = (0.01, -0.02, 0.03)
    lines = []
    for i in range(3):
        obj = "mug_a_norm" if i != 1 else "can_b_norm"
        lines.append(ev.format_pred_line(f"1 {10 + i} {obj}", f"2 {20 + i} {obj}", 0.5, 0.75, rel))
    csv.write_text("".join(lines))
    s = compute_metrics.main([str(csv), "--data-root", str(tmp_path), "--device", "cpu", "--batch", "2"])
    out = capsys.readouterr().out
    assert s["pairs"] == 3 and 0.0 <= s["VSD"] <= 1.0 and " & - & - & " not in s["latex_row"]
    m = json.load(open(s["metrics_json"]))
    assert len(m["VSD"]) == 3 and len(m["AR"]) == 3
    np.testing.assert_allclose(m["AR"], (np.array(m["VSD"]) + np.array(m["MSSD"]) + np.array(m["MSPD"])) / 3.0, rtol=1e-12)
    assert s["AR"] == np.mean(m["AR"]) and json.loads(out.strip().splitlines()[-1])["AR"] == s["AR"]
