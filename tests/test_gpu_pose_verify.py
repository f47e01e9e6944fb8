"""GPU tests of depth-consistency pose verification (csrc/pose_verify.hip, ops.pose_verify, geo6d.pose_depth_score, Pipeline
test.verify) against the numpy restatement of its definition (tests/pose_verify_restatement.py).

Bars.  Every output is an integer decided by float64 arithmetic the restatement repeats operation for operation, and no sum over rows
is formed in floating point: counts, cls and best are compared EXACTLY.  The margins of the discrete decisions (u + .5 and v + .5 from
an integer, | |d| - tol |, each >= 1e-9 in its unit) are asserted on the restatement first all the same: they say that the fixtures do
not sit on a threshold, where a one-bit difference would be a finding about the fixture and not about the kernel.

A batch shares one map size, so the fixtures' maps (48 x 48, 40 x 56, 56 x 40) are laid into the top-left corner of a 56 x 60 canvas
(depth 0, mask 0 elsewhere: pixel coordinates and intrinsics are unchanged) and the restatement is given the same canvas; the maps'
own shapes run as single-pair calls."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_plane_restatement as P  # noqa: E402
import pose_verify_restatement as R  # noqa: E402
import test_gpu_icp_plane as G  # noqa: E402  (its canvas, synthetic batch and pipeline builders)

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
CAP = 300                                   # the largest n_s: rows beyond a pair's count hold NaN
T_GT = 1                                    # the place of float32(T_gt) in R.candidates


def batch_pairs(cands=R.candidates):
    """The five fixtures on the canvas (300, 257, 256, 255 and 5 rows), a pair with a failure status between them and a pair without rows."""
    pairs = [G.on_canvas(P.fixture(k)) for k in sorted(P.FIXTURES)]
    pairs.insert(2, G.on_canvas(P.fixture(2), name="failed", status=2))
    pairs.append(G.on_canvas(P.fixture(3), name="no_rows", n=0))
    return [dict(p, poses=cands(p)) for p in pairs]


def pack(pairs, cap=None, dev="cuda"):
    B = len(pairs)
    ns = [p.get("n", p["src"].shape[0]) for p in pairs]
    cap = cap or max(max(ns), 1)
    src = np.full((B, cap, 3), np.nan)
    for b, p in enumerate(pairs):
        src[b, :ns[b]] = p["src"][:ns[b]]
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    return dict(src=t(src, torch.float64), n_src=t(np.array(ns), torch.int32), depth=t(np.stack([p["depth"] for p in pairs]), torch.float32),
                mask=t(np.stack([p["mask"] for p in pairs]), torch.int32), cam9=t(np.stack([p["cam9"] for p in pairs]), torch.float64),
                poses=t(np.stack([p["poses"] for p in pairs]), torch.float32), status=t(np.array([p.get("status", 0) for p in pairs]), torch.int32))


def run(pk, tol, **kw):
    from oryon_amd import ops
    out = ops.pose_verify(pk["src"], pk["n_src"], pk["depth"], pk["mask"], pk["cam9"], pk["poses"], tol=tol, status=pk["status"], want_cls=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


_restated = {}


def restate(pairs, tol):
    """The restatement of every pair (computed once per configuration and shared), with its margins asserted."""
    rs = []
    for p in pairs:
        n = p.get("n", p["src"].shape[0])
        key = (p["name"], p["depth"].shape, p["poses"].tobytes(), tol, n)
        if key not in _restated:
            _restated[key] = R.verify(p["src"], p["depth"], p["mask"], p["cam9"], p["poses"], tol, status_in=p.get("status", 0), n_s=n)
        r = _restated[key]
        assert r["frac_gap"] >= MARGIN and r["tol_gap"] >= MARGIN, (p["name"], r["frac_gap"], r["tol_gap"])
        rs.append(r)
    return rs


def compare(out, pairs, rs, what):
    for b, (p, r) in enumerate(zip(pairs, rs)):
        n = p.get("n", p["src"].shape[0])
        print(f"{what}[{b}] {p['name']}: n {n}, best {out['best'][b]} / {r['best']}, hits {out['counts'][b, :, R.HIT].tolist()} / "
              f"{r['counts'][:, R.HIT].tolist()}, margins {r['frac_gap']:.2e} px {r['tol_gap']:.2e} m")
        assert np.array_equal(out["counts"][b], r["counts"]), (p["name"], out["counts"][b].tolist(), r["counts"].tolist())
        assert out["best"][b] == r["best"]
        assert np.array_equal(out["cls"][b, :, :n], r["cls"][:, :n]) and (out["cls"][b, :, n:] == -1).all()
        live = p.get("status", 0) == 0
        assert (out["counts"][b].sum(axis=1) == (n if live else 0)).all()
        assert np.array_equal(out["score"][b], r["counts"][:, R.HIT] / float(max(n, 1)))


@pytest.mark.parametrize("tol", R.TOLS)
def test_the_fixtures_in_one_batch_beside_pairs_that_do_not_run(tol):
    pairs = batch_pairs()
    out = run(pack(pairs, cap=CAP), tol)
    assert out["counts"].shape == (7, 4, 7) and out["cls"].shape == (7, 4, CAP) and out["counts"].dtype == np.int32
    compare(out, pairs, restate(pairs, tol), "batch")
    for b, p in enumerate(pairs):
        if p["name"] in ("failed", "no_rows"):
            assert not out["counts"][b].any() and out["best"][b] == 0 and (out["cls"][b] == -1).all() and not out["score"][b].any()
        elif p["name"] != "pair5":
            assert out["best"][b] == T_GT and (out["counts"][b, 0] >= 1).all()          # every class occurs under T0


@pytest.mark.parametrize("k", sorted(P.FIXTURES))
def test_each_map_at_its_own_shape_cap_equal_to_n_and_the_extremes_of_k(k):
    """40 x 56 and 56 x 40: a swapped H and W, or a row stride that is not W, shows here.  cap_src = n_s exactly (257: two blocks, the
    second holding one row; 256: one full block).  K = 4, K = 1 (each candidate alone) and K = 16."""
    f = P.fixture(k)
    p = dict(f, poses=R.candidates(f))
    compare(run(pack([p]), 0.005), [p], restate([p], 0.005), "own shape")
    for j in range(4):
        one = dict(f, name=f"{f['name']}_only{j}", poses=p["poses"][j:j + 1])
        out = run(pack([one]), 0.005)
        compare(out, [one], restate([one], 0.005), "K = 1")
        assert out["best"][0] == 0 and np.array_equal(out["counts"][0, 0], R.restated(k, 0.005)["counts"][j])
    wide = dict(f, name=f["name"] + "_16", poses=R.sixteen(f))
    for tol in R.TOLS:
        out = run(pack([wide]), tol)
        assert out["counts"].shape == (1, 16, 7)
        compare(out, [wide], restate([wide], tol), "K = 16")
    from oryon_amd import ops
    pk = pack([one])
    flat = ops.pose_verify(pk["src"], pk["n_src"], pk["depth"], pk["mask"], pk["cam9"], pk["poses"][:, 0].contiguous(), tol=0.005)    # [B,4,4]: K = 1
    assert "cls" not in flat and np.array_equal(flat["counts"].cpu().numpy()[0], restate([one], 0.005)[0]["counts"])


def test_a_map_of_480_by_640_with_rows_in_the_far_corner():
    """py W + px up to 307 199: 250 of the 300 rows project into the last 30 lines and 40 columns of the map (a few past its edge), the
    rest all over it.  The second candidate shifts everything by some twenty pixels, the third pushes it 3 cm back, the fourth pulls it 3 cm
    forward (which also moves the corner's rows some ten pixels outwards: many leave the map)."""
    H, W, n = 480, 640, 300
    rng = np.random.default_rng(48)
    surf = lambda x, y: 900.0 + 30.0 * np.sin(0.02 * x + 0.3) * np.cos(0.017 * y) + 0.05 * x
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = surf(xx, yy).astype(np.float32)
    depth[H - 6:H - 4, W - 20:W - 10] = 0.0
    mask = ((xx >= W - 25) & (yy >= H - 20)).astype(np.int32)
    f = 600.0
    cam9 = np.array([f, 0.0, W / 2 - 0.5, 0.0, f, H / 2 - 0.5, 0.0, 0.0, 1.0], dtype=np.float32).astype(np.float64)
    x = np.concatenate([rng.uniform(W - 40.0, W + 1.0, 250), rng.uniform(-2.0, W + 1.0, 50)])
    y = np.concatenate([rng.uniform(H - 30.0, H + 1.0, 250), rng.uniform(-2.0, H + 1.0, 50)])
    z = surf(x, y)
    src = np.stack([(x - cam9[2]) * z / f / 1000.0, (y - cam9[5]) * z / f / 1000.0, z / 1000.0], axis=1)
    eye = np.eye(4, dtype=np.float32)
    poses = np.stack([eye, R.shifted(eye, 0.0), R.shifted(eye, 0.03), R.shifted(eye, -0.03)])
    poses[1, 0, 3], poses[1, 1, 3] = -0.03, -0.02                       # some twenty pixels away from the corner and out of most of the mask
    p = dict(name="vga", src=src, depth=depth, mask=mask, cam9=cam9, poses=poses)
    r = restate([p], 0.01)[0]
    inside = r["cls"][0] >= R.UNKNOWN
    pix = (np.floor(y + 0.5) * W + np.floor(x + 0.5))[inside]
    assert pix.max() > H * W - W and (pix > (H - 31) * W).sum() >= 200                  # the last line of the map is read
    assert (r["counts"][0] >= 1)[[R.OUTSIDE, R.UNKNOWN, R.OFF, R.HIT]].all() and r["counts"][2, R.OCCLUDED] >= 250 and r["counts"][3, R.VIOLATION] >= 100
    assert r["best"] == 0
    compare(run(pack([p]), 0.01), [p], [r], "480x640")


def test_identical_bytes_across_runs_streams_batch_position_and_batch_shape():
    from oryon_amd import ops
    pairs = batch_pairs()
    pk = pack(pairs, cap=CAP)
    keys = ("counts", "best", "cls", "score")
    first, again = run(pk, 0.005), run(pk, 0.005)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.pose_verify(pk["src"], pk["n_src"], pk["depth"], pk["mask"], pk["cam9"], pk["poses"], tol=0.005, status=pk["status"], want_cls=True)
    side.synchronize()
    other = {k: v.cpu().numpy() for k, v in other.items()}
    flipped = run({k: v.flip(0).contiguous() for k, v in pk.items()}, 0.005)
    for k in keys:
        assert first[k].tobytes() == again[k].tobytes(), k
        assert first[k].tobytes() == other[k].tobytes(), k
        assert first[k].tobytes() == flipped[k][::-1].tobytes(), k
    for b, p in enumerate(pairs):                                          # the ragged batch against single-pair calls, cap_src = n_s
        one = run(pack([p]), 0.005)
        n = p.get("n", p["src"].shape[0])
        for k in ("counts", "best", "score"):
            assert one[k][0].tobytes() == first[k][b].tobytes(), (p["name"], k)
        assert np.array_equal(one["cls"][0][:, :n], first["cls"][b][:, :n])


def test_permuted_and_duplicated_candidates():
    base = batch_pairs()
    first = run(pack(base, cap=CAP), 0.005)
    order = [2, 0, 3, 1]
    moved = run(pack(batch_pairs(lambda f: R.candidates(f)[order]), cap=CAP), 0.005)
    assert np.array_equal(moved["counts"], first["counts"][:, order]) and np.array_equal(moved["cls"], first["cls"][:, order])
    for b, p in enumerate(base):
        live = p.get("status", 0) == 0 and p.get("n", 1) > 0
        assert moved["best"][b] == (order.index(int(first["best"][b])) if live else 0)
    twice = run(pack(batch_pairs(lambda f: R.candidates(f)[[0, 1, 2, 1]]), cap=CAP), 0.005)       # the best candidate twice: the lower index
    for b, p in enumerate(base):
        if p["name"] in ("pair1", "pair2", "pair3", "pair4"):
            assert twice["best"][b] == 1 and np.array_equal(twice["counts"][b, 1], twice["counts"][b, 3])


def test_geo6d_facade_equals_the_operator():
    from oryon_amd import geo6d
    f = P.fixture(2)
    poses = R.candidates(f)
    g = geo6d.pose_depth_score(f["src"], f["depth"], f["mask"], f["cam9"].reshape(3, 3), poses, tol=0.005)
    o = run(pack([dict(f, poses=poses)]), 0.005)
    assert g["counts"].shape == (4, 7) and g["counts"].dtype == np.int32 and np.array_equal(g["counts"], o["counts"][0])
    assert g["best"] == int(o["best"][0]) == T_GT and np.array_equal(g["score"], o["score"][0]) and g["score"].shape == (4,)
    one = geo6d.pose_depth_score(f["src"], f["depth"], f["mask"], f["cam9"].reshape(3, 3), poses[1], tol=0.005)       # one [4,4]
    assert one["counts"].shape == (1, 7) and np.array_equal(one["counts"][0], g["counts"][1]) and one["best"] == 0
    none = geo6d.pose_depth_score(np.zeros((0, 3)), f["depth"], f["mask"], f["cam9"].reshape(3, 3), poses)
    assert not none["counts"].any() and none["best"] == 0 and not none["score"].any()


def test_pose_verify_rejects_tensors_it_would_have_to_convert():
    from oryon_amd import ops
    f = P.fixture(4)
    pk = pack([dict(f, poses=R.candidates(f))])
    names = ("src", "n_src", "depth", "mask", "cam9", "poses")
    args = lambda **kw: [dict(pk, **kw)[k] for k in names]
    wide = torch.zeros(1, 64, 6, dtype=torch.float64, device="cuda")
    for change, name in ((dict(src=pk["src"].float()), r"src\.dtype == float64"), (dict(src=wide[:, :, :3]), r"src\.is_contiguous"),
                         (dict(n_src=pk["n_src"].long()), "n_src is"), (dict(depth=pk["depth"].double()), r"depth\.dtype == float32"),
                         (dict(depth=pk["depth"][0]), r"depth\.shape"), (dict(depth=pk["depth"].transpose(1, 2)), r"depth\.is_contiguous"),
                         (dict(mask=pk["mask"].bool()), r"mask\.dtype == int32"), (dict(mask=pk["mask"][:, :-1].contiguous()), r"mask\.shape"),
                         (dict(cam9=pk["cam9"].float()), r"cam9\.dtype == float64"), (dict(cam9=pk["cam9"].reshape(1, 3, 3)), r"cam9\.shape"),
                         (dict(poses=pk["poses"].double()), r"poses\.dtype == float32"), (dict(poses=pk["poses"][:, :, :3]), r"poses\.shape"),
                         (dict(poses=pk["poses"].transpose(2, 3)), r"poses\.is_contiguous"), (dict(poses=pk["poses"][:, :0]), r"poses\.shape"),
                         (dict(poses=pk["poses"].repeat(1, 5, 1, 1)[:, :17].contiguous()), "K <= 16"), (dict(src=pk["src"].cpu()), r"src\.is_cuda"),
                         (dict(poses=pk["poses"].cpu()), r"poses\.is_cuda")):
        with pytest.raises(ValueError, match="pose_verify: " + name):
            ops.pose_verify(*args(**change))
    for kw, name in ((dict(tol=-1.0), "tol >= 0"), (dict(tol=float("nan")), "tol >= 0"), (dict(status=pk["status"].long()), "status is")):
        with pytest.raises(ValueError, match="pose_verify: .*" + name):
            ops.pose_verify(*args(), **kw)
    with pytest.raises(ValueError, match="cap_src <= 8192"):
        ops.pose_verify(*args(src=torch.zeros(1, 8193, 3, dtype=torch.float64, device="cuda")))


# ------------------------------------------------------------------------------------------------------------------ Pipeline
def _sides(pl, batch, b):
    """What the pipeline hands its helpers for pair b of the batch, built here from the batch alone."""
    depth_a = batch["anchor"]["orig_depth"][b].squeeze().to("cuda", torch.float32)[None].contiguous()
    depth_q = batch["query"]["orig_depth"][b].squeeze().to("cuda", torch.float32)[None].contiguous()
    cam_a, cam_q = batch["anchor"]["camera"][b:b + 1].cuda(), batch["query"]["camera"][b:b + 1].cuda()
    key = torch.tensor([b], dtype=torch.int64, device="cuda")
    src, n_src = pl._refine_cloud(batch["anchor"]["mask"][b:b + 1].cuda(), depth_a, cam_a, pl.REFINE_SEED_A, key)
    return src, n_src, pl.refine_target(batch["query"]["mask"][b:b + 1].cuda(), depth_q, cam_q)


def test_verify_score_per_sample_is_pose_verify_by_hand_and_batched_agrees(monkeypatch):
    import oryon_amd.pipeline as pipeline_module
    from oryon_amd import ops
    batch = G._batch([3, 4, 5, 6])
    batch["anchor"]["mask"][2] = 0                       # NO_MASK
    base, pl = G._pipeline(), G._pipeline(verify="score", refine_points=512)
    out0, out = base.test_step_batched(batch), pl.test_step_batched(batch)
    assert out["status"].cpu().tolist() == [0, 0, 1, 0] and not any(k.startswith("verify") for k in out0)
    assert out["pose"].cpu().numpy().tobytes() == out0["pose"].cpu().numpy().tobytes() and "pose_unrefined" not in out      # poses untouched
    assert tuple(out["verify_counts"].shape) == (4, 1, 7) and tuple(out["verify_score"].shape) == (4,) and "verify_best" not in out
    assert pl.last_verify["counts"] is out["verify_counts"]
    counts = out["verify_counts"].cpu().numpy()
    assert not counts[2].any() and float(out["verify_score"][2]) == 0.0
    starts = iter([out["pose"][b].cpu().double() for b in (0, 1, 3)])
    monkeypatch.setattr(pipeline_module, "get_pointdsc_pose", lambda *a, **k: next(starts))
    torch.manual_seed(1)
    recs = pl.test_step(batch, 0)
    assert [r["status"] for r in recs] == [0, 0, 1, 0] and "verify_counts" not in recs[2] and "verify_score" not in recs[2]
    for b in (0, 1, 3):
        rec = recs[b]
        assert rec["pred_pose_rel"].numpy().tobytes() == out["pose"][b].cpu().numpy().tobytes()
        src, n_src, target = _sides(pl, batch, b)
        assert int(n_src[0]) == 512
        hand = ops.pose_verify(src, n_src, target["depth"], target["mask"], target["cam9"], rec["pred_pose_rel"][None].cuda().contiguous(), tol=0.01)
        print(f"pair {b}: counts {rec['verify_counts']}, score {rec['verify_score']:.3f}")
        assert isinstance(rec["verify_counts"], list) and len(rec["verify_counts"]) == 7 and sum(rec["verify_counts"]) == 512
        assert rec["verify_counts"] == hand["counts"][0, 0].cpu().tolist() == counts[b, 0].tolist()
        assert rec["verify_score"] == float(hand["score"][0, 0]) == float(out["verify_score"][b]) == rec["verify_counts"][6] / 512
        assert rec["verify_score"] > 0.0                                   # a solved pair: some of the cloud is confirmed on the object
    s = pl.verify_summary()
    assert s["verify"] == "score" and s["verify_tol"] == 0.01 and s["verify_pairs"] == 6 and 0.0 < s["verify_score_mean"] <= 1.0
    assert "verify_refinements_kept" not in s and base.verify_summary() == {}
    # test.verify_tol reaches the kernel: at 0 a row agrees with the depth only where d == 0 exactly, and the hits can only shrink
    tight = G._pipeline(verify="score", refine_points=512, verify_tol=0.0).test_step_batched(batch)
    assert (tight["verify_counts"][:, 0, 6] <= out["verify_counts"][:, 0, 6]).all()
    assert int(tight["verify_counts"][:, 0, 6].sum()) < int(out["verify_counts"][:, 0, 6].sum())


@pytest.mark.parametrize("refine", ["icp", "icp_plane"])
def test_verify_guard_keeps_the_pose_the_counts_choose(refine):
    batch = G._batch([3, 4, 5, 6])
    batch["anchor"]["mask"][2] = 0                       # NO_MASK
    pl = G._pipeline(refine=refine, refine_points=512, verify="guard")
    out = pl.test_step_batched(batch)
    assert out["status"].cpu().tolist() == [0, 0, 1, 0]
    counts, best = out["verify_counts"].cpu().numpy(), out["verify_best"].cpu().numpy()
    assert counts.shape == (4, 2, 7) and best.shape == (4,) and best.dtype == np.int32
    cand = [out["pose_unrefined"].cpu().numpy(), out["pose_refined"].cpu().numpy()]
    for b in range(4):
        print(f"{refine} pair {b}: hits {counts[b, :, 6].tolist()}, bad {(counts[b, :, 0] + counts[b, :, 4] + counts[b, :, 5]).tolist()}, best {best[b]}")
        assert best[b] == R.select(counts[b])
        assert out["pose"][b].cpu().numpy().tobytes() == cand[best[b]][b].tobytes()
        assert float(out["verify_score"][b]) == counts[b, best[b], 6] / 512
        if b != 2:
            assert (counts[b].sum(axis=1) == 512).all() and cand[0][b].tobytes() != cand[1][b].tobytes()
    assert torch.equal(out["pose"][2].cpu(), torch.eye(4)) and not counts[2].any() and best[2] == 0
    np.testing.assert_allclose(out["pred_q"].cpu().numpy(), out["pose"].cpu().numpy() @ batch["anchor"]["pose"].numpy(), atol=1e-6)
    plain = G._pipeline(refine=refine, refine_points=512).test_step_batched(batch)             # the refinement itself is what it was
    assert plain["pose"].cpu().numpy().tobytes() == out["pose_refined"].cpu().numpy().tobytes()
    assert plain["pose_unrefined"].cpu().numpy().tobytes() == out["pose_unrefined"].cpu().numpy().tobytes()
    s = pl.verify_summary()
    assert s["verify"] == "guard" and s["verify_pairs"] == 3 and s["verify_refinements_kept"] == int((best[[0, 1, 3]] == 1).sum())


def test_verify_guard_per_sample_follows_the_same_rule(monkeypatch):
    import oryon_amd.pipeline as pipeline_module
    batch = G._batch([3, 4])
    pl = G._pipeline(refine="icp_plane", refine_points=512, verify="guard")
    out = pl.test_step_batched(batch)
    starts = iter([out["pose_unrefined"][b].cpu().double() for b in (0, 1)])
    monkeypatch.setattr(pipeline_module, "get_pointdsc_pose", lambda *a, **k: next(starts))
    torch.manual_seed(1)
    recs = pl.test_step(batch, 0)
    for b, rec in enumerate(recs):
        best = int(out["verify_best"][b])
        assert rec["verify_best"] == best and rec["verify_counts"] == out["verify_counts"][b, best].cpu().tolist()
        if best == 0:                                    # the solver's pose, handed in: the very bytes
            assert rec["pred_pose_rel"].numpy().tobytes() == out["pose"][b].cpu().numpy().tobytes()
        else:                                            # the refined pose: the two routes agree as test_gpu_icp_plane.py bars them
            assert float((rec["pred_pose_rel"] - out["pose"][b].cpu()).abs().max()) <= 1e-6


def test_verify_guard_keeps_a_refinement_that_repairs_a_bad_start(monkeypatch):
    """The solver's pose pushed 15 mm along the camera axis: every row then lies 15 mm off the measured surface, beyond the 10 mm
    tolerance, wherever the measured depth is within 5 mm of the model's (the synthetic depth is a re-projection snapped to pixels, so
    not everywhere: the start keeps a minority of its hits), while 15 mm is inside the refiner's 20 mm gate and it pulls the cloud back
    onto the surface.  The guard must keep the refinement, and the record's pose is the refiner's output byte for byte."""
    import oryon_amd.pipeline as pipeline_module
    batch = G._batch([3, 4])
    pl = G._pipeline(refine="icp_plane", refine_points=512, verify="guard")
    good = pl.test_step_batched(batch)["pose_unrefined"].cpu()
    bad = good.clone()
    bad[:, 2, 3] += 0.015
    starts = iter([bad[b].double() for b in (0, 1)])
    monkeypatch.setattr(pipeline_module, "get_pointdsc_pose", lambda *a, **k: next(starts))
    seen, verify_poses = [], pl.verify_poses                 # every pair's raw result and the refiner's output it was given

    def spy(*a, **k):
        seen.append((verify_poses(*a, **k), pl.last_refine["T"][0].cpu().numpy().tobytes()))
        return seen[-1][0]
    monkeypatch.setattr(pl, "verify_poses", spy)
    torch.manual_seed(1)
    recs = pl.test_step(batch, 0)
    for b, rec in enumerate(recs):
        v, refined = seen[b]
        counts = v["counts"][0].cpu().numpy()
        print(f"pair {b}: hits [start, refined] {counts[:, 6].tolist()}, bad {(counts[:, 0] + counts[:, 4] + counts[:, 5]).tolist()}, "
              f"iters {rec['refine_iters']}")
        assert int(v["best"][0]) == R.select(counts) == rec["verify_best"] == 1
        assert counts[0, 6] < 512 // 2 < counts[1, 6] and rec["verify_counts"] == counts[1].tolist()
        assert rec["pred_pose_rel"].numpy().tobytes() == refined != bad[b].numpy().tobytes()
    assert pl.verify_summary()["verify_refinements_kept"] >= 2


def test_verify_none_is_the_step_as_it_was():
    batch = G._batch([3, 4])
    named = G._pipeline(refine="icp_plane", refine_points=512, verify="none")
    bare = G._pipeline(refine="icp_plane", refine_points=512)
    del bare.args.test.verify, bare.args.test.verify_tol                   # arg objects from before the flag existed
    a, b = named.test_step_batched(batch), bare.test_step_batched(batch)
    assert set(a) == set(b) and not any(k.startswith("verify") or k == "pose_refined" for k in a)
    for k in ("pose", "pose_unrefined", "pred_q", "refine_iters", "status"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    torch.manual_seed(1)
    recs = named.test_step(batch, 0)
    assert all(not any(k.startswith("verify") for k in r) for r in recs) and named.last_verify is None and named.verify_summary() == {}
