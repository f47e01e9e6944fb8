"""GPU tests of ICP refinement (csrc/icp.hip, ops.icp_refine, geo6d.icp, Pipeline test.refine = icp) against the numpy restatement
of its definition (tests/icp_restatement.py) and the reference's recorded results (tests/golden/icp_*.npz).

Bars.  Neighbour indices, iteration counts and kept-row counts: exact - every case asserts FIRST, on the restatement alone, the
margins that make them independent of rounding (best vs second-best neighbour, |prev - mean| vs tolerance, dist vs max_dist, all
>= 1e-9 relative).  mean_err: 1e-12 relative - to the larger of the mean itself and the size of the numbers it is computed from:
a distance is the root of a sum of squared DIFFERENCES of coordinates around 1 m, so it carries an absolute error of ~1e-16 m however
small it is, and where the target is an exact rigid image of the source (goldens `identity`, `near`, `permuted`) the final mean IS
that rounding noise (~1e-16 m), of which no relative agreement exists; measured there: 8e-2 to 3e-1 of 1e-16 m.  Pose entries (T64): 1e-9, derived, not measured: row sums of <= 8192 float64 terms in
any order (<= n 2^-53 ~ 1e-12 relative), times 20 iterations, times the conditioning that the asserted singular-value ratio bounds by
~50.  Measured gaps: DESIGN.md "ICP refinement"."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS, TILE = 256, 1024          # a workgroup's block of source rows, the LDS tile of target rows (csrc/icp.hip, csrc/nn_tile.h)
POSE_BAR, MEAN_BAR, MARGIN = 1e-9, 1e-12, 1e-9


def golden(name):
    g = np.load(os.path.join(GOLDEN, f"icp_{name}.npz"))
    return dict(name=name, src=g["A"], dst=g["B"], T0=g["init_pose"] if int(g["has_init"]) else None, g=g)


def pack(pairs, cap_s=None, cap_d=None, dev="cuda"):
    """pairs: dicts with src [n_s,3], dst [n_d,3], T0 [4,4] | None, status (default 0) -> the tensors of one call; NaN beyond the counts."""
    B = len(pairs)
    cap_s = cap_s or max(1, max(p["src"].shape[0] for p in pairs))
    cap_d = cap_d or max(1, max(p["dst"].shape[0] for p in pairs))
    src, dst = np.full((B, cap_s, 3), np.nan), np.full((B, cap_d, 3), np.nan)
    T0 = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    for b, p in enumerate(pairs):
        src[b, :p["src"].shape[0]], dst[b, :p["dst"].shape[0]] = p["src"], p["dst"]
        if p.get("T0") is not None:
            T0[b] = np.asarray(p["T0"], dtype=np.float32)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    return dict(src=t(src, torch.float64), dst=t(dst, torch.float64),
                n_src=t(np.array([p["src"].shape[0] for p in pairs]), torch.int32), n_dst=t(np.array([p["dst"].shape[0] for p in pairs]), torch.int32),
                T_init=t(T0, torch.float32), status=t(np.array([p.get("status", 0) for p in pairs]), torch.int32))


def run(pk, **kw):
    from oryon_amd import ops
    out = ops.icp_refine(pk["src"], pk["dst"], pk["n_src"], pk["n_dst"], pk["T_init"], status=pk["status"], want_idx=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def restate(pairs, max_iter=20, tolerance=1e-3, max_dist=np.inf, degenerate=()):
    """The restatement of every pair, with its margins asserted (the precondition of the exact comparisons)."""
    rs = []
    for b, p in enumerate(pairs):
        r = R.icp(p["src"], p["dst"], p.get("T0"), max_iter, tolerance, max_dist, status_in=p.get("status", 0))
        if b not in degenerate:
            assert r["nn_gap"] >= MARGIN and r["conv_gap"] >= MARGIN and r["keep_gap"] >= MARGIN and r["sv_ratio"] >= 1e-2, (b, p.get("name"), r)
        rs.append(r)
    return rs


def compare(out, pairs, rs, what, pose=True):
    """-> the largest pose gap.  Prints every figure before asserting it."""
    worst = 0.0
    for b, (p, r) in enumerate(zip(pairs, rs)):
        n_s = p["src"].shape[0]
        gap = float(np.abs(out["T64"][b] - r["T"][:3]).max())
        scale = max(float(np.nanmax(np.abs(p["src"]))), float(np.nanmax(np.abs(p["dst"])))) if n_s and p["dst"].shape[0] else 1.0
        rel = abs(out["mean_err"][b] - r["mean_err"]) / max(abs(r["mean_err"]), scale) if r["iters"] else abs(out["mean_err"][b])
        print(f"{what}[{b}] {p.get('name', '')}: n {n_s} x {p['dst'].shape[0]}, iters {out['iters'][b]} / {r['iters']}, kept {out['n_kept'][b]} / "
              f"{r['n_kept']}, |T64 - restatement| {gap:.2e}, mean_err {r['mean_err']:.3e} off by {abs(out['mean_err'][b] - r['mean_err']):.2e} "
              f"(bar {MEAN_BAR * max(abs(r['mean_err']), scale):.1e})")
        assert out["iters"][b] == r["iters"] and out["n_kept"][b] == r["n_kept"]
        assert np.array_equal(out["idx"][b, :n_s], r["idx"]) and (out["idx"][b, n_s:] == -1).all()
        assert rel <= MEAN_BAR
        if pose:
            assert gap <= POSE_BAR
            worst = max(worst, gap)
        assert np.array_equal(out["T"][b, :3].view(np.uint32), out["T64"][b].astype(np.float32).view(np.uint32))       # T == float32(T64) bitwise
        assert out["status"][b] == p.get("status", 0)
    return worst


@pytest.mark.parametrize("fine", [False, True], ids=["tolerance_1e-3", "tolerance_1e-6"])
def test_all_goldens_in_one_batch_beside_a_failed_pair(fine):
    """Tolerance is an argument of the call: the batch runs once at 1e-3 and once at 1e-6 (where `all20` runs all 20 iterations); every
    golden holds the reference's result at both (and at its own)."""
    tag, tol = ("_fine", R.FINE_TOLERANCE) if fine else ("_coarse", R.TOLERANCE)
    pairs = [golden(n) for n in sorted(R.GOLDEN_CASES)]
    failed = dict(golden("noisy"), name="failed", status=2, T0=np.diag([1.0, 1.0, 1.0, 1.0]) + np.eye(4, k=3) * 0.25)
    pairs.insert(3, failed)
    pk = pack(pairs, cap_s=768, cap_d=800)                # larger than every n (<= 700): NaN beyond the counts
    out = run(pk, max_iter=20, tolerance=tol)
    rs = restate(pairs, 20, tol)
    worst = compare(out, pairs, rs, "goldens")
    ref_gap = 0.0
    for b, p in enumerate(pairs):
        if "status" in p:
            continue
        assert out["iters"][b] == int(p["g"]["iters" + tag])
        ref_gap = max(ref_gap, float(np.abs(out["T64"][b] - p["g"]["T" + tag]).max()))
    print(f"goldens at tolerance {tol:g}: |T64 - restatement| <= {worst:.2e}, |T64 - reference| <= {ref_gap:.2e}")
    assert ref_gap <= POSE_BAR
    if fine:
        assert out["iters"][sorted(R.GOLDEN_CASES).index("all20")] == 20
    # the failed pair: T_init and its status come back, nothing ran
    assert np.array_equal(out["T"][3], pk["T_init"][3].cpu().numpy()) and out["status"][3] == 2 and out["iters"][3] == 0
    assert out["n_kept"][3] == 0 and out["mean_err"][3] == 0.0 and (out["idx"][3] == -1).all()


def _moved(rng, n_s, n_d, angle=0.1, noise=0.0):
    """A source cloud and a target that holds its moved image (n_d >= n_s: plus other points of the surface; n_d < n_s: a part of it)."""
    A = R.object_cloud(rng, max(n_s, n_d))
    c = A.mean(axis=0)
    Rt, tt = R._rot(rng.normal(size=3), angle), rng.normal(size=3) * 0.004
    B = (A - c) @ Rt.T + c + tt + rng.normal(size=A.shape) * noise
    return dict(src=np.ascontiguousarray(A[:n_s]), dst=np.ascontiguousarray(B[rng.permutation(B.shape[0])[:n_d]]))


def test_shapes_where_the_kernel_can_go_wrong():
    """n_s around a wave (63, 64, 65), the smallest (3), one row past a workgroup's block, two blocks + 1; n_d at the tile, one past
    it, two tiles + 1; n = cap exactly on both sides (the last pair)."""
    rng = np.random.default_rng(77)
    shapes = [(3, 40), (63, TILE), (64, TILE + 1), (65, 2 * TILE + 1), (ROWS + 1, 300), (2 * ROWS + 1, 700), (2 * ROWS + 1, 2 * TILE + 1)]
    pairs = [dict(_moved(rng, ns, nd), name=f"{ns}x{nd}") for ns, nd in shapes]
    pk = pack(pairs)
    assert pk["src"].shape[1] == 2 * ROWS + 1 and pk["dst"].shape[1] == 2 * TILE + 1
    out = run(pk, max_iter=20, tolerance=1e-4)
    worst = compare(out, pairs, restate(pairs, 20, 1e-4), "shapes")
    print(f"shapes: |T64 - restatement| <= {worst:.2e}")


def test_one_target_row_and_max_iter_1():
    """n_d = 1: every row's neighbour is row 0, H = 0 and the rotation of the fit is free - what IS determined is that the fit moves
    the source's centroid onto the one target point.  max_iter = 1: one update, whatever the tolerance."""
    rng = np.random.default_rng(78)
    one = dict(_moved(rng, 65, 1), name="65x1")
    pairs = [one, golden("noisy"), golden("near")]
    out = run(pack(pairs), max_iter=1, tolerance=1e-3)
    rs = restate(pairs, 1, 1e-3, degenerate=(0,))
    for b in (1, 2):
        gap = float(np.abs(out["T64"][b] - rs[b]["T"][:3]).max())
        print(f"max_iter=1 [{b}]: |T64 - restatement| {gap:.2e}")
        assert out["iters"][b] == 1 == rs[b]["iters"] and gap <= POSE_BAR and np.array_equal(out["idx"][b, :pairs[b]["src"].shape[0]], rs[b]["idx"])
    assert out["iters"][0] == 1 and out["n_kept"][0] == 65 and (out["idx"][0, :65] == 0).all()
    moved = out["T64"][0][:, :3] @ one["src"].mean(axis=0) + out["T64"][0][:, 3]
    print(f"n_d = 1: |T c_src - dst_0| = {np.abs(moved - one['dst'][0]).max():.2e}")
    assert np.abs(moved - one["dst"][0]).max() <= POSE_BAR and np.isfinite(out["T64"][0]).all()


@pytest.mark.parametrize("names", [("identity",), ("identity", "all20", "noisy", "permuted", "near")], ids=["B1", "B5"])
def test_pairs_that_finish_at_different_iterations(names):
    """At tolerance 1e-6 the five pairs finish after 10, 20, 7, 6 and 4 iterations: done pairs sit beside running ones."""
    pairs = [golden(n) for n in names]
    out = run(pack(pairs), max_iter=20, tolerance=R.FINE_TOLERANCE)
    rs = restate(pairs, 20, R.FINE_TOLERANCE)
    assert len({r["iters"] for r in rs}) == len(names)
    compare(out, pairs, rs, "B%d" % len(names))


def few_rows_pair():
    """Three rows within max_dist = 0.0126 at the first iteration; its fit moves one of them out of reach: two at the second, which
    ends the pair with ONE update applied (seed found by search on the restatement)."""
    rng = np.random.default_rng(5213)
    dst = R.object_cloud(rng, 9)
    sc = rng.choice([0.004, 0.01, 0.02])
    src = dst[rng.permutation(9)[:6]] + rng.normal(size=(6, 3)) * sc
    return dict(src=src, dst=dst, name="few_rows")


def test_finite_max_dist_drops_rows_and_ends_a_pair_below_three():
    rng = np.random.default_rng(79)
    a = _moved(rng, 300, 340, angle=0.03, noise=0.001)
    a["src"] = np.concatenate([a["src"], a["src"][:9] + 0.3])        # nine rows 30 cm away: always beyond max_dist
    b = _moved(rng, 70, 50, angle=0.02)                              # the target holds only a part of the source's image
    pairs = [dict(a, name="outliers"), few_rows_pair(), dict(b, name="partial")]
    max_dist = 0.0126
    rs = restate(pairs, 20, 1e-5, max_dist)
    assert rs[0]["n_kept"] < 309 and rs[2]["n_kept"] < 70 and min(rs[0]["n_kept"], rs[2]["n_kept"]) >= 3          # rows are dropped
    assert rs[1]["n_kept_seq"] == [3, 2] and rs[1]["iters"] == 1                                               # below 3 at the 2nd iteration
    out = run(pack(pairs), max_iter=20, tolerance=1e-5, max_dist=max_dist)
    compare(out, pairs, rs, "max_dist")


def test_nan_rows_inside_the_counts():
    """A NaN target row never wins, a NaN source row has no neighbour (idx -1) and is dropped - on the device as in the restatement."""
    rng = np.random.default_rng(80)
    p = _moved(rng, 100, 130, angle=0.05)
    p["dst"][17] = np.nan
    p["src"][5] = np.nan
    rs = restate([p], 20, 1e-5)
    assert rs[0]["n_kept"] == 99 and rs[0]["idx"][5] == -1 and 17 not in rs[0]["idx"]
    compare(run(pack([p]), max_iter=20, tolerance=1e-5), [p], rs, "nan")


def test_bit_stable_across_runs_streams_and_batch_position():
    from oryon_amd import ops
    pairs = [golden(n) for n in ("identity", "noisy", "mirrored", "all20")]
    pk = pack(pairs, cap_s=768, cap_d=768)
    keys = ("T", "T64", "iters", "mean_err", "n_kept", "idx")
    first = run(pk, max_iter=20, tolerance=1e-6)
    again = run(pk, max_iter=20, tolerance=1e-6)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.icp_refine(pk["src"], pk["dst"], pk["n_src"], pk["n_dst"], pk["T_init"], max_iter=20, tolerance=1e-6, status=pk["status"],
                               want_idx=True)
    side.synchronize()
    other = {k: v.cpu().numpy() for k, v in other.items()}
    flipped = run({k: v.flip(0).contiguous() for k, v in pk.items()}, max_iter=20, tolerance=1e-6)
    for k in keys:
        assert first[k].tobytes() == again[k].tobytes(), k
        assert first[k].tobytes() == other[k].tobytes(), k
        assert first[k].tobytes() == flipped[k][::-1].tobytes(), k


def test_geo6d_facade_against_the_goldens():
    from oryon_amd import geo6d
    worst = 0.0
    for name in sorted(R.GOLDEN_CASES):
        p = golden(name)
        g = p["g"]
        T = geo6d.icp(g["A"], g["B"], init_pose=p["T0"], max_iterations=int(g["max_iterations"]), tolerance=float(g["tolerance"]))
        assert T.shape == (3, 4) and T.dtype == np.float64
        worst = max(worst, float(np.abs(T - g["T"]).max()))
        # the reference's closing line: the fit of A onto its moved image IS the pose
        moved = g["A"] @ g["T"][:, :3].T + g["T"][:, 3]
        F = geo6d.best_fit_transform_icp(g["A"], moved)
        assert F.shape == (4, 4) and np.array_equal(F[3], [0.0, 0.0, 0.0, 1.0])
        worst = max(worst, float(np.abs(F[:3] - g["T"]).max()))
        Fr = R.best_fit_transform_icp(g["A"], g["B"])                    # and a fit that is no identity pairing of a rigid image
        assert np.abs(geo6d.best_fit_transform_icp(g["A"], g["B"]) - Fr).max() <= POSE_BAR
    print(f"facade: |T - reference| <= {worst:.2e}")
    assert worst <= POSE_BAR
    unequal = geo6d.icp(golden("noisy")["src"][:500], golden("noisy")["dst"], tolerance=1e-3)          # lengths need not be equal
    assert np.abs(unequal - R.icp(golden("noisy")["src"][:500], golden("noisy")["dst"], None, 20, 1e-3)["T"][:3]).max() <= POSE_BAR


def test_icp_refine_rejects_tensors_it_would_have_to_convert():
    from oryon_amd import ops
    pk = pack([golden("near")])
    args = lambda **kw: [dict(pk, **kw)[k] for k in ("src", "dst", "n_src", "n_dst", "T_init")]
    wide = torch.zeros(1, 64, 6, dtype=torch.float64, device="cuda")
    for change, name in ((dict(src=pk["src"].float()), r"src\.dtype == float64"), (dict(dst=pk["dst"].half()), r"dst\.dtype == float64"),
                         (dict(src=wide[:, :, :3]), r"src\.is_contiguous"), (dict(dst=wide[:, :, 3:]), r"dst\.is_contiguous"),
                         (dict(n_src=pk["n_src"].long()), "n_src is"), (dict(n_dst=pk["n_dst"][None]), "n_dst is"),
                         (dict(T_init=pk["T_init"].double()), r"T_init\.dtype == float32"), (dict(T_init=pk["T_init"][:, :3]), r"T_init\.shape"),
                         (dict(T_init=pk["T_init"].transpose(1, 2)), r"T_init\.is_contiguous"), (dict(src=pk["src"].cpu()), r"src\.is_cuda"),
                         (dict(dst=pk["dst"][:, :, :2].contiguous()), r"dst\.shape")):
        with pytest.raises(ValueError, match="icp_refine: " + name):
            ops.icp_refine(*args(**change))
    for kw, name in ((dict(max_iter=0), "max_iter"), (dict(tolerance=-1.0), "tolerance >= 0"), (dict(max_dist=float("nan")), "max_dist >= 0"),
                     (dict(status=pk["status"].long()), "status is")):
        with pytest.raises(ValueError, match="icp_refine: .*" + name):
            ops.icp_refine(*args(), **kw)
    with pytest.raises(ValueError, match="cap <= 8192"):
        ops.icp_refine(torch.zeros(1, 8193, 3, dtype=torch.float64, device="cuda"), pk["dst"], pk["n_src"], pk["n_dst"], pk["T_init"])


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
    batch = {
        "featmap_a": st("feat_a").to(dev), "featmap_q": st("feat_q").to(dev),
        "anchor": {"mask": st("mask_a").to(torch.uint8), "orig_depth": [p["depth_a"] for p in pairs], "camera": st("camera"),
                   "pose": anchor_pose, "instance_id": [f"s {i} a" for i in idx], "sizes": torch.tensor([[H, H]] * B)},
        "query": {"mask": st("mask_q").to(torch.uint8), "orig_depth": [p["depth_q"] for p in pairs], "camera": st("camera"),
                  "pose": st("pose").float(), "instance_id": [f"s {i} q" for i in idx], "sizes": torch.tensor([[H, H]] * B)},
        "instance_id": [f"s {i}" for i in idx], "cls_id": [1] * B,
    }
    return batch, pairs


def _pipeline(H=48, **test_flags):
    from oryon_amd.pipeline import Pipeline, default_args
    args = default_args(**{"test.mask": "oracle", "model.image_encoder.img_size": [H, H], "dataset.img_size": [H, H]})
    for k, v in test_flags.items():
        setattr(args.test, k, v)
    return Pipeline(args, pointdsc_solver=_solver())


@pytest.fixture(scope="module")
def unrefined():
    """The poses of a Pipeline that has never heard of test.refine: per-sample records and the batched step's output, computed once."""
    batch, _ = _batch([3, 4, 5])
    pl = _pipeline()
    torch.manual_seed(1)
    recs = pl.test_step(batch, 0)
    out = pl.test_step_batched(batch)
    return dict(recs=recs, pose=out["pose"].clone(), status=out["status"].clone(), lines=list(pl.pred_lines))


def test_refine_none_is_todays_behaviour_byte_for_byte(unrefined):
    batch, _ = _batch([3, 4, 5])
    pl = _pipeline(refine="none")
    torch.manual_seed(1)
    recs = pl.test_step(batch, 0)
    out = pl.test_step_batched(batch)
    for a, b in zip(recs, unrefined["recs"]):
        assert a["status"] == b["status"] and a["pred_pose_rel"].numpy().tobytes() == b["pred_pose_rel"].numpy().tobytes()
    assert out["pose"].cpu().numpy().tobytes() == unrefined["pose"].cpu().numpy().tobytes() and torch.equal(out["status"], unrefined["status"])
    assert pl.pred_lines == unrefined["lines"] and "pose_unrefined" not in out and pl.last_refine is None


def _hand_clouds(pl, batch, b, dev="cuda"):
    depth_a = batch["anchor"]["orig_depth"][b].squeeze().to(dev, torch.float32)[None].contiguous()
    depth_q = batch["query"]["orig_depth"][b].squeeze().to(dev, torch.float32)[None].contiguous()
    return pl.refine_clouds(batch["anchor"]["mask"][b:b + 1].to(dev), batch["query"]["mask"][b:b + 1].to(dev), depth_a, depth_q,
                            batch["anchor"]["camera"][b:b + 1].to(dev), batch["query"]["camera"][b:b + 1].to(dev),
                            torch.tensor([b], dtype=torch.int64, device=dev))


def test_refine_icp_per_sample_is_icp_refine_by_hand(unrefined):
    from oryon_amd import ops
    batch, _ = _batch([3, 4, 5])
    pl = _pipeline(refine="icp", refine_points=512)                  # 48 x 48 maps: the masks hold ~600 / ~2000 pixels, so 512 subsamples
    torch.manual_seed(1)
    recs = pl.test_step(batch, 0)
    for b, (rec, base) in enumerate(zip(recs, unrefined["recs"])):
        assert rec["status"] == base["status"] == 0
        c = _hand_clouds(pl, batch, b)
        assert int(c["n_src"][0]) == 512 or int(c["n_dst"][0]) == 512                                  # the subsample took place
        hand = ops.icp_refine(c["src"], c["dst"], c["n_src"], c["n_dst"], base["pred_pose_rel"][None].cuda().contiguous(), max_iter=20,
                              tolerance=1e-3)
        assert int(hand["iters"][0]) >= 1
        assert hand["T"][0].cpu().numpy().tobytes() == rec["pred_pose_rel"].numpy().tobytes()
        assert not torch.equal(rec["pred_pose_rel"], base["pred_pose_rel"])
        np.testing.assert_allclose(rec["pred_pose"].numpy(), rec["pred_pose_rel"].numpy() @ batch["anchor"]["pose"][b].numpy(), atol=1e-6)


def test_refine_icp_batched_agrees_with_per_sample_and_leaves_failed_pairs_alone(monkeypatch):
    """The batched step against the per-sample loop (test_step -> get_pose), both with test.refine = icp, from the SAME solver pose:
    same iteration counts, poses within 1e-6.  The two routes' own solver poses are not the same pose - the per-sample matcher draws
    its correspondences from the host generator, the engine from the device's (measured here: they differ by 2.6e-3 to 4.4e-3 per
    entry) - and two ICP runs from starts that far apart, stopped at tolerance 1e-3 after two iterations, differ by 1.4e-4 to 1.9e-3:
    that difference is the solvers', not the refinement's.  So the per-sample loop's solver call is answered with the engine's
    unrefined pose of the same pair; everything this feature adds to the per-sample route - masks, the keyed subsample, the lift, the
    one-pair ICP call - runs as it is.  The unmodified routes' figures are printed first."""
    import oryon_amd.pipeline as pipeline_module
    batch, _ = _batch([3, 4, 5, 6])
    batch["anchor"]["mask"][2] = 0                       # NO_MASK
    pl = _pipeline(refine="icp", refine_points=512)
    out = pl.test_step_batched(batch)
    iters = out["refine_iters"].cpu().tolist()
    assert out["status"].cpu().tolist() == [0, 0, 1, 0]
    assert torch.equal(out["pose"][2].cpu(), torch.eye(4)) and iters[2] == 0 and torch.equal(out["pose_unrefined"][2].cpu(), torch.eye(4))
    torch.manual_seed(1)
    own = pl.test_step(batch, 0)
    for b in (0, 1, 3):
        print(f"pair {b}, each route from its own solver pose: iters per-sample {own[b]['refine_iters']} / batched {iters[b]}, |pose difference| "
              f"{float((own[b]['pred_pose_rel'] - out['pose'][b].cpu()).abs().max()):.2e}")
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
    np.testing.assert_allclose(out["pred_q"][0].cpu().numpy(), out["pose"][0].cpu().numpy() @ batch["anchor"]["pose"][0].numpy(), atol=1e-6)


def test_run_pose_parses_refine_and_an_unknown_refinement_raises():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_pose
    assert run_pose.parse(["--refine", "icp", "--pairs", "2", "--solver", "ransac"]) == ("ransac", ["--pairs", "2"])
    assert run_pose.take_refine(["--refine", "icp", "--pairs", "2", "--solver", "ransac"])[0] == "icp"
    with pytest.raises(RuntimeError, match="Refinement gicp not implemented"):
        _pipeline(refine="gicp")
