"""GPU tests of the RANSAC pose solver (csrc/ransac.hip, test.solver = ransac): the C entry point against the float64 restatement
and the reference's recorded poses on every fixture, the device RNG, the geo6d facade (pose and numpy generator state), both
Pipeline routes and the step engine.

max_iter, match_err and fix_percent are per-call arguments, so fixtures that differ in them cannot share a launch: fixtures 1, 3,
5 and 6 (K = 256, reference parameters; n = 500, 64, 500, 3) run as ONE batch together with a pair that arrives with a failure
status; fixtures 2, 4 and 7 run as calls of their own."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import ransac_restatement as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5          # pose entries against the reference's golden (the bar of PointDSC's seed transforms)


@functools.lru_cache(maxsize=None)
def fixtures():
    """name -> fixture arrays + the restatement's result (computed once, shared, never modified)."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ransac_*.npz"))):
        z = np.load(path)
        f = dict(A=z["A"], B=z["B"], idx=z["idx"], max_iter=int(z["max_iter"]), match_err=float(z["match_err"]),
                 fix_percent=float(z["fix_percent"]), pose=z["pose"], seed=int(z["seed"]), state_words=z["state_words"],
                 state_pos=int(z["state_pos"]))
        f["r"] = rr.restate(f["A"], f["B"], f["idx"], f["max_iter"], f["match_err"], f["fix_percent"])
        f["bad"] = rr.rank_deficient(f["idx"], f["max_iter"])
        out[os.path.basename(path)[len("ransac_"):-len(".npz")]] = f
    assert len(out) == 7
    return out


def _pack(fs, n_cap, extra=0):
    """Rows of the fixtures `fs` (+ `extra` all-NaN pairs) as [B,n_cap,3] tensors; rows past a pair's n are NaN: a kernel that read
    one would count wrongly or return a NaN pose."""
    B = len(fs) + extra
    src = torch.full((B, n_cap, 3), float("nan"))
    tgt = torch.full((B, n_cap, 3), float("nan"))
    n = torch.zeros(B, dtype=torch.int32)
    K = fs[0]["max_iter"]
    idx = torch.zeros((B, K, 4), dtype=torch.int32)
    for b, f in enumerate(fs):
        m = f["A"].shape[0]
        src[b, :m], tgt[b, :m], n[b] = torch.from_numpy(f["A"]), torch.from_numpy(f["B"]), m
        idx[b] = torch.from_numpy(f["idx"])
    return src.cuda(), tgt.cuda(), n.cuda(), idx.cuda()


def _check_against_restatement(name, f, T, winner, exited, counts):
    r = f["r"]
    T = T.cpu().numpy().astype(np.float64)
    assert int(winner) == r["winner"] and bool(int(exited)) == r["exited"], (name, int(winner), r["winner"], int(exited))
    if f["A"].shape[0] >= 4:
        keep = ~f["bad"]
        got = counts.cpu().numpy()
        print(f"{name}: {int(f['bad'].sum())} of {f['max_iter']} hypotheses excluded as rank-deficient; "
              f"{int((got[keep] != r['counts'][keep]).sum())} counts differ; max |T - golden| = {np.abs(T[:3] - f['pose']).max():.3e}")
        assert f["bad"].sum() <= (0.02 if name == "7_workload" else 0.10) * f["max_iter"]      # the bound on what the comparison leaves out
        assert np.array_equal(got[keep], r["counts"][keep]), name
    assert np.abs(T[:3] - f["pose"]).max() <= TOL, name
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    if r["winner"] < 0:
        assert not T[:3].any(), name                                   # the exact zero pose, placed in eye(4)


def test_register_on_the_batch_of_fixtures():
    from oryon_amd import ops
    fx = fixtures()
    names = ["1_best_of_k", "3_exit_at_0", "5_all_zero", "6_n3"]
    fs = [fx[k] for k in names]
    assert len({(f["max_iter"], f["match_err"], f["fix_percent"]) for f in fs}) == 1
    src, tgt, n, idx = _pack(fs, 512, extra=1)
    # the fifth pair arrives with a failure status (its rows are all NaN and its n is 0): identity, status passed through
    status = torch.tensor([0, 0, 0, 0, 2], dtype=torch.int32, device="cuda")
    out = ops.ransac_register(src, tgt, n, fs[0]["max_iter"], fs[0]["match_err"], fs[0]["fix_percent"], idx, status=status, want_counts=True)
    torch.cuda.synchronize()
    for b, (name, f) in enumerate(zip(names, fs)):
        _check_against_restatement(name, f, out["T"][b], out["winner"][b], out["exited"][b], out["counts"][b])
    assert out["status"].tolist() == [0, 0, 0, 0, 2]
    assert torch.equal(out["T"][4].cpu(), torch.eye(4)) and int(out["winner"][4]) == -1 and int(out["exited"][4]) == 0


@pytest.mark.parametrize("name,n_cap", [("2_exit_sampled", 256), ("4_n37", 37), ("7_workload", 500)])
def test_register_on_the_other_fixtures(name, n_cap):
    """An exit at a sampled hypothesis followed by the refit; n = 37 in a buffer of exactly n rows (no multiple of anything); one pair
    at the workload's own size (10 000 iterations: 40 blocks per pair, the atomics across blocks decide)."""
    from oryon_amd import ops
    f = fixtures()[name]
    src, tgt, n, idx = _pack([f], n_cap)
    out = ops.ransac_register(src, tgt, n, f["max_iter"], f["match_err"], f["fix_percent"], idx, want_counts=True)
    torch.cuda.synchronize()
    _check_against_restatement(name, f, out["T"][0], out["winner"][0], out["exited"][0], out["counts"][0])
    assert out["status"].tolist() == [0]


def test_points_inside_the_fp32_band_are_decided_in_float64():
    """The scoring loop tests a point in fp32 against two thresholds around match_err and decides what falls between them in fp64.
    No fixture has such a point (they keep 1e-6 m clear of match_err), so this case puts match_err 1e-9 m above, then 1e-9 m below,
    the float64 error of one inlier of the winning hypothesis: far inside the fp32 band (about 1.7e-6 m here), far outside what
    float64 rounding and the Jacobi-vs-LAPACK difference of the fits can move (1e-13 m).  Counts must follow float64 both times."""
    from oryon_amd import ops
    f = fixtures()["1_best_of_k"]
    r = f["r"]
    k = r["winner"]
    i = int(np.argsort(r["err"][k])[150])                              # a mid-range inlier of the winner
    src, tgt, n, idx = _pack([f], 512)
    seen = []
    for me in (r["err"][k, i] + 1e-9, r["err"][k, i] - 1e-9):
        want = (r["err"] <= me).sum(1)
        clear = (np.abs(r["err"] - me) > 1e-11).all(1) | (np.arange(f["max_iter"]) == k)
        clear &= ~f["bad"]
        out = ops.ransac_register(src, tgt, n, f["max_iter"], float(me), f["fix_percent"], idx, want_counts=True)
        got = out["counts"][0].cpu().numpy()
        assert np.array_equal(got[clear], want[clear])
        seen.append(int(got[k]))
    assert seen[0] == seen[1] + 1 == 151


def test_row_limit_is_an_argument_error():
    from oryon_amd import _lib, ops
    z = torch.zeros((1, 2176, 3), device="cuda")
    with pytest.raises(_lib.OryonError):
        ops.ransac_register(z, z, torch.tensor([2176], dtype=torch.int32, device="cuda"), 16)


def test_device_rng_matches_its_restatement_and_ignores_sharding():
    from oryon_amd import ops
    fx = fixtures()
    fs = [fx["1_best_of_k"], fx["4_n37"], fx["3_exit_at_0"]]
    K, seed = 256, 12345
    src = torch.full((3, 512, 3), float("nan"))
    tgt = torch.full((3, 512, 3), float("nan"))
    for b, f in enumerate(fs):
        m = f["A"].shape[0]
        src[b, :m], tgt[b, :m] = torch.from_numpy(f["A"]), torch.from_numpy(f["B"])
    src, tgt = src.cuda(), tgt.cuda()
    ns = [f["A"].shape[0] for f in fs]
    n = torch.tensor(ns, dtype=torch.int32, device="cuda")
    keys = [5, 9, 1000]
    key = torch.tensor(keys, dtype=torch.int64, device="cuda")
    table = torch.from_numpy(np.stack([rr.device_sample_idx(seed, k, m, K) for k, m in zip(keys, ns)])).cuda()
    kw = dict(max_iter=K, match_err=0.001, fix_percent=0.9999, seed=seed, want_counts=True)
    a = ops.ransac_register(src, tgt, n, sample_idx=None, pair_key=key, **kw)
    t = ops.ransac_register(src, tgt, n, sample_idx=table, pair_key=key, **kw)
    a2 = ops.ransac_register(src, tgt, n, sample_idx=None, pair_key=key, **kw)
    for k in ("T", "winner", "exited", "counts", "status"):
        assert torch.equal(a[k], t[k]), k                              # the device draws the table its restatement draws: same bits
        assert torch.equal(a[k], a2[k]), k                             # and draws it again
    assert a["winner"].min() >= 0 and (a["counts"].max(1).values >= 15).all()       # real hypotheses won, not the zero pose
    # two shards with the keys carried along give the same rows
    parts = [ops.ransac_register(src[s], tgt[s], n[s], sample_idx=None, pair_key=key[s], **kw) for s in (slice(0, 1), slice(1, 3))]
    for k in ("T", "winner", "counts"):
        assert torch.equal(torch.cat([p[k] for p in parts]), a[k]), k
    # without keys the pair index is the key
    d = ops.ransac_register(src, tgt, n, sample_idx=None, pair_key=None, **kw)
    e = ops.ransac_register(src, tgt, n, sample_idx=None, pair_key=torch.arange(3, dtype=torch.int64, device="cuda"), **kw)
    assert torch.equal(d["T"], e["T"]) and torch.equal(d["counts"], e["counts"]) and not torch.equal(d["counts"], a["counts"])


@pytest.mark.parametrize("name", ["1_best_of_k", "2_exit_sampled", "3_exit_at_0"])
def test_geo6d_facade_pose_and_generator_state(name):
    """best_fit_transform_with_RANSAC under np.random.seed(s): the golden's pose, and numpy's global generator left exactly where
    the reference's run left it (no exit: max_iter draws; exit at iteration k: k draws)."""
    from oryon_amd import geo6d
    f = fixtures()[name]
    saved = np.random.get_state()
    try:
        np.random.seed(f["seed"])
        pose = geo6d.best_fit_transform_with_RANSAC(f["A"], f["B"], f["max_iter"], f["match_err"], f["fix_percent"])
        state = np.random.get_state()
    finally:
        np.random.set_state(saved)
    assert isinstance(pose, np.ndarray) and pose.shape == (3, 4)
    assert np.abs(pose - f["pose"]).max() <= TOL
    assert np.array_equal(state[1][:8], f["state_words"]) and int(state[2]) == f["state_pos"]


def test_geo6d_best_fit_transform_and_short_input():
    from oryon_amd import geo6d
    f = fixtures()["3_exit_at_0"]
    want = rr.fit(f["A"], f["B"])
    assert np.abs(geo6d.best_fit_transform(f["A"], f["B"]) - want).max() <= TOL
    assert np.abs(geo6d.best_fit_transform(torch.from_numpy(f["A"][:3]), torch.from_numpy(f["B"][:3])) - rr.fit(f["A"][:3], f["B"][:3])).max() <= TOL
    z = geo6d.best_fit_transform_with_RANSAC(f["A"][:3], f["B"][:3])
    assert z.shape == (3, 4) and not z.any()


# ------------------------------------------------------------------------------------------------ callers
def _pointdsc(L=2, C=32):
    from oracle import oryon_oracle as orc
    from oryon_amd.pointdsc import PointDSC
    m = PointDSC(in_dim=6, num_layers=L, num_channels=C, num_iterations=10, ratio=0.1, sigma_d=0.1, k=40, nms_radius=0.1)
    m.load_state_dict(orc.analytic_pointdsc_params(L, C), strict=True)
    return m.cuda().eval()


def _batch(first, B, H=48, C=32, dev="cuda"):
    """Two-sided batch dict of Pipeline.test_step from synth.make_batch."""
    from oryon_amd.synth import make_batch
    mb = make_batch(first, B, H, H, C)
    anchor_pose = torch.eye(4).repeat(B, 1, 1)
    anchor_pose[:, :3, 3] = torch.tensor([0.01, -0.02, 0.8])
    idx = list(range(first, first + B))
    return {
        "featmap_a": mb["feat_a"].to(dev), "featmap_q": mb["feat_q"].to(dev),
        "anchor": {"mask": mb["mask_a"].to(torch.uint8), "orig_depth": list(mb["depth_a"]), "camera": mb["camera"], "pose": anchor_pose,
                   "instance_id": [f"s {i} a" for i in idx], "sizes": torch.tensor([[H, H]] * B)},
        "query": {"mask": mb["mask_q"].to(torch.uint8), "orig_depth": list(mb["depth_q"]), "camera": mb["camera"], "pose": mb["pose"].float(),
                  "instance_id": [f"s {i} q" for i in idx], "sizes": torch.tensor([[H, H]] * B)},
        "instance_id": [f"s {i}" for i in idx], "cls_id": [1] * B,
    }, mb


def _ransac_pipeline(H=48):
    from oryon_amd.pipeline import Pipeline, default_args
    args = default_args(**{"test.mask": "oracle", "test.solver": "ransac", "model.image_encoder.img_size": [H, H], "dataset.img_size": [H, H]})
    return Pipeline(args, pointdsc_solver=None)


def test_pipeline_per_sample_route_runs_the_ransac_solver():
    pl = _ransac_pipeline()
    batch, _ = _batch(3, 2)
    torch.manual_seed(1)
    saved = np.random.get_state()
    try:
        np.random.seed(1)
        recs = pl.test_step(batch, 0)
    finally:
        np.random.set_state(saved)
    assert [r["status"] for r in recs] == [0, 0]
    for r in recs:
        T = r["pred_pose_rel"]
        assert T.dtype == torch.float32 and T.shape == (4, 4) and T[3].tolist() == [0.0, 0.0, 0.0, 1.0] and bool(torch.isfinite(T).all())
    assert len(pl.pred_lines) == 2


def test_pipeline_batched_route_equals_the_entry_point_bit_for_bit():
    from oryon_amd import ops
    pl = _ransac_pipeline()
    first, B = 20, 3
    batch, _ = _batch(first, B)
    batch["anchor"]["mask"][2] = 0                                       # pair 2: NO_MASK -> identity, status 1
    out = pl.test_step_batched(batch, first_pair_index=first)
    torch.cuda.synchronize()
    nat = pl._engine._native
    assert nat is not None and nat.ecfg.solver == 1
    slot = (nat.steps - 1) % nat.n_slots
    key = torch.arange(first, first + B, dtype=torch.int64, device="cuda")
    # (the engine's thresholds are the float32 values of its configuration struct, widened: 0.001f, 0.9999f)
    want = ops.ransac_register(nat.view(slot, "pcd_a"), nat.view(slot, "pcd_q"), nat.view(slot, "n_lift"), 10000, nat.ecfg.ransac_match_err,
                               nat.ecfg.ransac_fix_percent, None, pl.args.seed, key, nat.view(slot, "status"))
    assert nat.ecfg.ransac_match_err == np.float32(0.001) and nat.ecfg.ransac_fix_percent == np.float32(0.9999)
    assert torch.equal(out["pose"], want["T"]) and torch.equal(out["status"], want["status"])
    assert out["status"].tolist() == [0, 0, 1] and torch.equal(out["pose"][2].cpu(), torch.eye(4))
    assert (want["winner"][:2] >= 0).all()                               # a hypothesis with inliers won: not the zero pose
    # the per-call schedule (native=False) is the same computation
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    eng = MatchPoseEngine(None, MatchPoseConfig(solver="ransac", seed=pl.args.seed), native=False)
    stack = lambda x: torch.stack([d.squeeze() for d in x]).cuda().float().contiguous()
    mask = lambda m: ops.mask_resize_nearest(m.cuda(), (48, 48))
    o2 = eng.run(batch["featmap_a"], batch["featmap_q"], mask(batch["anchor"]["mask"]), mask(batch["query"]["mask"]),
                 stack(batch["anchor"]["orig_depth"]), stack(batch["query"]["orig_depth"]), batch["anchor"]["camera"].cuda(),
                 batch["query"]["camera"].cuda(), key)
    assert torch.equal(o2["pose"], out["pose"]) and torch.equal(o2["status"], out["status"])


def test_pointdsc_engine_is_unchanged_next_to_a_ransac_engine():
    """A PointDSC engine created AFTER a RANSAC engine of the same process (same stream pool, a differently carved arena before it)
    gives the poses a PointDSC engine gave before."""
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    from oryon_amd.synth import make_batch
    mb = make_batch(30, 3, 48, 48, 32, device="cuda")
    cam = mb["camera"].cuda()
    run = lambda eng: eng.run(mb["feat_a"], mb["feat_q"], mb["mask_a"], mb["mask_q"], mb["depth_a"], mb["depth_q"], cam, cam)
    solver = _pointdsc()
    before = run(MatchPoseEngine(solver, MatchPoseConfig()))
    ransac = run(MatchPoseEngine(None, MatchPoseConfig(solver="ransac")))
    after = run(MatchPoseEngine(solver, MatchPoseConfig()))
    torch.cuda.synchronize()
    assert before["status"].tolist() == [0, 0, 0] and ransac["status"].tolist() == [0, 0, 0]
    assert torch.equal(before["pose"], after["pose"]) and torch.equal(before["status"], after["status"])
    assert not torch.equal(ransac["pose"], before["pose"])
