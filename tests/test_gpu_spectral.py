"""GPU tests of the spectral pose solver (csrc/spectral.hip, test.solver = spectral) through oryon_spectral_stages /
oryon_spectral_register, geo6d.spectral_pose, MatchPoseEngine and Pipeline, against the float64 restatement
(tests/spectral_restatement.py).  Inputs sit in padded buffers whose tails - the rows >= n of every pair included - hold NaN; outputs
sit in guarded buffers.  Every new stage is checked on the DEVICE's own upstream output, so no pair is ever skipped:

  compat   the restatement's bits, exactly (float64 without contraction on both sides).
  conf     max |got - want| / max |want| <= R = 4 R_REF (R_REF: numpy float32 against float64, test_spectral_restatement.r_ref).  Two
           correct fp32 evaluations differ in summation order and in the rounding of M's entries; that is all the factor covers.
  seeds    pdsc_restatement.seeds on the device's conf; the kernel is PointDSC's, unchanged: a mismatch is tolerated only when that
           helper reports a distance within NEAR of the radius (its margin rule).  The count is printed.
  scores   C . (C C) on the device's seeds, exactly; sets: exactly, tie order included (ties are the normal case: printed).
  Mmat     |got - want| <= u (8 + 8 (a + b) |d| / sigma^2), u = 2^-24, a = |s_i - s_j|, b = |t_i - t_j|, d = a - b, per entry.  Derivation
           (the file is built without contraction, so every fp32 operation rounds once, relative error <= u): a coordinate difference
           u; its square 3 u; the sum of three squares 5 u; the root 3.5 u: |a_f - a| <= 3.5 u a, likewise b; d_f = fl(a_f - b_f):
           |d_f - d| <= 3.5 u (a + b) + u |d|.  t = d^2 / sigma^2 is formed as fl(fl(d_f d_f) fl(1 / fl(sigma sigma))): 4 u relative on
           top of (2 |d| |d_f - d|) / sigma^2, and 1 - t rounds once more (u, as |1 - t| <= 1 wherever an entry is not clamped;
           max(0, .) is 1-Lipschitz).  First order: u (1 + 6 t + 7 (a + b) |d| / sigma^2) with t <= 1; 8 and 8 leave room for the
           second-order terms.  Not fitted: the measured worst ratio to the bound is printed.
  tail     with stop = the device's stopping iteration (the first at which every seed's `close` flag is set, else the last), from the
           device's sets: fitness equals the restatement's count up to the rows within NEAR of the threshold, for every seed whose
           weighted covariance is well conditioned (s2 > 1e-2 s1; the transform of a degenerate set - an outlier seed whose members do
           not agree - is not determined, in float64 either) and seed_T within 1e-4 there; every seed's fitness equals the float64
           count under the DEVICE's own transform up to the NEAR rows; best is the first maximum of the device's fitness; T0 is
           seed_T[best], bytes.
  T        the planted-pose bars of test_spectral_restatement.py (1 degree, 3 mm); register == stages, bytes; two runs, a pair alone
           or at any position of a batch, a side stream: bytes."""
import functools

import numpy as np
import pytest
import torch

import pdsc_restatement as pr
import spectral_restatement as sr
from test_spectral_restatement import ROT_BAR_DEG, TRANS_BAR_M, r_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
CFG = sr.DEFAULTS
U24 = 2.0 ** -24


def padded(real: torch.Tensor, fill, extra=4096):
    """`real` as a contiguous view at the start of a larger buffer whose tail holds `fill`."""
    buf = torch.full((real.numel() + extra,), fill, dtype=real.dtype, device=DEV)
    buf[:real.numel()] = real.flatten().to(DEV)
    return buf[:real.numel()].view(real.shape)


def sentinel(dtype):
    return -7.5 if dtype.is_floating_point else -7


def guarded(shape, dtype):
    """-> (a contiguous view of `shape` holding the sentinel, the whole buffer): the GUARD elements behind the view must keep it."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), sentinel(dtype), dtype=dtype, device=DEV)
    return buf[:n].view(shape), buf


def stage_shapes(B, n_cap, cfg=CFG):
    S_cap, k, nit = int(n_cap * pr.f32(cfg["ratio"])) + 1, cfg["k"], cfg["num_iterations"]
    i32, f32 = torch.int32, torch.float32
    return dict(compat=(i32, (B, n_cap, n_cap // 32)), conf=(f32, (B, n_cap)), seeds=(i32, (B, S_cap)), n_seeds=(i32, (B,)),
                sets=(i32, (B, S_cap, k)), scores=(i32, (B, S_cap, n_cap)), Mmat=(f32, (B, S_cap, k, k)), close=(i32, (B, S_cap, nit)),
                seed_T=(f32, (B, S_cap, 4, 4)), fitness=(f32, (B, S_cap)), best=(i32, (B,)), T0=(f32, (B, 4, 4)), T=(f32, (B, 4, 4)),
                status=(i32, (B,)))


def pack(pairs, n_cap):
    """[(src [n,3], tgt [n,3])] -> NaN-filled [B,n_cap,3] x2 in padded device buffers + n [B]."""
    B = len(pairs)
    src = torch.full((B, n_cap, 3), float("nan"))
    tgt = torch.full((B, n_cap, 3), float("nan"))
    for b, (s, t) in enumerate(pairs):
        src[b, :len(s)], tgt[b, :len(s)] = torch.from_numpy(s), torch.from_numpy(t)
    n = torch.tensor([len(s) for s, _ in pairs], dtype=torch.int32)
    return padded(src, float("nan")), padded(tgt, float("nan")), padded(n, 1 << 20)


def run_stages(pairs, n_cap, status=None, stream=None):
    """ops.spectral_stages into guarded buffers -> {name: numpy array}; the guards are checked here."""
    from oryon_amd import ops
    src, tgt, n = pack(pairs, n_cap)
    bufs = {k: guarded(shape, dt) for k, (dt, shape) in stage_shapes(len(pairs), n_cap).items()}
    st = None if status is None else padded(torch.tensor(status, dtype=torch.int32), 0)
    if stream is None:
        ops.spectral_stages(src, tgt, n, st, out={k: v[0] for k, v in bufs.items()})
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ops.spectral_stages(src, tgt, n, st, out={k: v[0] for k, v in bufs.items()})
    torch.cuda.synchronize()
    for k, (view, buf) in bufs.items():
        assert bool((buf[view.numel():] == sentinel(buf.dtype)).all()), f"{k}: wrote past its end"
    return {k: v[0].cpu().numpy() for k, v in bufs.items()}


SHAPES = {
    "3x128": (128, [(128, 0.5, 10), (65, 0.5, 11), (24, 0.5, 0)]),
    "2x256": (256, [(129, 0.5, 0), (200, 0.7, 0)]),
    "2x512": (512, [(500, 0.8, 0), (512, 0.8, 12)]),
    "1x2048": (2048, [(2048, 0.9, 0)]),
}


@functools.lru_cache(maxsize=None)
def shape_inputs(name):
    n_cap, specs = SHAPES[name]
    made = [sr.planted(n, of, seed) for n, of, seed in specs]
    return n_cap, [(m[0], m[1]) for m in made], [m[2] for m in made]


@functools.lru_cache(maxsize=None)
def shape_run(name):
    """The device's stages on one of SHAPES: computed once, shared, never modified."""
    n_cap, pairs, _ = shape_inputs(name)
    return run_stages(pairs, n_cap)


def covariance_ratio(A, B, w):
    """s2 / s1 of the weighted covariance Kabsch decomposes (0 when it vanishes)."""
    w = np.where(w < 0, 0.0, w)
    den = w.sum() + 1e-6
    ca, cb = (A * w[:, None]).sum(0) / den, (B * w[:, None]).sum(0) / den
    s = np.linalg.svd((A - ca).T @ (w[:, None] * (B - cb)), compute_uv=False)
    return float(s[1] / s[0]) if s[0] > 0 else 0.0


def check_pair(tag, src, tgt, n_cap, r, b, G=None):
    """Every stage of pair b of the device result r against the restatement run on the device's own upstream output."""
    n = len(src)
    k, nit, tau, sig = CFG["k"], CFG["num_iterations"], CFG["inlier_threshold"], CFG["sigma_d"]
    S = int(n * pr.f32(CFG["ratio"]))
    kk = min(k, n - 1)
    s64, t64 = src.astype(np.float64), tgt.astype(np.float64)
    # S1
    C, _ = sr.compat(src, tgt, tau)
    assert np.array_equal(r["compat"][b].view(np.uint32), sr.pack_bits(C, n_cap)), f"{tag}: compat bits"
    # S2
    want = sr.confidence(src, tgt, sig, nit)
    got = r["conf"][b].astype(np.float64)
    assert np.isfinite(got).all() and not got[n:].any()
    ratio = float(np.abs(got[:n] - want).max() / np.abs(want).max())
    R = 4 * r_ref()
    # S3
    assert int(r["n_seeds"][b]) == S
    seeds = r["seeds"][b, :S].astype(np.int64)
    sd = pr.seeds(src, r["conf"][b, :n], CFG["nms_radius"], S)
    seed_mismatch = int((seeds != sd["seeds"]).sum())
    # S4
    assert len(set(seeds.tolist())) == S and (seeds >= 0).all() and (seeds < n).all()
    want_scores = np.zeros((S, n_cap), np.int64)
    want_scores[:, :n] = sr.scores(C, seeds)
    assert np.array_equal(r["scores"][b, :S], want_scores), f"{tag}: scores"
    want_sets, ties = sr.consensus_sets(C, seeds, k)
    sets = r["sets"][b, :S].astype(np.int64)
    assert np.array_equal(sets[:, :kk], want_sets) and (sets[:, kk:] == -1).all(), f"{tag}: consensus sets"
    # S5
    Md = r["Mmat"][b, :S].astype(np.float64)
    a = np.stack([sr._lengths(s64[idx]) for idx in want_sets])
    q = np.stack([sr._lengths(t64[idx]) for idx in want_sets])
    d = a - q
    want_M = np.stack([sr.spatial_matrix(src[idx], tgt[idx], sig) for idx in want_sets])
    bound = U24 * (8 + 8 * (a + q) * np.abs(d) / pr.f32(sig) ** 2)
    m_ratio = float((np.abs(Md[:, :kk, :kk] - want_M) / bound).max())
    assert m_ratio <= 1.0, f"{tag}: Mmat {m_ratio:.3f} of its bound"
    outside = Md.copy()
    outside[:, :kk, :kk] = 0
    assert not outside.any()
    # S6 - S8
    close = r["close"][b, :S].astype(bool)                      # [S, nit]
    joint = close.all(0)
    stop = int(np.argmax(joint)) if joint.any() else nit - 1
    tl = sr.tail(want_sets, src, tgt, sig, nit, tau, stop=stop)
    fit = r["fitness"][b, :S].astype(np.float64)
    Td = r["seed_T"][b, :S].astype(np.float64)
    assert np.isfinite(Td).all() and np.isfinite(fit).all()
    own = pr.residuals(Td, s64, t64)
    own_near = (np.abs(own - pr.f32(tau)) < pr.NEAR).sum(1)
    assert (np.abs(fit - (own < pr.f32(tau)).mean(1)) <= (own_near + 1e-3) / n).all(), f"{tag}: fitness under the device's own transforms"
    good = np.array([covariance_ratio(s64[idx], t64[idx], w) > 1e-2 for idx, w in zip(want_sets, tl["weights"])])
    assert good.any()
    t_err = float(np.abs(Td[good] - tl["T"][good]).max())
    assert t_err <= 1e-4, f"{tag}: seed transforms {t_err:.2e}"
    assert (np.abs(fit[good] - tl["fitness"][good]) <= (tl["near"][good] + own_near[good] + 1e-3) / n).all(), f"{tag}: fitness"
    best = int(r["best"][b])
    assert best == int(np.argmax(r["fitness"][b, :S])), f"{tag}: best is not the first maximum"
    assert r["T0"][b].tobytes() == r["seed_T"][b, best].tobytes()
    # S9 and the whole
    T = r["T"][b].astype(np.float64)
    assert np.isfinite(T).all() and T[3].tolist() == [0.0, 0.0, 0.0, 1.0] and int(r["status"][b]) == 0
    line = (f"{tag}: n={n} conf ratio {ratio:.2e} (R = {R:.2e}) seeds {S} seed mismatches {seed_mismatch} (gap {sd['gap']:.1e}) "
            f"tie-decided sets {int(ties.sum())} Mmat {m_ratio:.3f} of its bound stop {stop} well-conditioned seeds {int(good.sum())} "
            f"seed_T err {t_err:.1e}")
    if G is not None:
        rot, trans = sr.pose_error(T, G)
        line += f" pose {rot:.3f} deg {trans * 1e3:.2f} mm"
    print(line)
    assert ratio <= R, f"{tag}: conf ratio {ratio:.3e} > {R:.3e}"
    assert seed_mismatch == 0 or sd["gap"] < pr.NEAR, f"{tag}: {seed_mismatch} seeds differ with every distance clear of the radius"
    if G is not None:
        assert rot < ROT_BAR_DEG and trans < TRANS_BAR_M, f"{tag}: pose"


@pytest.mark.parametrize("name", list(SHAPES))
def test_stages_against_the_restatement(name):
    n_cap, pairs, truth = shape_inputs(name)
    r = shape_run(name)
    for b, ((src, tgt), G) in enumerate(zip(pairs, truth)):
        check_pair(f"{name}[{b}]", src, tgt, n_cap, r, b, G)


def test_register_equals_stages_and_runs_repeat_bit_for_bit():
    from oryon_amd import ops
    n_cap, pairs, _ = shape_inputs("3x128")
    r = shape_run("3x128")
    src, tgt, n = pack(pairs, n_cap)
    out = ops.spectral_register(src, tgt, n, want_labels=True)
    torch.cuda.synchronize()
    assert out["T"].cpu().numpy().tobytes() == r["T"].tobytes() and out["status"].tolist() == [0, 0, 0]
    lab = out["labels"].cpu().numpy()
    for b, (s, t) in enumerate(pairs):                            # labels: the inliers of the best hypothesis; rows >= n are 0
        res = pr.residuals(r["T0"][b][None].astype(np.float64), s.astype(np.float64), t.astype(np.float64))[0]
        clear = np.abs(res - pr.f32(CFG["inlier_threshold"])) > pr.NEAR
        assert np.array_equal(lab[b, :len(s)][clear], (res < pr.f32(CFG["inlier_threshold"]))[clear]) and not lab[b, len(s):].any()
    again = run_stages(pairs, n_cap)
    S = r["n_seeds"]
    for key in ("compat", "conf", "n_seeds", "best", "T0", "T", "status"):
        assert again[key].tobytes() == r[key].tobytes(), key
    for b in range(len(pairs)):
        for key in ("seeds", "sets", "scores", "Mmat", "close", "seed_T", "fitness"):
            assert again[key][b, :S[b]].tobytes() == r[key][b, :S[b]].tobytes(), key


def test_a_pair_alone_at_any_batch_position_and_on_a_side_stream():
    n_cap, pairs, _ = shape_inputs("3x128")
    r = shape_run("3x128")
    keys = ("compat", "conf", "T0", "T", "best")
    for b, pair in enumerate(pairs):
        alone = run_stages([pair], n_cap)
        for key in keys:
            assert alone[key][0].tobytes() == r[key][b].tobytes(), (b, key)
    perm = [2, 0, 1]
    moved = run_stages([pairs[i] for i in perm] + [pairs[0]], n_cap)
    for pos, i in enumerate(perm + [0]):
        S = int(r["n_seeds"][i])
        for key in keys:
            assert moved[key][pos].tobytes() == r[key][i].tobytes(), (pos, key)
        for key in ("seeds", "sets", "seed_T", "fitness"):
            assert moved[key][pos, :S].tobytes() == r[key][i, :S].tobytes(), (pos, key)
    side = run_stages(pairs, n_cap, stream=torch.cuda.Stream())
    for key in keys:
        assert side[key].tobytes() == r[key].tobytes(), key


def test_a_wider_buffer_does_not_change_a_pair():
    """The same pair in a buffer of 128 and of 256 rows (other grid, other S_cap): the same pose, bytes."""
    n_cap, pairs, _ = shape_inputs("3x128")
    r = shape_run("3x128")
    wide = run_stages([pairs[1]], 256)
    assert wide["T"][0].tobytes() == r["T"][1].tobytes() and wide["conf"][0, :128].tobytes() == r["conf"][1].tobytes()


def test_edges_short_pairs_and_small_consensus_sets():
    ns = [0, 1, 2, 9, 10, 11, 41]
    made = [sr.planted(max(n, 1), 0.0, 20 + i) for i, n in enumerate(ns)]
    pairs = [(m[0][:n], m[1][:n]) for m, n in zip(made, ns)]
    r = run_stages(pairs, 128)
    eye = np.eye(4, dtype=np.float32)
    for b, n in enumerate(ns):
        if n < 10:
            assert int(r["n_seeds"][b]) == 0 and int(r["status"][b]) == 2 and np.array_equal(r["T"][b], eye) and int(r["best"][b]) == -1
        else:
            kk = min(40, n - 1)
            assert int(r["n_seeds"][b]) == n // 10 and int(r["status"][b]) == 0
            assert (r["sets"][b, 0, :kk] >= 0).all() and (r["sets"][b, 0, kk:] == -1).all() and kk == {10: 9, 11: 10, 41: 40}[n]
            check_pair(f"edge n={n}", pairs[b][0], pairs[b][1], 128, r, b, made[b][2])


def test_status_in_pure_outliers_and_coincident_points():
    rng = np.random.default_rng(5)
    src, tgt, G, _ = sr.planted(200, 0.7, 3)
    noise_a = rng.uniform(-0.15, 0.15, (200, 3)).astype(np.float32)
    noise_b = rng.uniform(-0.15, 0.15, (200, 3)).astype(np.float32)
    same = np.tile(np.float32([[0.01, 0.02, 0.03]]), (200, 1))
    pairs = [(src, tgt), (src, tgt), (noise_a, noise_b), (same, noise_b)]
    r = run_stages(pairs, 256, status=[0, 1, 0, 0])
    assert r["status"].tolist() == [0, 1, 0, 0]
    assert np.array_equal(r["T"][1], np.eye(4, dtype=np.float32))                      # a failure status: identity, status passed on
    rot, trans = sr.pose_error(r["T"][0].astype(np.float64), G)
    assert rot < ROT_BAR_DEG and trans < TRANS_BAR_M
    for b in (2, 3):
        for key in ("conf", "T0", "T"):
            assert np.isfinite(r[key][b]).all(), (b, key)
        S = int(r["n_seeds"][b])
        assert S == 20 and np.isfinite(r["seed_T"][b, :S]).all() and np.isfinite(r["Mmat"][b, :S]).all() and np.isfinite(r["fitness"][b, :S]).all()
        R3 = r["T"][b, :3, :3].astype(np.float64)
        assert np.abs(R3 @ R3.T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(R3) - 1) < 1e-5


def test_unsupported_shapes_raise():
    from oryon_amd import _lib, ops
    z = torch.zeros((1, 2176, 3), device=DEV)
    n = torch.tensor([100], dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.OryonError):
        ops.spectral_register(z, z, n)
    with pytest.raises(_lib.OryonError):
        ops.spectral_register(z[:, :100].contiguous(), z[:, :100].contiguous(), n)
    with pytest.raises(_lib.OryonError):
        ops.spectral_register(z[:, :128].contiguous(), z[:, :128].contiguous(), n, k=64)


def test_geo6d_facade_equals_the_batched_result():
    from oryon_amd import geo6d
    _, pairs, _ = shape_inputs("2x256")
    r = shape_run("2x256")
    for b, (src, tgt) in enumerate(pairs):
        T = geo6d.spectral_pose(torch.from_numpy(src), torch.from_numpy(tgt), DEV)
        assert T.dtype == torch.float32 and T.shape == (4, 4) and T.device.type == "cpu"
        assert T.numpy().tobytes() == r["T"][b].tobytes()
    assert torch.equal(geo6d.spectral_pose(pairs[0][0][:5], pairs[0][1][:5], DEV), torch.eye(4))          # no seed: identity
    # other thresholds reach the kernels
    loose = geo6d.spectral_pose(pairs[1][0], pairs[1][1], DEV, inlier_threshold=0.10, sigma_d=0.10, nms_radius=0.10)
    assert bool(torch.isfinite(loose).all()) and loose.numpy().tobytes() != r["T"][1].tobytes()


# ------------------------------------------------------------------------------------------------ callers
def _batch(first, B, H=48, C=32, dev=DEV):
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


def _spectral_pipeline(H=48):
    from oryon_amd.pipeline import Pipeline, default_args
    args = default_args(**{"test.mask": "oracle", "test.solver": "spectral", "model.image_encoder.img_size": [H, H], "dataset.img_size": [H, H]})
    return Pipeline(args, pointdsc_solver=None)


def test_pipeline_per_sample_route_runs_the_spectral_solver():
    pl = _spectral_pipeline()
    batch, _ = _batch(3, 2)
    torch.manual_seed(1)
    recs = pl.test_step(batch, 0)
    assert [r["status"] for r in recs] == [0, 0]
    for r in recs:
        T = r["pred_pose_rel"]
        assert T.dtype == torch.float32 and T.shape == (4, 4) and T[3].tolist() == [0.0, 0.0, 0.0, 1.0] and bool(torch.isfinite(T).all())
    assert len(pl.pred_lines) == 2
    pl.args.test.solver = "ransac"                                      # the solver is fixed at construction
    with pytest.raises(RuntimeError, match="fixed at construction"):
        pl.test_step(batch, 0)


def test_engine_and_pipeline_batched_route_equal_the_entry_point_bit_for_bit():
    from oryon_amd import geo6d, ops
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    pl = _spectral_pipeline()
    first, B = 20, 3
    batch, _ = _batch(first, B)
    batch["anchor"]["mask"][2] = 0                                       # pair 2: NO_MASK -> identity, status 1
    out = pl.test_step_batched(batch, first_pair_index=first)
    torch.cuda.synchronize()
    assert pl._engine._native is None and pl._engine.cfg.solver == "spectral"          # the per-call schedule
    assert out["status"].tolist() == [0, 0, 1] and torch.equal(out["pose"][2].cpu(), torch.eye(4))
    key = torch.arange(first, first + B, dtype=torch.int64, device=DEV)
    eng = MatchPoseEngine(None, MatchPoseConfig(solver="spectral", seed=pl.args.seed))
    stack = lambda x: torch.stack([d.squeeze() for d in x]).to(DEV).float().contiguous()
    mask = lambda m: ops.mask_resize_nearest(m.to(DEV), (48, 48))
    o2 = eng.run(batch["featmap_a"], batch["featmap_q"], mask(batch["anchor"]["mask"]), mask(batch["query"]["mask"]),
                 stack(batch["anchor"]["orig_depth"]), stack(batch["query"]["orig_depth"]), batch["anchor"]["camera"].to(DEV),
                 batch["query"]["camera"].to(DEV), key, keep=True)
    torch.cuda.synchronize()
    assert torch.equal(o2["pose"], out["pose"]) and torch.equal(o2["status"], out["status"])
    want = ops.spectral_register(o2["pcd_a"], o2["pcd_q"], o2["n_lifted"], o2["status"])
    assert torch.equal(want["T"], out["pose"]) and torch.equal(want["status"], out["status"])
    assert not torch.equal(out["pose"][0].cpu(), torch.eye(4))
    # the per-sample facade on the same points is the same computation
    for b in (0, 1):
        m = int(o2["n_lifted"][b])
        T = geo6d.spectral_pose(o2["pcd_a"][b, :m], o2["pcd_q"][b, :m], DEV)
        assert torch.equal(T, out["pose"][b].cpu())
