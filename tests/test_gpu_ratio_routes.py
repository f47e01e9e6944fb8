"""test.ratio through the façade, on synthetic 48 x 48 pairs (C = 32): pcd.match_presample / nn_correspondences_filtered,
MatchPoseEngine (solver = ransac: no weights), Pipeline and run_pose.py.  The kernel itself is tests/test_gpu_match_second.py; here
every route is checked against ops.match_second called by hand on the route's own inputs, the switched-off routes against a call
without the keyword, and the case the filter exists for - a block of descriptors that occurs twice in the query map - against a
float64 all-pairs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ratio_restatement as rr  # noqa: E402
from test_gpu_ransac import _batch  # noqa: E402  (the two-sided batch dict of Pipeline.test_step on the same synthetic pairs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, C, B = 48, 32, 4
THR = 0.6                                    # every anchor is valid: the ratio test does the cutting
RATIO, R = 0.8, 5


@pytest.fixture(scope="module")
def mb():
    from oryon_amd.synth import make_batch
    return make_batch(40, B, H, H, C, device=DEV)


def _presample(mb, p, **kw):
    from oryon_amd import pcd
    return pcd.match_presample(mb["feat_a"][p], mb["feat_q"][p], mb["mask_a"][p], mb["mask_q"][p], THR, **kw)


def _by_hand(mb, p, pre, mutual, ratio, radius):
    """ops on the rows match_presample reports: -> (gate u8, second_dist, second_argmin, keep) of pair p."""
    from oryon_amd import ops
    n1, n2 = pre["roi1"].shape[0], pre["roi2"].shape[0]
    roi1 = (pre["roi1"][:, 0] * H + pre["roi1"][:, 1]).to(torch.int32)[None].contiguous()
    roi2 = (pre["roi2"][:, 0] * H + pre["roi2"][:, 1]).to(torch.int32)[None].contiguous()
    c1, c2 = torch.tensor([n1], dtype=torch.int32, device=DEV), torch.tensor([n2], dtype=torch.int32, device=DEV)
    a_hat = ops.gather_normalise(mb["feat_a"][p:p + 1].contiguous(), roi1, c1, ops.round_up(n1, ops.ROW_PAD))
    q_hat = ops.gather_normalise(mb["feat_q"][p:p + 1].contiguous(), roi2, c2, ops.round_up(n2, ops.ROW_PAD))
    if mutual:
        md, am, va, _, _, gate = ops.match_mutual(a_hat, q_hat, c1, c2, THR)
    else:
        md, am, gate = ops.match(a_hat, q_hat, c1, c2, THR)
    sd, sa, kp = ops.match_second(a_hat, q_hat, c1, c2, roi2, H, radius, md, am, gate, ratio)
    return md[0, :n1], am[0, :n1], gate[0, :n1], sd[0, :n1], sa[0, :n1], kp[0, :n1]


def test_match_presample_ratio_keys_agree_with_the_entry_point(mb):
    base = {"roi1", "roi2", "min_dist", "argmin", "valid"}
    seconds = {}
    for mutual in (False, True):
        for mode in ("exact", "screened8"):                              # ratio takes the exact scan whatever the mode says
            pre = _presample(mb, 0, ratio=RATIO, ratio_radius=R, mutual=mutual, mode=mode)
            assert set(pre) == base | {"second_dist", "second_argmin", "keep"} | ({"mutual", "rev_argmin", "rev_min_dist"} if mutual else set())
            n1 = pre["roi1"].shape[0]
            assert pre["keep"].dtype == torch.bool and pre["keep"].shape == (n1,)
            assert pre["second_argmin"].dtype == torch.int64 and pre["second_dist"].dtype == torch.float32
            md, am, gate, sd, sa, kp = _by_hand(mb, 0, pre, mutual, RATIO, R)
            assert torch.equal(pre["min_dist"], md) and torch.equal(pre["argmin"], am.long())
            assert torch.equal(pre["second_dist"], sd) and torch.equal(pre["second_argmin"], sa.long()) and torch.equal(pre["keep"], kp.bool())
            assert torch.equal(pre["mutual" if mutual else "valid"], gate.bool())
            # mutual + ratio: the conjunction, by the numpy statement
            want = rr.keep_flags(md.cpu().numpy(), sd.cpu().numpy(), gate.cpu().numpy(), RATIO)
            assert np.array_equal(pre["keep"].cpu().numpy(), want) and 1 < want.sum() < gate.sum().item()
            seconds[mutual] = pre
    # the second minimum does not depend on the gate; with both filters on keep = mutual & (the ratio test on valid rows)
    for k in ("second_dist", "second_argmin"):
        assert torch.equal(seconds[False][k], seconds[True][k])
    assert bool(seconds[False]["valid"].all())                           # THR passes every row, so keep[False] is the bare ratio test
    assert torch.equal(seconds[True]["keep"], seconds[True]["mutual"] & seconds[False]["keep"])


def test_match_presample_without_ratio_is_what_it_was(mb):
    for kw in (dict(), dict(subsample_source=500), dict(mode="screened8"), dict(mutual=True)):
        torch.manual_seed(3)
        a = _presample(mb, 1, **kw)
        s_a = torch.get_rng_state()
        torch.manual_seed(3)
        b = _presample(mb, 1, ratio=0.0, ratio_radius=3, **kw)
        assert torch.equal(s_a, torch.get_rng_state())
        assert set(a) == set(b) and "keep" not in a and "second_dist" not in a
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    from oryon_amd import pcd
    empty = torch.zeros_like(mb["mask_a"][1])
    pre = pcd.match_presample(mb["feat_a"][1], mb["feat_q"][1], empty, mb["mask_q"][1], THR, ratio=RATIO)
    assert pre["keep"].shape == (0,) and pre["second_dist"].shape == (0,) and pre["second_argmin"].dtype == torch.int64
    pre = pcd.match_presample(mb["feat_a"][1], mb["feat_q"][1], mb["mask_a"][1], empty, THR, ratio=RATIO)
    assert not pre["keep"].any() and bool(torch.isinf(pre["second_dist"]).all()) and pre["keep"].shape == pre["valid"].shape


def _two_equal_pixels(mb, p):
    """-> (feat_q, mask_q) of pair p with ONE descriptor at two pixels 20 apart and nothing else in the mask: every anchor's nearest
    row has an exact copy outside any disc of radius <= 20, so no row passes a ratio < 1 (distances are not zero)."""
    fq = mb["feat_q"][p].clone()
    fq[:, 30, 34] = fq[:, 10, 34]
    mq = torch.zeros_like(mb["mask_q"][p])
    mq[10, 34] = mq[30, 34] = 1
    return fq, mq


def test_nn_correspondences_filtered_rows_and_generator_state(mb):
    from oryon_amd import pcd
    # both draws are made, the second WITH replacement in every call (more rows asked for than any call keeps): see the mutual test
    args = (mb["feat_a"][2], mb["feat_q"][2], mb["mask_a"][2], mb["mask_q"][2], THR, 1000, 400, "cpu")
    assert int(mb["mask_a"][2].sum()) > 400
    torch.manual_seed(9)
    one = pcd.nn_correspondences(*args)
    s_one = torch.get_rng_state()
    torch.manual_seed(9)
    same = pcd.nn_correspondences_filtered(*args, ratio=0.0)
    assert torch.equal(s_one, torch.get_rng_state()) and torch.equal(one, same)
    torch.manual_seed(9)
    same_m = pcd.nn_correspondences_filtered(*args, mutual=True)
    s_m = torch.get_rng_state()
    torch.manual_seed(9)
    assert torch.equal(pcd.nn_correspondences(*args, mutual=True), same_m) and torch.equal(s_m, torch.get_rng_state())
    torch.manual_seed(9)
    flt = pcd.nn_correspondences_filtered(*args, ratio=RATIO, ratio_radius=R)
    assert torch.equal(s_one, torch.get_rng_state())                    # the same two host draws, in the same order
    assert flt is not None and flt.shape == (1000, 4) and flt.dtype == torch.int64 and not torch.equal(flt, one)
    torch.manual_seed(9)
    pre = pcd.match_presample(*args[:5], subsample_source=400, ratio=RATIO, ratio_radius=R)
    rows = torch.cat((pre["roi1"], pre["roi2"][pre["argmin"]]), dim=1)
    kept = {tuple(r) for r in rows[pre["keep"]].cpu().tolist()}
    dropped = {tuple(r) for r in rows[pre["valid"] & ~pre["keep"]].cpu().tolist()}
    assert len(kept) > 1 and len(dropped) > 1 and all(tuple(r) in kept for r in flt.cpu().tolist())
    assert any(tuple(r) in dropped for r in one.cpu().tolist())         # the unfiltered call does return such rows
    # at most one kept row -> None
    fq, mq = _two_equal_pixels(mb, 2)
    assert pcd.nn_correspondences_filtered(args[0], fq, args[2], mq, 1.5, 100, None, "cpu", ratio=0.99, ratio_radius=R) is None
    assert pcd.nn_correspondences_filtered(args[0], fq, args[2], mq, 1.5, 100, None, "cpu", ratio=1.0, ratio_radius=R) is not None
    assert pcd.nn_correspondences(args[0], fq, args[2], mq, 1.5, 100, None, "cpu") is not None


def _engine_run(mb, keep=True, feat_q=None, mask_q=None, **cfg):
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    eng = MatchPoseEngine(None, MatchPoseConfig(solver="ransac", dist_th=THR, **cfg))
    cam = mb["camera"].to(DEV)
    key = torch.arange(40, 40 + B, dtype=torch.int64, device=DEV)
    out = eng.run(mb["feat_a"], mb["feat_q"] if feat_q is None else feat_q, mb["mask_a"], mb["mask_q"] if mask_q is None else mask_q,
                  mb["depth_a"], mb["depth_q"], cam, cam, key, keep=keep)
    torch.cuda.synchronize()
    return eng, out, key


@pytest.mark.parametrize("mutual", [False, True])
def test_engine_ratio_equals_the_facade_and_the_staged_recomputation(mb, mutual):
    from oryon_amd import ops, pcd
    from oryon_amd.engine import PAIR_NO_CORR
    feat_q, mask_q = mb["feat_q"].clone(), mb["mask_q"].clone()
    feat_q[0], mask_q[0] = _two_equal_pixels(mb, 0)                      # pair 0: the filter leaves no row
    eng, out, key = _engine_run(mb, feat_q=feat_q, mask_q=mask_q, ratio=RATIO, ratio_radius=R, mutual=mutual, src_sampling=None)
    assert eng._native is None                                           # the per-call schedule: the C step engine is kept away
    for k in ("second_dist", "second_argmin", "keep", "roi_a", "roi_q", "n_a", "n_q", "argmin", "valid", "corrs"):
        assert k in out, k
    na = out["n_a"].tolist()
    for p in range(B):                                                   # the façade on the same pair (no subsampling on either side)
        pre = pcd.match_presample(mb["feat_a"][p], feat_q[p], mb["mask_a"][p], mask_q[p], THR, ratio=RATIO, ratio_radius=R, mutual=mutual)
        n = na[p]
        assert n == pre["keep"].shape[0]
        assert torch.equal(out["keep"][p, :n].bool(), pre["keep"]) and torch.equal(out["second_dist"][p, :n], pre["second_dist"])
        assert torch.equal(out["second_argmin"][p, :n].long(), pre["second_argmin"]) and torch.equal(out["argmin"][p, :n].long(), pre["argmin"])
        assert int(out["n_valid"][p]) == int(pre["keep"].sum())          # n_valid counts the kept rows
    gate = out["mutual"] if mutual else out["valid"]
    cap_a, cap_q = out["argmin"].shape[1], out["roi_q"].shape[1]
    a_hat = ops.gather_normalise(mb["feat_a"].contiguous(), out["roi_a"], out["n_a"], cap_a)
    q_hat = ops.gather_normalise(feat_q.contiguous(), out["roi_q"], out["n_q"], ops.round_up(H * H, ops.ROW_PAD))
    sd, sa, kp = ops.match_second(a_hat, q_hat, out["n_a"], out["n_q"], out["roi_q"], H, R, out["min_dist"], out["argmin"], gate, RATIO)
    for p in range(B):
        assert torch.equal(out["keep"][p, :na[p]], kp[p, :na[p]]) and torch.equal(out["second_dist"][p, :na[p]], sd[p, :na[p]])
    sel = ops.select_corrs(out["roi_a"], out["roi_q"], out["n_a"], out["n_q"], out["argmin"], out["keep"], H, eng.cfg.n_corrs,
                           eng.cfg.seed, key, corr_rows=eng.n_cap)
    assert torch.equal(out["corrs"], sel[0]) and torch.equal(out["n_valid"], sel[1])
    assert int(out["n_valid"][0]) <= 1 and int(out["status"][0]) == PAIR_NO_CORR and torch.equal(out["pose"][0].cpu(), torch.eye(4))
    assert out["status"][1:].tolist() == [0] * (B - 1) and (out["n_valid"][1:] > 1).all()
    for p in range(1, B):                                                # every correspondence is a kept row
        m = out["keep"][p, :na[p]].bool()
        pix_a = out["roi_a"][p, :na[p]][m].cpu().tolist()
        pix_q = out["roi_q"][p][out["argmin"][p, :na[p]][m].long()].cpu().tolist()
        pairs = {(a // H, a % H, q // H, q % H) for a, q in zip(pix_a, pix_q)}
        rows = out["corrs"][p, : int(sel[2][p])].cpu().tolist()
        assert len(rows) > 1 and all(tuple(r) in pairs for r in rows)
    one_way = _engine_run(mb, keep=False, mutual=mutual, src_sampling=None)[1]
    # the filter only removes rows, and on these pairs it does remove some (not on every pair: one has a true match for every anchor)
    assert (out["n_valid"][1:] <= one_way["n_valid"][1:]).all() and (out["n_valid"][1:] < one_way["n_valid"][1:]).any()


def test_engine_without_ratio_is_todays_run_and_sample_first_is_refused(mb):
    _, a, _ = _engine_run(mb)
    eng, b, _ = _engine_run(mb, ratio=0.0, ratio_radius=7)
    assert set(a) == set(b) and "keep" not in a and "second_dist" not in a
    for k in ("pose", "status", "n_valid", "n_lifted", "corrs", "n_a"):
        assert torch.equal(a[k], b[k]), k
    for p, n in enumerate(a["n_a"].tolist()):                            # rows >= n_a of the per-row outputs are never written
        for k in ("argmin", "valid", "min_dist"):
            assert torch.equal(a[k][p, :n], b[k][p, :n]), k
    cam = mb["camera"].to(DEV)
    with pytest.raises(ValueError, match="sample_first"):
        eng.cfg.ratio, eng.cfg.sample_first = 0.8, 100
        eng.run(mb["feat_a"], mb["feat_q"], mb["mask_a"], mb["mask_q"], mb["depth_a"], mb["depth_q"], cam, cam)


# ------------------------------------------------------------------------------------------------ the case the filter exists for
def test_a_repeated_block_is_rejected_and_unique_pixels_are_kept():
    """A 6 x 6 block of the query map is copied r + 7 pixels away; the anchor map is the query map + noise, pixel for pixel.  An anchor
    on either copy finds its own pixel and, outside the disc, an exact copy of it: min_dist / second = 1.  An anchor on a unique pixel
    finds second ~ 0.1 against min_dist ~ 1e-3.  In float64 both groups are at least a factor 2 away from the cut."""
    from oryon_amd import pcd
    ratio, r, noise = 0.25, 5, 0.05
    g = torch.Generator().manual_seed(123)
    fq = torch.randn(C, H, H, generator=g)
    fq[:, 26:32, 26:32] = fq[:, 14:20, 14:20]                            # the copy: 12 pixels down and right (>= r + 2)
    fa = fq + noise * torch.randn(C, H, H, generator=g)
    mask = torch.zeros(H, H, dtype=torch.int32)
    mask[8:40, 8:40] = 1
    # float64 all-pairs on the CPU: the two groups against the cut
    pix = torch.nonzero(mask.reshape(-1)).squeeze(1).numpy()
    y, x = pix // H, pix % H
    a64, q64 = fa.reshape(C, -1)[:, pix].T.double().numpy(), fq.reshape(C, -1)[:, pix].T.double().numpy()
    d = 0.5 * (1.0 - (a64 / np.linalg.norm(a64, axis=1, keepdims=True)) @ (q64 / np.linalg.norm(q64, axis=1, keepdims=True)).T)
    am = d.argmin(axis=1)
    outside = (y[None, :] - y[am][:, None]) ** 2 + (x[None, :] - x[am][:, None]) ** 2 >= r * r
    second = np.where(outside, d, np.inf).min(axis=1)
    quot = d.min(axis=1) / second
    block = ((y >= 14) & (y < 20) & (x >= 14) & (x < 20)) | ((y >= 26) & (y < 32) & (x >= 26) & (x < 32))
    assert block.sum() == 72 and (quot[block] >= 2 * ratio).all() and (quot[~block] <= ratio / 2).all(), (quot[block].min(), quot[~block].max())
    assert (np.sort(d, axis=1)[~block][:, 1] - np.sort(d, axis=1)[~block][:, 0] > 1e-3).all()      # unique pixels: argmin is float-proof
    sub = np.r_[np.nonzero(block)[0][:3], np.nonzero(~block)[0][:3]]    # ... and the loop-by-loop statement agrees with the vectorised one
    bf = rr.brute_force(a64[sub], q64, pix, H, r, ratio, THR)
    assert np.allclose(bf["second_dist"], second[sub], rtol=0, atol=1e-12) and np.array_equal(bf["keep"], ~block[sub])
    # the device
    pre = pcd.match_presample(fa.to(DEV), fq.to(DEV), mask.to(DEV), mask.to(DEV), THR, ratio=ratio, ratio_radius=r)
    assert bool(pre["valid"].all())                                      # the distance threshold passes all of them
    keep = pre["keep"].cpu().numpy()
    assert np.array_equal(keep, ~block)
    assert np.array_equal(pre["argmin"].cpu().numpy()[~block], np.arange(len(pix))[~block])
    mut = pcd.match_presample(fa.to(DEV), fq.to(DEV), mask.to(DEV), mask.to(DEV), THR, mutual=True)["mutual"].cpu().numpy()
    assert mut[block].sum() >= 36                                        # the cross-check passes at least one anchor per repeated pixel
    both = pcd.match_presample(fa.to(DEV), fq.to(DEV), mask.to(DEV), mask.to(DEV), THR, mutual=True, ratio=ratio, ratio_radius=r)
    assert np.array_equal(both["keep"].cpu().numpy(), mut & keep) and not both["keep"].cpu().numpy()[block].any()
    # radius 1 (Lowe's test on a dense map) asks less: the block is still rejected (an exact copy), unique pixels are still kept
    lowe = pcd.match_presample(fa.to(DEV), fq.to(DEV), mask.to(DEV), mask.to(DEV), THR, ratio=ratio, ratio_radius=1)
    assert np.array_equal(lowe["keep"].cpu().numpy(), ~block)


# ------------------------------------------------------------------------------------------------ pipeline and driver
def test_pipeline_ratio_runs_and_counts_no_more_rows():
    from oryon_amd.pipeline import Pipeline, default_args
    base = {"test.mask": "oracle", "test.solver": "ransac", "model.image_encoder.img_size": [H, H], "dataset.img_size": [H, H],
            "test.dist_th": THR}
    assert default_args(**base).test.ratio == 0.0
    pl_r = Pipeline(default_args(**{**base, "test.ratio": RATIO, "test.ratio_radius": 3}), pointdsc_solver=None)
    pl_0 = Pipeline(default_args(**base), pointdsc_solver=None)
    batch, _ = _batch(3, 2)
    out_r = pl_r.test_step_batched(batch, first_pair_index=3)
    out_0 = pl_0.test_step_batched(batch, first_pair_index=3)
    torch.cuda.synchronize()
    assert (pl_r._engine.cfg.ratio, pl_r._engine.cfg.ratio_radius) == (RATIO, 3) and pl_0._engine.cfg.ratio == 0.0
    assert out_r["status"].tolist() == [0, 0] and (out_r["n_valid"] < out_0["n_valid"]).all() and (out_r["n_valid"] > 1).all()
    torch.manual_seed(1)
    saved = np.random.get_state()
    try:
        np.random.seed(1)
        recs = pl_r.test_step(batch, 0)                                  # the per-sample loop hands the flags to nn_correspondences_filtered
    finally:
        np.random.set_state(saved)
    assert [r["status"] for r in recs] == [0, 0]
    old = default_args(**{k: v for k, v in base.items() if k != "test.dist_th"})      # an args object from before the flags existed keeps working
    del old.test.ratio, old.test.ratio_radius
    assert Pipeline(old, pointdsc_solver=None).test_step_batched(batch, first_pair_index=3)["status"].tolist() == [0, 0]


def test_run_pose_ratio_sets_the_default_and_records_the_flags(tmp_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_pose
    from oryon_amd import engine
    out = str(tmp_path / "pred.csv")
    common = ["--solver", "ransac", "--pairs", "4", "--batch", "2", "--size", "64", "--channels", "32", "--out", out]
    try:
        s = run_pose.main(common + ["--ratio", "0.8", "--ratio-radius", "3"])
        assert engine.default_ratio() == (0.8, 3) and s["ratio"] == 0.8 and s["ratio_radius"] == 3 and s["pairs"] == 4 and s["failures"] == 0
        assert "mutual" not in s
        s0 = run_pose.main(common)
        assert engine.default_ratio() == (0.0, 5) and "ratio" not in s0 and "ratio_radius" not in s0 and s0["pairs"] == 4
    finally:
        engine.set_default_ratio(0.0, 5)
        engine.set_default_solver("pointdsc")
