"""test.mutual through the façade, on synth.make_batch at a small map (48 x 48, C = 32): pcd.match_presample / nn_correspondences,
MatchPoseEngine (solver = ransac: no weights) and Pipeline.  The kernel itself is tests/test_gpu_match_mutual.py; here every route is
checked against ops.match_mutual on the route's own inputs, and the switched-off routes against a call without the keyword."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutual_restatement as mr  # noqa: E402
from test_gpu_ransac import _batch  # noqa: E402  (the two-sided batch dict of Pipeline.test_step on the same synthetic pairs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, C, B = 48, 32, 4


@pytest.fixture(scope="module")
def mb():
    from oryon_amd.synth import make_batch
    return make_batch(40, B, H, H, C, device=DEV)


def _presample(mb, p, **kw):
    from oryon_amd import pcd
    return pcd.match_presample(mb["feat_a"][p], mb["feat_q"][p], mb["mask_a"][p], mb["mask_q"][p], 0.25, **kw)


def test_match_presample_mutual_keys_agree_with_the_entry_point(mb):
    from oryon_amd import ops
    for mode in ("exact", "screened8"):                                  # mutual takes the exact scan whatever the mode says
        pre = _presample(mb, 0, mutual=True, mode=mode)
        assert set(pre) == {"roi1", "roi2", "min_dist", "argmin", "valid", "mutual", "rev_argmin", "rev_min_dist"}
        n1, n2 = pre["roi1"].shape[0], pre["roi2"].shape[0]
        assert pre["mutual"].dtype == torch.bool and pre["mutual"].shape == (n1,)
        assert pre["rev_argmin"].dtype == torch.int64 and pre["rev_argmin"].shape == (n2,) and pre["rev_min_dist"].shape == (n2,)
        roi1 = (pre["roi1"][:, 0] * H + pre["roi1"][:, 1]).to(torch.int32)[None].contiguous()
        roi2 = (pre["roi2"][:, 0] * H + pre["roi2"][:, 1]).to(torch.int32)[None].contiguous()
        c1, c2 = torch.tensor([n1], dtype=torch.int32, device=DEV), torch.tensor([n2], dtype=torch.int32, device=DEV)
        a_hat = ops.gather_normalise(mb["feat_a"][0:1].contiguous(), roi1, c1, ops.round_up(n1, ops.ROW_PAD))
        q_hat = ops.gather_normalise(mb["feat_q"][0:1].contiguous(), roi2, c2, ops.round_up(n2, ops.ROW_PAD))
        md, am, va, rmd, ram, mu = ops.match_mutual(a_hat, q_hat, c1, c2, 0.25)
        assert torch.equal(pre["min_dist"], md[0, :n1]) and torch.equal(pre["argmin"], am[0, :n1].long()) and torch.equal(pre["valid"], va[0, :n1].bool())
        assert torch.equal(pre["rev_min_dist"], rmd[0, :n2]) and torch.equal(pre["rev_argmin"], ram[0, :n2].long())
        assert torch.equal(pre["mutual"], mu[0, :n1].bool())
        want = mr.mutual_flags(pre["argmin"].cpu().numpy(), pre["valid"].cpu().numpy(), pre["rev_argmin"].cpu().numpy())
        assert np.array_equal(pre["mutual"].cpu().numpy(), want) and 1 < want.sum() <= pre["valid"].sum().item()


def test_match_presample_without_mutual_is_what_it_was(mb):
    for kw in (dict(), dict(subsample_source=500), dict(mode="screened8")):
        torch.manual_seed(3)
        a = _presample(mb, 1, **kw)
        s_a = torch.get_rng_state()
        torch.manual_seed(3)
        b = _presample(mb, 1, mutual=False, **kw)
        assert torch.equal(s_a, torch.get_rng_state())
        assert set(a) == set(b) == {"roi1", "roi2", "min_dist", "argmin", "valid"}
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    empty = torch.zeros_like(mb["mask_a"][1])
    from oryon_amd import pcd
    pre = pcd.match_presample(mb["feat_a"][1], mb["feat_q"][1], empty, mb["mask_q"][1], 0.25, mutual=True)
    assert pre["mutual"].shape == (0,) and not pre["rev_argmin"].any() and bool(torch.isinf(pre["rev_min_dist"]).all())
    assert set(pcd.match_presample(mb["feat_a"][1], mb["feat_q"][1], empty, mb["mask_q"][1], 0.25)) == {"roi1", "roi2", "min_dist", "argmin", "valid"}


def test_nn_correspondences_mutual_rows_and_generator_state(mb):
    from oryon_amd import pcd
    # both calls make both draws: more anchors than subsample_source, and more rows asked for (1000) than either call keeps, so the
    # second draw is with replacement in both - a draw WITHOUT replacement consumes the generator by the number of rows kept, which
    # is what mutual changes, and the two states could not be compared
    args = (mb["feat_a"][2], mb["feat_q"][2], mb["mask_a"][2], mb["mask_q"][2], 0.25, 1000, 400, "cpu")
    assert int(mb["mask_a"][2].sum()) > 400
    torch.manual_seed(9)
    one = pcd.nn_correspondences(*args)
    s_one = torch.get_rng_state()
    torch.manual_seed(9)
    same = pcd.nn_correspondences(*args, mutual=False)
    assert torch.equal(s_one, torch.get_rng_state()) and torch.equal(one, same)
    torch.manual_seed(9)
    mut = pcd.nn_correspondences(*args, mutual=True)
    assert torch.equal(s_one, torch.get_rng_state())                    # the same two host draws, in the same order
    assert mut is not None and mut.shape == (1000, 4) and mut.dtype == torch.int64 and not torch.equal(mut, one)
    torch.manual_seed(9)
    pre = pcd.match_presample(*args[:5], subsample_source=400, mutual=True)
    rows = torch.cat((pre["roi1"], pre["roi2"][pre["argmin"]]), dim=1)[pre["mutual"]]
    keep = {tuple(r) for r in rows.cpu().tolist()}
    assert all(tuple(r) in keep for r in mut.cpu().tolist())            # every returned row is a mutual row
    assert len({tuple(r[2:]) for r in mut.cpu().tolist()}) == len({tuple(r) for r in mut.cpu().tolist()})   # one anchor per query pixel
    # at most one mutual row -> None: one query pixel can be the mutual partner of one anchor only
    one_q = torch.zeros_like(mb["mask_q"][2])
    one_q[H // 2, H // 2] = 1
    assert pcd.nn_correspondences(args[0], args[1], args[2], one_q, 1.5, 100, None, "cpu", mutual=True) is None
    assert pcd.nn_correspondences(args[0], args[1], args[2], one_q, 1.5, 100, None, "cpu") is not None


def _engine_run(mb, keep=True, **cfg):
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    eng = MatchPoseEngine(None, MatchPoseConfig(solver="ransac", **cfg))
    cam = mb["camera"].to(DEV)
    key = torch.arange(40, 40 + B, dtype=torch.int64, device=DEV)
    out = eng.run(mb["feat_a"], mb["feat_q"], mb["mask_a"], mb["mask_q"], mb["depth_a"], mb["depth_q"], cam, cam, key, keep=keep)
    torch.cuda.synchronize()
    return eng, out, key


def test_engine_mutual_equals_the_staged_recomputation(mb):
    from oryon_amd import ops
    eng, out, key = _engine_run(mb, mutual=True)
    assert eng._native is None                                           # the per-call schedule: the C step engine is kept away
    for k in ("mutual", "rev_argmin", "rev_min_dist", "roi_a", "roi_q", "n_a", "n_q", "argmin", "valid", "corrs"):
        assert k in out, k
    cap_a, cap_q = out["argmin"].shape[1], out["rev_argmin"].shape[1]
    a_hat = ops.gather_normalise(mb["feat_a"].contiguous(), out["roi_a"], out["n_a"], cap_a)
    q_hat = ops.gather_normalise(mb["feat_q"].contiguous(), out["roi_q"], out["n_q"], cap_q)
    md, am, va, rmd, ram, mu = ops.match_mutual(a_hat, q_hat, out["n_a"], out["n_q"], eng.cfg.dist_th)
    na, nq = out["n_a"].tolist(), out["n_q"].tolist()
    for p in range(B):
        for got, want, n in ((out["min_dist"], md, na[p]), (out["argmin"], am, na[p]), (out["valid"], va, na[p]), (out["mutual"], mu, na[p]),
                             (out["rev_min_dist"], rmd, nq[p]), (out["rev_argmin"], ram, nq[p])):
            assert torch.equal(got[p, :n], want[p, :n])
    corrs, n_valid, n_sel, status = ops.select_corrs(out["roi_a"], out["roi_q"], out["n_a"], out["n_q"], am, mu, H, eng.cfg.n_corrs,
                                                     eng.cfg.seed, key, corr_rows=eng.n_cap)
    sel = ops.select_corrs(out["roi_a"], out["roi_q"], out["n_a"], out["n_q"], out["argmin"], out["mutual"], H, eng.cfg.n_corrs,
                           eng.cfg.seed, key, corr_rows=eng.n_cap)
    assert torch.equal(out["corrs"], corrs) and torch.equal(out["n_valid"], n_valid) and torch.equal(sel[2], n_sel)
    assert torch.equal(out["corrs"], sel[0]) and torch.equal(out["n_valid"], sel[1])
    # n_valid counts the mutual rows; every correspondence maps back to an anchor row with mutual == 1
    for p in range(B):
        m = out["mutual"][p, :na[p]].bool()
        assert int(out["n_valid"][p]) == int(m.sum()) > 1
        pix_a = out["roi_a"][p, :na[p]][m].cpu().tolist()
        pix_q = out["roi_q"][p][out["argmin"][p, :na[p]][m].long()].cpu().tolist()
        pairs = {(a // H, a % H, q // H, q % H) for a, q in zip(pix_a, pix_q)}
        rows = corrs[p, : int(n_sel[p])].cpu().tolist()
        assert len(rows) > 1 and all(tuple(r) in pairs for r in rows)
    # the planted poses: what tests/test_gpu_ransac.py asks of the one-directional route on these pairs (a status of 0, a finite
    # rigid pose), plus the recorded status being the sampler's
    assert out["status"].tolist() == [0] * B and status.tolist() == [0] * B
    T = out["pose"].cpu()
    assert T.dtype == torch.float32 and bool(torch.isfinite(T).all()) and all(T[p, 3].tolist() == [0.0, 0.0, 0.0, 1.0] for p in range(B))
    one_way = _engine_run(mb, keep=False)[1]
    err = lambda P: (P.cpu().double()[:, :3, 3] - mb["pose"].cpu().double()[:, :3, 3]).norm(dim=1)
    print("translation error (m): mutual", err(out["pose"]).tolist(), "one-directional", err(one_way["pose"]).tolist())
    assert (out["n_valid"] <= one_way["n_valid"]).all()


def test_engine_without_mutual_is_todays_run(mb):
    from oryon_amd.engine import MatchPoseConfig
    assert MatchPoseConfig().mutual is False
    _, a, _ = _engine_run(mb)
    _, b, _ = _engine_run(mb, mutual=False)
    assert set(a) == set(b) and "mutual" not in a and "rev_argmin" not in a
    for k in ("pose", "status", "n_valid", "n_lifted", "corrs", "argmin", "valid", "min_dist"):
        assert torch.equal(a[k], b[k]), k


def test_engine_mutual_few_rows_is_no_corr_and_half_descriptors_compose(mb):
    from oryon_amd.engine import PAIR_NO_CORR
    one_q = mb["mask_q"].clone()
    one_q[0] = 0
    one_q[0, H // 2, H // 2] = 1                                         # pair 0: one query pixel -> at most one mutual row
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    eng = MatchPoseEngine(None, MatchPoseConfig(solver="ransac", mutual=True, half_descriptors=True, dist_th=0.6))
    cam = mb["camera"].to(DEV)
    out = eng.run(mb["feat_a"], mb["feat_q"], mb["mask_a"], one_q, mb["depth_a"], mb["depth_q"], cam, cam, keep=True)
    torch.cuda.synchronize()
    assert int(out["n_valid"][0]) <= 1 and int(out["status"][0]) == PAIR_NO_CORR and torch.equal(out["pose"][0].cpu(), torch.eye(4))
    assert out["status"][1:].tolist() == [0] * (B - 1)
    with pytest.raises(ValueError, match="sample_first"):
        eng.cfg.sample_first = 100
        eng.run(mb["feat_a"], mb["feat_q"], mb["mask_a"], one_q, mb["depth_a"], mb["depth_q"], cam, cam)


def test_pipeline_mutual_runs_and_counts_no_more_rows():
    from oryon_amd.pipeline import Pipeline, default_args
    base = {"test.mask": "oracle", "test.solver": "ransac", "model.image_encoder.img_size": [H, H], "dataset.img_size": [H, H]}
    assert default_args(**base).test.mutual is False
    pl_m = Pipeline(default_args(**{**base, "test.mutual": True}), pointdsc_solver=None)
    pl_0 = Pipeline(default_args(**base), pointdsc_solver=None)
    batch, _ = _batch(3, 2)
    out_m = pl_m.test_step_batched(batch, first_pair_index=3)
    out_0 = pl_0.test_step_batched(batch, first_pair_index=3)
    torch.cuda.synchronize()
    assert pl_m._engine.cfg.mutual is True and pl_0._engine.cfg.mutual is False
    assert out_m["status"].tolist() == [0, 0] and (out_m["n_valid"] <= out_0["n_valid"]).all() and (out_m["n_valid"] > 1).all()
    # the per-sample, reference-shaped loop hands the flag to nn_correspondences
    torch.manual_seed(1)
    saved = np.random.get_state()
    try:
        np.random.seed(1)
        recs = pl_m.test_step(batch, 0)
    finally:
        np.random.set_state(saved)
    assert [r["status"] for r in recs] == [0, 0]
    for r in recs:
        T = r["pred_pose_rel"]
        assert T.shape == (4, 4) and T[3].tolist() == [0.0, 0.0, 0.0, 1.0] and bool(torch.isfinite(T).all())
    # an args object from before the flag existed keeps working
    old = default_args(**base)
    del old.test.mutual
    assert Pipeline(old, pointdsc_solver=None).test_step_batched(batch, first_pair_index=3)["status"].tolist() == [0, 0]


def test_run_pose_mutual_sets_the_default_and_records_the_flag(tmp_path):
    """run_pose.py --mutual: the flag becomes the process-wide default that the pipeline run_test.py builds reads, and the summary
    records it; without the flag the summary is run_test.py's own."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_pose
    from oryon_amd import engine
    out = str(tmp_path / "pred.csv")
    common = ["--solver", "ransac", "--pairs", "4", "--batch", "2", "--size", "64", "--channels", "32", "--out", out]
    try:
        s = run_pose.main(common + ["--mutual"])
        assert engine.default_mutual() is True and s["mutual"] is True and s["pairs"] == 4 and s["failures"] == 0
        s0 = run_pose.main(common)
        assert engine.default_mutual() is False and "mutual" not in s0 and s0["pairs"] == 4
    finally:
        engine.set_default_mutual(False)
        engine.set_default_solver("pointdsc")
