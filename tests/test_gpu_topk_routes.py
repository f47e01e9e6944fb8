"""test.topk through every layer, on synthetic 48 x 48 pairs (C = 32, B = 4; solvers ransac and spectral: no weights):
ops.topk_corrs against the numpy statement of the expansion (tests/topk_restatement.py) applied to its own draws and candidate
tables, and those tables against ops.match_next on ALL rows; the engine against the by-hand recomputation through ops and against
the façade; the switched-off routes against today's calls; the refused combinations; and the case the feature exists for - the
planted-decoy pairs of tests/topk_cases.py - against the generator's own winner table.  The scan kernel itself is
tests/test_gpu_match_next.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_cases as tc  # noqa: E402
import topk_restatement as tr  # noqa: E402
from test_gpu_ransac import _batch  # noqa: E402  (the two-sided batch dict of Pipeline.test_step on the same synthetic pairs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, C, B = 48, 32, 4
THR = 0.25
R = 5


@pytest.fixture(scope="module")
def mb():
    from oryon_amd.synth import make_batch
    return make_batch(40, B, H, H, C, device=DEV)


@pytest.fixture(scope="module")
def planted():
    """the four planted pairs as a batch, after their float64 conditions have been asserted on the host"""
    for index in tc.PAIRS:
        tc.conditions(index, tr.ranks)
    items = [tc.planted_pair(i) for i in tc.PAIRS]
    out = {k: torch.stack([it[k] for it in items]).to(DEV) for k in ("feat_a", "feat_q", "mask_a", "mask_q", "depth_a", "depth_q", "camera", "pose")}
    out["winner"] = [it["winner"] for it in items]
    return out


@pytest.fixture(scope="module")
def matched(mb):
    """K0 + K1 on the batch, by hand: what ops.topk_corrs is given.  Pair 3's anchor mask is emptied in a second variant."""
    from oryon_amd import ops
    out = {}
    for name, mask_a in (("full", mb["mask_a"]), ("hole", torch.cat([mb["mask_a"][:3], torch.zeros_like(mb["mask_a"][3:])]))):
        roi_a, n_a = ops.roi_compact(mask_a)
        roi_q, n_q = ops.roi_compact(mb["mask_q"])
        cap = ops.round_up(H * H, ops.ROW_PAD)
        a_hat = ops.gather_normalise(mb["feat_a"].contiguous(), roi_a, n_a, cap)
        q_hat = ops.gather_normalise(mb["feat_q"].contiguous(), roi_q, n_q, cap)
        out[name] = dict(roi_a=roi_a, roi_q=roi_q, n_a=n_a, n_q=n_q, a_hat=a_hat, q_hat=q_hat)
    return out


def _match(m, thr):
    from oryon_amd import ops
    md, am, va = ops.match(m["a_hat"], m["q_hat"], m["n_a"], m["n_q"], thr)
    return md, am, va


def _full_tables(m, am, md, K, radius):
    """ranks of ALL anchor rows by K - 1 full scans: [K, B, cap_a]"""
    from oryon_amd import ops
    cd = torch.empty((K,) + tuple(md.shape), dtype=torch.float32, device=DEV)
    ca = torch.empty((K,) + tuple(am.shape), dtype=torch.int32, device=DEV)
    cd[0], ca[0] = md, am
    for r in range(1, K):
        ops.match_next(m["a_hat"], m["q_hat"], m["n_a"], m["n_q"], m["roi_q"], H, radius, ca[:r], out=(cd[r], ca[r]))
    return cd, ca


def _check_against_the_statement(m, md, am, out, K, thr, margin, max_corrs, corr_rows, full=None):
    """out: ops.topk_corrs(tables=True).  Exact: rows, ranks, counts and the untouched tail."""
    n_sel, n_rows = out["n_sel"].tolist(), out["n_rows"].tolist()
    sel, cd, ca = out["sel_rows"].cpu().numpy(), out["cand_dist"].cpu().numpy(), out["cand_argmin"].cpu().numpy()
    roi_a, roi_q = m["roi_a"].cpu().numpy().astype(np.int64), m["roi_q"].cpu().numpy().astype(np.int64)
    corrs, rank = out["corrs"].cpu().numpy(), out["rank"].cpu().numpy()
    md_np, am_np = md.cpu().numpy(), am.cpu().numpy()
    for p in range(len(n_sel)):
        n = n_sel[p]
        assert n in (0, max_corrs) and (n == max_corrs) == (int(out["status"][p]) == 0)
        rows = sel[p, :n]
        # rank 1 of the tables is K1's output of the drawn row; the later ranks are the full scans' rows, byte for byte
        assert cd[0, p, :n].tobytes() == md_np[p, rows].tobytes() and np.array_equal(ca[0, p, :n], am_np[p, rows])
        if full is not None:
            for r in range(1, K):
                assert cd[r, p, :n].tobytes() == full[0][r, p].cpu().numpy()[rows].tobytes(), (p, r)
                assert np.array_equal(ca[r, p, :n], full[1][r, p].cpu().numpy()[rows]), (p, r)
        assert np.isnan(cd[:, p, n:]).all() and (ca[:, p, n:] == -2).all() and (sel[p, n:] == -2).all()      # slots >= n_sel: not written
        s, r = tr.expand(n, cd[:, p, :n], ca[:, p, :n], thr, margin)
        assert n_rows[p] == len(s) and n <= n_rows[p] <= K * max_corrs
        pa = roi_a[p, rows[s]]
        pq = roi_q[p, ca[r - 1, p, s]]
        want = np.stack([pa // H, pa % H, pq // H, pq % H], axis=1)
        assert np.array_equal(corrs[p, :len(s)], want), p
        assert np.array_equal(rank[p, :len(s)], r), p
        assert not corrs[p, len(s):].any() and not rank[p, len(s):].any()                                  # the tail is left untouched
    return n_rows


# ------------------------------------------------------------------------------------------------ ops.topk_corrs
@pytest.mark.parametrize("K,thr,margin,max_corrs", [(2, 0.25, 0.05, 200), (3, 0.6, float("inf"), 200), (4, 0.6, 0.1, 130),
                                                    (4, 0.25, 0.0, 128), (2, 0.6, float("inf"), 700)])
def test_topk_corrs_is_the_statement_on_its_own_draws_and_tables(matched, K, thr, margin, max_corrs):
    from oryon_amd import ops
    for name in ("full", "hole"):
        m = matched[name]
        md, am, va = _match(m, thr)
        key = torch.arange(40, 40 + B, dtype=torch.int64, device=DEV)
        corr_rows = K * max_corrs + 37
        out = ops.topk_corrs(m["a_hat"], m["q_hat"], m["roi_a"], m["roi_q"], m["n_a"], m["n_q"], md, am, va, thr, H, max_corrs, 7, K, R,
                             margin, key, corr_rows=corr_rows, tables=True)
        torch.cuda.synchronize()
        assert out["sel_rows"].shape == (B, ops.round_up(max_corrs, 128)) and out["cand_dist"].shape == (K, B, ops.round_up(max_corrs, 128))
        full = _full_tables(m, am, md, K, R) if name == "full" else None
        n_rows = _check_against_the_statement(m, md, am, out, K, thr, margin, max_corrs, corr_rows, full)
        # the draws are oryon_select_corrs's: same slots, same counts, and the rank-1 rows are its rows in order
        sel = ops.select_corrs(m["roi_a"], m["roi_q"], m["n_a"], m["n_q"], am, va, H, max_corrs, 7, key)
        for k, t in zip(("n_valid", "n_sel", "status"), sel[1:]):
            assert torch.equal(out[k], t), k
        for p in range(B):
            first = out["corrs"][p, :n_rows[p]][out["rank"][p, :n_rows[p]] == 1]
            assert torch.equal(first, sel[0][p, :int(sel[2][p])]), p
        if name == "hole":
            assert int(out["status"][3]) == 1 and n_rows[3] == 0                       # ORYON_PAIR_NO_MASK: nothing drawn, nothing emitted
        if max_corrs == 700:
            assert (out["n_valid"][:3] < 700).all()                                    # drawn WITH replacement: slots repeat rows
        if margin == float("inf") and name == "full":
            assert max(n_rows) > max_corrs                                             # the case is not vacuous
        if margin == 0.0:
            assert n_rows == out["n_sel"].tolist()                                     # no exact ties on these pairs: rank 1 alone
    # a second run gives the same bytes
    again = ops.topk_corrs(m["a_hat"], m["q_hat"], m["roi_a"], m["roi_q"], m["n_a"], m["n_q"], md, am, va, thr, H, max_corrs, 7, K, R,
                           margin, key, corr_rows=corr_rows, tables=True)
    for k in ("corrs", "rank", "n_rows", "sel_rows", "cand_argmin"):
        assert torch.equal(out[k], again[k]), k


def test_k_one_is_select_corrs_byte_for_byte(matched):
    from oryon_amd import ops
    key = torch.arange(40, 40 + B, dtype=torch.int64, device=DEV)
    for name in ("full", "hole"):
        m = matched[name]
        md, am, va = _match(m, THR)
        for max_corrs, corr_rows in ((200, 256), (700, 700)):
            out = ops.topk_corrs(m["a_hat"], m["q_hat"], m["roi_a"], m["roi_q"], m["n_a"], m["n_q"], md, am, va, THR, H, max_corrs, 3, 1, R,
                                 0.1, key, corr_rows=corr_rows, tables=True)
            sel = ops.select_corrs(m["roi_a"], m["roi_q"], m["n_a"], m["n_q"], am, va, H, max_corrs, 3, key, corr_rows=corr_rows)
            assert set(out) == {"corrs", "rank", "n_valid", "n_sel", "status", "n_rows"}          # no tables at K = 1
            for k, t in zip(("corrs", "n_valid", "n_sel", "status"), sel):
                assert out[k].cpu().numpy().tobytes() == t.cpu().numpy().tobytes(), k
            assert torch.equal(out["n_rows"], out["n_sel"])
            for p in range(B):
                n = int(out["n_sel"][p])
                assert bool((out["rank"][p, :n] == 1).all()) and not out["rank"][p, n:].any()


def test_ops_refuse_what_they_would_have_to_convert(matched):
    from oryon_amd import _lib, ops
    m = matched["full"]
    md, am, va = _match(m, THR)
    args = [m["a_hat"], m["q_hat"], m["roi_a"], m["roi_q"], m["n_a"], m["n_q"], md, am, va, THR, H, 100, 1, 2, R, 0.1]
    for i, bad in ((0, m["a_hat"].double()), (2, m["roi_a"].long()), (6, md.double()), (7, am.long()), (8, va.bool())):
        with pytest.raises(AssertionError):
            ops.topk_corrs(*(args[:i] + [bad] + args[i + 1:]))
    for k, radius, margin in ((5, R, 0.1), (2, 0, 0.1), (2, R, -1.0)):
        with pytest.raises(_lib.OryonError):
            ops.topk_corrs(*(args[:13] + [k, radius, margin]))


# ------------------------------------------------------------------------------------------------ the engine
def _engine_run(mb, keep=True, solver="ransac", **cfg):
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    eng = MatchPoseEngine(None, MatchPoseConfig(solver=solver, dist_th=THR, **cfg))
    cam = mb["camera"].to(DEV)
    key = torch.arange(40, 40 + B, dtype=torch.int64, device=DEV)
    out = eng.run(mb["feat_a"], mb["feat_q"], mb["mask_a"], mb["mask_q"], mb["depth_a"], mb["depth_q"], cam, cam, key, keep=keep)
    torch.cuda.synchronize()
    return eng, out, key


def test_engine_with_topk_one_is_todays_run(mb):
    _, a, _ = _engine_run(mb)
    eng, b, _ = _engine_run(mb, topk=1, topk_radius=7, topk_margin=0.3)
    assert set(a) == set(b) and "n_rows" not in a and "cand_dist" not in a and eng.n_cap == 512
    for k in ("pose", "status", "n_valid", "n_lifted", "corrs", "n_a"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    for match_mode in ("exact", "screened"):                             # no keep: whatever route the mode picks, the same poses
        x = _engine_run(mb, keep=False, match_mode=match_mode)[1]
        y = _engine_run(mb, keep=False, match_mode=match_mode, topk=1, topk_margin=0.0)[1]
        assert set(x) == set(y)
        for k in ("pose", "status", "n_valid", "n_lifted"):
            assert torch.equal(x[k], y[k]), (match_mode, k)


@pytest.mark.parametrize("K,margin,solver", [(2, 0.05, "ransac"), (4, float("inf"), "ransac"), (3, 0.1, "spectral")])
def test_engine_topk_equals_the_recomputation_through_ops_and_the_facade(mb, K, margin, solver):
    from oryon_amd import ops, pcd
    n_corrs = 200
    eng, out, key = _engine_run(mb, solver=solver, n_corrs=n_corrs, topk=K, topk_radius=R, topk_margin=margin, src_sampling=None,
                                match_mode="screened")
    assert eng._native is None and eng.n_cap == ops.round_up(n_corrs * K, 128)             # exact scan, per-call schedule
    for k in ("n_rows", "sel_rows", "cand_dist", "cand_argmin", "corr_rank", "corrs", "roi_a", "roi_q", "argmin", "valid", "min_dist"):
        assert k in out, k
    assert out["corrs"].shape == (B, eng.n_cap, 4) and out["corr_rank"].shape == (B, eng.n_cap)
    cap_a = out["argmin"].shape[1]
    a_hat = ops.gather_normalise(mb["feat_a"].contiguous(), out["roi_a"], out["n_a"], cap_a)
    q_hat = ops.gather_normalise(mb["feat_q"].contiguous(), out["roi_q"], out["n_q"], ops.round_up(H * H, ops.ROW_PAD))
    md, am, va = ops.match(a_hat, q_hat, out["n_a"], out["n_q"], THR)
    hand = ops.topk_corrs(a_hat, q_hat, out["roi_a"], out["roi_q"], out["n_a"], out["n_q"], md, am, va, THR, H, n_corrs, eng.cfg.seed, K, R,
                          margin, key, corr_rows=eng.n_cap, tables=True)
    for mine, theirs in (("corrs", "corrs"), ("corr_rank", "rank"), ("n_rows", "n_rows"), ("n_valid", "n_valid"), ("sel_rows", "sel_rows"),
                         ("cand_argmin", "cand_argmin")):
        assert torch.equal(out[mine], hand[theirs]), mine
    assert out["cand_dist"].cpu().numpy().tobytes() == hand["cand_dist"].cpu().numpy().tobytes()
    m = dict(roi_a=out["roi_a"], roi_q=out["roi_q"])
    _check_against_the_statement(m, md, am, hand, K, THR, margin, n_corrs, eng.n_cap)
    # the lift takes n_rows; the solver gets every lifted row
    cam = mb["camera"].to(DEV).reshape(B, 9).float().contiguous()
    _, _, n_lift = ops.lift_pairs(hand["corrs"], hand["n_rows"], (H, H), mb["depth_a"], mb["depth_q"], cam, cam, hand["status"])
    assert torch.equal(out["n_lifted"], n_lift) and (out["n_lifted"] > 3).all() and (out["n_lifted"] <= out["n_rows"]).all()
    assert out["status"].tolist() == [0] * B and bool(torch.isfinite(out["pose"]).all())
    # the façade's tables (K - 1 full scans over all rows) equal the engine's (scans of the drawn rows) on the same anchors
    for p in range(B):
        pre = pcd.match_presample(mb["feat_a"][p], mb["feat_q"][p], mb["mask_a"][p], mb["mask_q"][p], THR, topk=K, topk_radius=R,
                                  mode="screened8")
        assert set(pre) == {"roi1", "roi2", "min_dist", "argmin", "valid", "cand_dist", "cand_argmin"}
        assert pre["cand_dist"].shape == (K, int(out["n_a"][p])) and pre["cand_argmin"].dtype == torch.int64
        n = int(hand["n_sel"][p])
        rows = out["sel_rows"][p, :n].long()
        assert torch.equal(pre["cand_argmin"][:, rows], out["cand_argmin"][:, p, :n].long()), p
        assert pre["cand_dist"][:, rows].cpu().numpy().tobytes() == out["cand_dist"][:, p, :n].cpu().numpy().tobytes(), p
        assert torch.equal(pre["cand_argmin"][0], pre["argmin"]) and torch.equal(pre["cand_dist"][0], pre["min_dist"])


def test_a_margin_only_adds_rows_and_the_facade_without_topk_is_what_it_was(mb):
    from oryon_amd import pcd
    none = _engine_run(mb, n_corrs=200, topk=3, topk_margin=0.0, src_sampling=None)[1]
    wide = _engine_run(mb, n_corrs=200, topk=3, topk_margin=float("inf"), src_sampling=None)[1]
    assert (wide["n_rows"] >= none["n_rows"]).all() and (wide["n_rows"] > none["n_rows"]).any()
    for p in range(B):                                                   # the same draws: the rank-1 rows are the same rows in the same order
        a = none["corrs"][p, :int(none["n_rows"][p])][none["corr_rank"][p, :int(none["n_rows"][p])] == 1]
        b = wide["corrs"][p, :int(wide["n_rows"][p])][wide["corr_rank"][p, :int(wide["n_rows"][p])] == 1]
        assert torch.equal(a, b) and a.shape[0] == 200
    # the per-sample façade: topk = 1 is nn_correspondences, draws included; topk = 2 makes the same two draws
    args = (mb["feat_a"][2], mb["feat_q"][2], mb["mask_a"][2], mb["mask_q"][2], THR, 300, 400, "cpu")
    torch.manual_seed(9)
    one = pcd.nn_correspondences(*args)
    s_one = torch.get_rng_state()
    torch.manual_seed(9)
    same = pcd.nn_correspondences_topk(*args, topk=1, topk_radius=3, topk_margin=0.5)
    assert torch.equal(s_one, torch.get_rng_state()) and torch.equal(one, same)
    torch.manual_seed(9)
    two = pcd.nn_correspondences_topk(*args, topk=2, topk_radius=R, topk_margin=float("inf"))
    assert torch.equal(s_one, torch.get_rng_state())
    assert two.dtype == torch.int64 and 300 <= two.shape[0] <= 600 and two.shape[1] == 4
    torch.manual_seed(9)
    zero = pcd.nn_correspondences_topk(*args, topk=2, topk_radius=R, topk_margin=0.0)
    assert torch.equal(zero, one)                                        # margin 0, no exact ties: the rank-1 rows alone, in the draws' order
    for kw in (dict(), dict(subsample_source=500), dict(mode="screened8")):
        torch.manual_seed(3)
        a = pcd.match_presample(*args[:5], **kw)
        torch.manual_seed(3)
        b = pcd.match_presample(*args[:5], topk=1, topk_radius=9, **kw)
        assert set(a) == set(b) and "cand_dist" not in a
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    empty = torch.zeros_like(mb["mask_a"][1])
    pre = pcd.match_presample(mb["feat_a"][1], mb["feat_q"][1], mb["mask_a"][1], empty, THR, topk=3)
    assert pre["cand_dist"].shape == (3, pre["valid"].shape[0]) and bool(torch.isinf(pre["cand_dist"]).all()) and bool((pre["cand_argmin"] == -1).all())


def test_the_refused_combinations_raise(mb):
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    for kw, word in ((dict(mutual=True), "reverse ranks"), (dict(ratio=0.8), "ratio test deletes"), (dict(sample_first=100), "first-stage subset")):
        with pytest.raises(ValueError, match=word):
            MatchPoseConfig(solver="ransac", topk=2, **kw)
        eng = MatchPoseEngine(None, MatchPoseConfig(solver="ransac", topk=2))
        for k, v in kw.items():
            setattr(eng.cfg, k, v)
        cam = mb["camera"].to(DEV)
        with pytest.raises(ValueError, match=word):
            eng.run(mb["feat_a"], mb["feat_q"], mb["mask_a"], mb["mask_q"], mb["depth_a"], mb["depth_q"], cam, cam)
    with pytest.raises(ValueError, match="row cap"):
        MatchPoseConfig(solver="ransac", topk=3, n_corrs=700)


# ------------------------------------------------------------------------------------------------ the case the feature exists for
def _true_rows(winner, corrs, n):
    return tc.is_true_row(winner, corrs[:n].cpu().numpy())


def _pose_error(batch, pose):
    """mean distance (metres) between the anchor's masked cloud moved by `pose` and by the ground-truth pose, per pair"""
    errs = []
    for p in range(B):
        mask = batch["mask_a"][p].cpu().numpy() == 1
        z = batch["depth_a"][p].cpu().numpy().astype(np.float64)[mask] / 1000.0
        K = batch["camera"][p].cpu().numpy().astype(np.float64).reshape(3, 3)
        ys, xs = np.nonzero(mask)
        pts = np.stack([(xs - K[0, 2]) * z / K[0, 0], (ys - K[1, 2]) * z / K[1, 1], z], axis=1)
        T, G = pose[p].cpu().numpy().astype(np.float64), batch["pose"][p].cpu().numpy().astype(np.float64)
        errs.append(float(np.linalg.norm((pts @ T[:3, :3].T + T[:3, 3]) - (pts @ G[:3, :3].T + G[:3, 3]), axis=1).mean()))
    return errs


def test_planted_pairs_at_topk_one_give_the_solver_nothing_but_outliers(planted):
    _, out, _ = _engine_run(planted, n_corrs=256, src_sampling=None)
    assert out["status"].tolist() == [0] * B
    for p in range(B):
        assert not _true_rows(planted["winner"][p], out["corrs"][p], 256).any(), p


@pytest.mark.parametrize("solver", ["ransac", "spectral"])
def test_planted_pairs_at_topk_two_hand_over_the_true_rows(planted, mb, solver):
    n_corrs = 256
    _, out, _ = _engine_run(planted, solver=solver, n_corrs=n_corrs, topk=2, topk_radius=R, topk_margin=0.05, src_sampling=None)
    assert out["status"].tolist() == [0] * B
    for p in range(B):
        n = int(out["n_rows"][p])
        true = _true_rows(planted["winner"][p], out["corrs"][p], n)
        rank = out["corr_rank"][p, :n].cpu().numpy()
        share = true.sum() / n_corrs
        print(f"pair {tc.PAIRS[p]}: {n} rows, {int(true.sum())} true rows, share of the drawn anchors {share:.3f}")
        assert share >= 0.8, (p, share)                                  # the CPU shares (planted / 576) are 0.86 - 1.0
        assert (rank[true] == 2).all()                                   # every true row carries rank 2
    # the pose: against the UNPLANTED pairs at topk = 1 (today's route, pinned byte for byte above) in the same session
    _, base, _ = _engine_run(mb, solver=solver, n_corrs=n_corrs, src_sampling=None)
    e_planted, e_plain = _pose_error(planted, out["pose"]), _pose_error(mb, base["pose"])
    print(f"{solver}: mean point distance to the ground-truth pose, planted topk=2 {np.mean(e_planted):.6f} m {e_planted}, "
          f"unplanted topk=1 {np.mean(e_plain):.6f} m {e_plain}, ratio {np.mean(e_planted) / np.mean(e_plain):.3f}")
    assert np.mean(e_planted) <= 3.0 * np.mean(e_plain)


# ------------------------------------------------------------------------------------------------ pipeline and driver
def test_pipeline_per_sample_equals_batched_on_rows():
    """One pair, n_corrs = the pair's number of valid rows: both samplers then draw every valid row exactly once (the device one in
    row order, the host one as a permutation), so the two routes must emit the same rows."""
    from oryon_amd.pipeline import Pipeline, default_args
    base = {"test.mask": "oracle", "test.solver": "ransac", "model.image_encoder.img_size": [H, H], "dataset.img_size": [H, H],
            "test.src_sampling": None}
    batch, mbc = _batch(41, 1)
    probe = Pipeline(default_args(**base), pointdsc_solver=None).test_step_batched(batch, first_pair_index=41)
    nv = int(probe["n_valid"][0])
    assert 128 < nv <= 576
    flags = {**base, "test.n_corrs": nv, "test.topk": 2, "test.topk_radius": R, "test.topk_margin": float("inf")}
    assert default_args(**base).test.topk == 1
    pl = Pipeline(default_args(**flags), pointdsc_solver=None)
    out = pl.test_step_batched(batch, first_pair_index=41)
    torch.cuda.synchronize()
    cfg = pl._engine.cfg
    assert (cfg.topk, cfg.topk_radius, cfg.topk_margin, cfg.n_corrs) == (2, R, float("inf"), nv) and out["status"].tolist() == [0]
    assert nv < int(out["n_rows"][0]) <= 2 * nv
    cam = mbc["camera"].to(DEV)
    kept = pl._engine.run(batch["featmap_a"], batch["featmap_q"], mbc["mask_a"].to(DEV), mbc["mask_q"].to(DEV), mbc["depth_a"].to(DEV),
                          mbc["depth_q"].to(DEV), cam, cam, torch.tensor([41], device=DEV), keep=True)
    assert torch.equal(kept["n_rows"], out["n_rows"]) and torch.equal(kept["pose"], out["pose"][:, :4, :4].to(kept["pose"].dtype))
    rows_b = kept["corrs"][0, :int(kept["n_rows"][0])].cpu().tolist()
    torch.manual_seed(1)
    rows_s, _, _ = pl.get_featmap_corrs(batch, {"featmap_a": batch["featmap_a"], "featmap_q": batch["featmap_q"]}, {}, 0)
    assert rows_s.shape[0] == len(rows_b) and sorted(map(tuple, rows_s.cpu().tolist())) == sorted(map(tuple, rows_b))
    saved = np.random.get_state()
    try:
        np.random.seed(1)
        recs = pl.test_step(batch, 0)                                    # the per-sample solvers take the larger row count
    finally:
        np.random.set_state(saved)
    assert [r["status"] for r in recs] == [0]
    old = default_args(**base)                                           # an args object from before the flags existed keeps working
    del old.test.topk, old.test.topk_radius, old.test.topk_margin
    assert Pipeline(old, pointdsc_solver=None).test_step_batched(batch, first_pair_index=41)["status"].tolist() == [0]


def test_run_pose_topk_sets_the_default_and_records_the_flags(tmp_path, capsys):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_pose
    from oryon_amd import engine
    out = str(tmp_path / "pred.csv")
    try:
        s = run_pose.main(["--solver", "ransac", "--topk", "2", "--pairs", "4", "--batch", "2", "--size", "48", "--out", out])
        assert engine.default_topk() == (2, 5, 0.1)
        assert (s["topk"], s["topk_radius"], s["topk_margin"]) == (2, 5, 0.1) and s["pairs"] == 4
        last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert (last["topk"], last["topk_radius"], last["topk_margin"]) == (2, 5, 0.1)
        s0 = run_pose.main(["--solver", "ransac", "--pairs", "4", "--batch", "2", "--size", "48", "--out", out])
        assert engine.default_topk() == (1, 5, 0.1) and "topk" not in s0 and s0["pairs"] == 4
    finally:
        engine.set_default_topk(1, 5, 0.1)
        engine.set_default_solver("pointdsc")
