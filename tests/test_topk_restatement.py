"""CPU tests of the one-to-many matcher (csrc/match_next.hip, oryon_topk_corrs, test.topk): the numpy statement of the ranks and of
the expansion (tests/topk_restatement.py) against a brute-force float64 all-pairs and against the ratio test's statement, the
planted-decoy pairs in float64 (tests/topk_cases.py), every argument check of the two C entries by name, and the flags of the façade,
the engine and the drivers.  The device side is tests/test_gpu_match_next.py and tests/test_gpu_topk_routes.py."""
import dataclasses
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ratio_restatement as rr  # noqa: E402
import topk_cases as tc  # noqa: E402
import topk_restatement as tr  # noqa: E402

NAMES = ("oryon_match_next_workspace_bytes", "oryon_match_next_f32", "oryon_topk_corrs_workspace_bytes", "oryon_topk_corrs")
GAP = 1e-5       # float32 cosine distances of <= 16-channel rows differ from float64 by < 1e-6: a decision 1e-5 clear is the same in both


def _f32_dist(a, q):
    a32 = (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    q32 = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return (np.float32(0.5) - np.float32(0.5) * (a32 @ q32.T)).astype(np.float32)


def _inputs(seed, n_a, n_q, W, C):
    rng = np.random.default_rng(seed)
    a, q = rng.normal(size=(n_a, C)), rng.normal(size=(n_q, C))
    roi = np.sort(rng.choice(W * ((n_q + W - 1) // W + 2), size=n_q, replace=False))      # a ragged ROI: distinct pixels, row-major
    return a, q, roi


# ------------------------------------------------------------------------------------------------ the statement against the brute force
@pytest.mark.parametrize("seed,n_a,n_q,W,C,N,K", [
    (0, 1, 1, 1, 4, 1, 4), (1, 7, 12, 4, 3, 1, 4), (2, 5, 20, 5, 8, 2, 3), (13, 12, 36, 6, 4, 3, 4), (4, 6, 30, 6, 16, 5, 2),
    (5, 9, 25, 5, 4, 64, 4), (6, 8, 40, 8, 6, 2, 4), (7, 10, 48, 7, 8, 4, 4)])
def test_ranks_against_brute_force(seed, n_a, n_q, W, C, N, K):
    a, q, roi = _inputs(seed, n_a, n_q, W, C)
    bd, bj = tr.brute_force(a, q, roi, W, N, K)
    an, qn = a / np.linalg.norm(a, axis=1, keepdims=True), q / np.linalg.norm(q, axis=1, keepdims=True)
    d64 = 0.5 * (1.0 - an @ qn.T)
    for i in range(n_a):                                                 # every rank is decided by more than GAP in float64
        row = np.sort(d64[i])
        assert n_q < 2 or np.diff(row).min() > GAP
    d32 = _f32_dist(a, q)
    cd, cj = tr.ranks(d32, roi, W, N, K)
    assert cd.dtype == np.float32 and cd.shape == (K, n_a) == cj.shape
    assert np.array_equal(cj, bj)
    assert np.array_equal(np.isinf(cd), np.isinf(bd)) and np.array_equal(np.isinf(cd), cj < 0)
    fin = np.isfinite(cd)
    assert np.allclose(cd[fin], bd[fin], atol=2e-6, rtol=0)
    # K = 1 is the argmin; the ranks do not decrease; a rank without a candidate is (inf, -1) from there on
    assert np.array_equal(cj[0], np.argmin(d32, axis=1)) and np.array_equal(tr.ranks(d32, roi, W, N, 1)[1][0], cj[0])
    assert (cd[1:] >= cd[:-1]).all()
    for r in range(1, K):
        gone = cj[r - 1] < 0
        assert (cj[r][gone] == -1).all() and np.isinf(cd[r][gone]).all()
    if N == 64 or n_q == 1:
        assert (cj[1:] == -1).all()
    # the ranks of one anchor are pairwise at least N pixels apart
    y, x = roi // W, roi % W
    for i in range(n_a):
        js = cj[:, i][cj[:, i] >= 0]
        for u in range(len(js)):
            for v in range(u):
                assert (y[js[u]] - y[js[v]]) ** 2 + (x[js[u]] - x[js[v]]) ** 2 >= N * N


@pytest.mark.parametrize("N", [1, 2, 3, 5, 7, 64])
def test_rank_two_is_the_second_minimum_of_the_ratio_test(N):
    a, q, roi = _inputs(11, 14, 60, 9, 8)
    d32 = _f32_dist(a, q)
    cd, cj = tr.ranks(d32, roi, 9, N, 2)
    second, sidx, _ = rr.second_and_keep(d32, roi, 9, N, cj[0], None, 0.9)
    assert cd[1].tobytes() == second.tobytes()
    assert np.array_equal(cj[1], np.where(np.isinf(second), -1, sidx))   # that statement writes 0 for "none"


def test_ranks_edges():
    d = np.array([[0.1, 0.1, 0.3, 0.1]], dtype=np.float32)              # pixels 0, 1, 2 of row 0 and pixel 0 of row 5 (W = 4)
    roi = [0, 1, 2, 20]
    cd, cj = tr.ranks(d, roi, 4, 1, 4)                                  # ties go to the first index, every pixel is its own disc
    assert cj[:, 0].tolist() == [0, 1, 3, 2] and cd[:, 0].tolist() == [np.float32(0.1)] * 3 + [np.float32(0.3)]
    cd, cj = tr.ranks(d, roi, 4, 2, 4)                                  # pixel 1 is inside pixel 0's disc, pixel 2 (distance 2) on its rim
    assert cj[:, 0].tolist() == [0, 3, 2, -1] and np.isinf(cd[3, 0])
    cd, cj = tr.ranks(d[:, :3], roi[:3], 4, 3, 3)
    assert cj[:, 0].tolist() == [0, -1, -1] and np.isinf(cd[1:, 0]).all()
    cd, cj = tr.ranks(np.zeros((2, 0), dtype=np.float32), [], 4, 1, 2)
    assert np.isinf(cd).all() and (cj == -1).all()


def test_expand_statement():
    cd = np.array([[0.10, 0.00, 0.20, 0.24], [0.15, 0.04, 0.21, np.inf], [0.30, 0.05, 0.2400001, np.inf]], dtype=np.float32)
    cj = np.array([[3, 4, 5, 6], [7, 8, 9, -1], [1, 2, 0, -1]])
    s, r = tr.expand(4, cd, cj, 0.25, 0.05)
    # slot 0: rank 2 at the margin's edge (0.15 <= float32(0.10 + 0.05)) is kept, rank 3 is over the threshold; slot 1: both;
    # slot 2: both within 0.05 and under 0.25; slot 3: nothing left
    assert s.tolist() == [0, 0, 1, 1, 1, 2, 2, 2, 3] and r.tolist() == [1, 2, 1, 2, 3, 1, 2, 3, 1]
    s, r = tr.expand(4, cd, cj, 0.25, 0.0)                               # margin 0: only exact ties of the nearest
    assert r.tolist() == [1, 1, 1, 1]
    s, r = tr.expand(4, cd, cj, 0.25, np.inf)                            # no margin: the threshold alone
    assert r.tolist() == [1, 2, 1, 2, 3, 1, 2, 3, 1]
    s, r = tr.expand(4, cd, cj, 0.5, np.inf)
    assert r.tolist() == [1, 2, 3, 1, 2, 3, 1, 2, 3, 1]
    s, r = tr.expand(2, cd, cj, 0.25, 0.05)                              # only the slots asked for
    assert s.tolist() == [0, 0, 1, 1, 1]
    s, r = tr.expand(0, cd, cj, 0.25, 0.05)
    assert len(s) == 0 and len(r) == 0
    # an infinite nearest distance (no query row) emits its rank-1 row only: inf <= inf + margin, but inf < thr fails
    s, r = tr.expand(1, np.full((2, 1), np.inf, dtype=np.float32), np.array([[0], [-1]]), 0.25, 0.1)
    assert r.tolist() == [1]


# ------------------------------------------------------------------------------------------------ the planted-decoy pairs, in float64
@pytest.mark.parametrize("index", tc.PAIRS)
def test_planted_pairs_are_what_the_device_tests_take_them_for(index):
    got = tc.conditions(index, tr.ranks)
    print(index, got)
    assert got["n"] == tc.PLANTED[index]
    assert got["d1_max"] <= 1e-12 and got["d2_min"] >= 1e-4 and got["d3_min"] - got["d2_max"] >= 0.05
    # what the routes see: at topk = 2 with the device tests' margin 0.05 half of a planted anchor's rows are inliers
    p = tc.planted_pair(index)
    assert len(np.unique(p["decoy_px"])) == len(p["decoy_px"]) and not np.intersect1d(p["decoy_px"], p["true_px"]).size
    dy, dx = p["decoy_px"] // tc.W - p["true_px"] // tc.W, p["decoy_px"] % tc.W - p["true_px"] % tc.W
    assert (dy * dy + dx * dx >= tc.DECOY_MIN_PX ** 2).all()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_declared_bound_and_exported():
    from oryon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "oryon_hip.h")).read()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert "match_next.hip" in open(os.path.join(ROOT, "oryon_amd", "csrc", "Makefile")).read()
    assert len(_lib._PROTOS["oryon_match_next_f32"][1]) == 19 and len(_lib._PROTOS["oryon_topk_corrs"][1]) == 36
    assert "K1n" in hdr and "K1k" in hdr


def _next_args(**change):
    """A complete, acceptable argument list (fake non-null pointers: every check comes before any launch or dereference)."""
    a = dict(a_hat=0x1000, q_hat=0x1000, B=1, C=32, cap_a=256, cap_q=256, n_a=0x1000, n_q=0x1000, roi_q=0x1000, roi_stride_q=256, W_q=16,
             radius=5, prev_argmin=0x1000, n_prev=1, next_dist=0x1000, next_argmin=0x1000, workspace=0x1000, workspace_bytes=1 << 40,
             stream=None)
    a.update(change)
    return list(a.values())


@pytest.mark.parametrize("change,names", [
    (dict(a_hat=None), "a_hat"), (dict(q_hat=None), "q_hat"), (dict(n_a=None), "n_a"), (dict(n_q=None), "n_q"), (dict(roi_q=None), "roi_q"),
    (dict(prev_argmin=None), "prev_argmin"), (dict(next_dist=None), "next_dist"), (dict(next_argmin=None), "next_argmin"),
    (dict(n_prev=0), "n_prev >= 1"), (dict(n_prev=4), "n_prev <= NEXT_PREV_MAX"),
    (dict(radius=0), "radius >= 1"), (dict(radius=1025), "radius <= 1024"),
    (dict(W_q=0), "W_q >= 1"), (dict(W_q=65536), "W_q <= 65535"), (dict(roi_stride_q=0), "roi_stride_q"),
    (dict(C=48), "C % BK"), (dict(C=0), "C > 0"), (dict(cap_a=200), "cap_a % MT"), (dict(cap_q=192 + 1), "cap_q % MT"),
    (dict(cap_q=128), "cap_q % 256"), (dict(B=-1), "B >= 0"), (dict(B=70000), "B <= 65535"),
])
def test_every_rejection_of_the_rank_scan_names_its_check(change, names):
    from oryon_amd import _lib
    L = _lib.lib()
    assert L.oryon_match_next_f32(*_next_args(**change)) == -1
    err = L.oryon_last_error().decode()
    assert "oryon_match_next_f32: invalid argument" in err and names in err, err


def _topk_args(**change):
    a = dict(a_hat=0x1000, q_hat=0x1000, B=1, C=32, cap_a=256, cap_q=256, roi_a=0x1000, roi_q=0x1000, roi_stride_a=256, roi_stride_q=256,
             n_a=0x1000, n_q=0x1000, min_dist=0x1000, argmin=0x1000, valid=0x1000, threshold=0.25, W=16, max_corrs=100, corr_rows=256,
             seed=1, pair_key=None, K=2, radius=5, margin=0.1, corrs=0x1000, rank=0x1000, n_valid=0x1000, n_sel=0x1000, status=0x1000,
             n_rows=0x1000, sel_rows=None, cand_dist=None, cand_argmin=None, workspace=0x1000, workspace_bytes=1 << 40, stream=None)
    a.update(change)
    return list(a.values())


@pytest.mark.parametrize("change,names", [
    (dict(a_hat=None), "a_hat"), (dict(q_hat=None), "q_hat"), (dict(roi_a=None), "roi_a"), (dict(roi_q=None), "roi_q"),
    (dict(n_a=None), "n_a"), (dict(n_q=None), "n_q"), (dict(min_dist=None), "min_dist"), (dict(argmin=None), "argmin"),
    (dict(valid=None), "valid"), (dict(corrs=None), "corrs"), (dict(n_valid=None), "n_valid"), (dict(status=None), "status"),
    (dict(rank=None), "rank && n_rows"), (dict(n_rows=None), "rank && n_rows"), (dict(K=1, rank=None), "n_rows"),
    (dict(K=0), "K >= 1"), (dict(K=5), "K <= 4"), (dict(K=1, sel_rows=0x1000), "sel_rows"), (dict(K=1, cand_dist=0x1000), "cand_dist"),
    (dict(radius=0), "radius >= 1"), (dict(radius=1025), "radius <= 1024"),
    (dict(margin=-0.1), "margin >= 0"), (dict(margin=float("nan")), "margin"),
    (dict(corr_rows=199), "corr_rows >= K * max_corrs"), (dict(K=4, corr_rows=399), "corr_rows >= K * max_corrs"),
    (dict(max_corrs=0), "max_corrs > 0"), (dict(W=0), "W >= 1"), (dict(W=65536), "W <= 65535"),
    (dict(roi_stride_a=0), "roi_stride_a"), (dict(roi_stride_q=0), "roi_stride_q"),
    (dict(C=48), "C % 32"), (dict(C=0), "C > 0"), (dict(cap_a=200), "cap_a %"), (dict(cap_q=192 + 1), "cap_q %"),
    (dict(cap_q=128), "cap_q % 256"), (dict(B=-1), "B >= 0"), (dict(B=70000), "B <= 65535"),
])
def test_every_rejection_of_topk_corrs_names_its_check(change, names):
    from oryon_amd import _lib
    L = _lib.lib()
    assert L.oryon_topk_corrs(*_topk_args(**change)) == -1
    err = L.oryon_last_error().decode()
    assert "oryon_topk_corrs: invalid argument" in err and names in err, err


def test_workspace_refusals_and_the_no_ops():
    from oryon_amd import _lib
    L = _lib.lib()
    need = L.oryon_match_next_workspace_bytes(1, 256)
    assert need > 0 and need == L.oryon_match_second_workspace_bytes(1, 256)              # K1's split buffers
    assert L.oryon_match_next_workspace_bytes(0, 256) == 0 and L.oryon_match_next_workspace_bytes(4, 0) == 0
    for change in (dict(workspace=None), dict(workspace_bytes=0), dict(workspace_bytes=need - 1)):
        assert L.oryon_match_next_f32(*_next_args(**change)) != 0
        assert "oryon_match_next_f32: workspace too small" in L.oryon_last_error().decode()
    assert L.oryon_match_next_f32(*_next_args(B=0, workspace=None, workspace_bytes=0)) == 0
    sizes = [L.oryon_topk_corrs_workspace_bytes(1, 32, 256, 100, K) for K in (1, 2, 3, 4)]
    assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3]                                   # the candidate tables grow with K
    # the gathered rows dominate: cap_s = 128 rows of C floats, not cap_a
    assert sizes[1] - sizes[0] < 128 * 32 * 4 + 128 * 4 * 4 + 128 * 4 + 4 * 128 * 4 + need + 8 * 256
    for bad in ((0, 32, 256, 100, 2), (1, 0, 256, 100, 2), (1, 32, 0, 100, 2), (1, 32, 256, 0, 2), (1, 32, 256, 100, 0), (1, 32, 256, 100, 5)):
        assert L.oryon_topk_corrs_workspace_bytes(*bad) == 0
    for K, need in zip((1, 2), sizes):
        for change in (dict(workspace=None), dict(workspace_bytes=0), dict(workspace_bytes=need - 1)):
            assert L.oryon_topk_corrs(*_topk_args(K=K, **change)) != 0
            assert "oryon_topk_corrs: workspace too small" in L.oryon_last_error().decode()
    assert L.oryon_topk_corrs(*_topk_args(B=0, workspace=None, workspace_bytes=0)) == 0
    assert L.oryon_topk_corrs(*_topk_args(B=0, K=1, rank=None, n_rows=None, n_sel=None, workspace=None, workspace_bytes=0)) == 0


# ------------------------------------------------------------------------------------------------ the flags
def test_flags_of_the_facade_the_engine_and_the_drivers():
    from oryon_amd import ops, pcd
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    from oryon_amd.pipeline import default_args
    c = MatchPoseConfig()
    assert (c.topk, c.topk_radius, c.topk_margin) == (1, 5, 0.1)
    names = [f.name for f in dataclasses.fields(MatchPoseConfig)]
    assert names[names.index("topk"):names.index("topk") + 3] == ["topk", "topk_radius", "topk_margin"]
    t = default_args().test
    assert (t.topk, t.topk_radius, t.topk_margin) == (1, 5, 0.1) and default_args(**{"test.topk": 3}).test.topk == 3
    assert MatchPoseConfig(topk=2, half_descriptors=True, match_mode="screened").topk == 2                 # composes
    for bad, word in ((dict(topk=0), "topk"), (dict(topk=5), "topk"), (dict(topk=2.5), "topk"), (dict(topk=2, topk_radius=0), "topk_radius"),
                      (dict(topk=2, topk_radius=1025), "topk_radius"), (dict(topk=2, topk_margin=-0.1), "topk_margin"),
                      (dict(topk=2, topk_margin=float("nan")), "topk_margin")):
        with pytest.raises(ValueError, match=word):
            MatchPoseConfig(**bad)
    assert MatchPoseConfig(topk=2, topk_margin=float("inf")).topk_margin == float("inf")
    # the solvers' row cap, named
    with pytest.raises(ValueError, match="2048.*row cap"):
        MatchPoseConfig(topk=4, n_corrs=513)
    assert MatchPoseConfig(topk=4, n_corrs=512).topk == 4 and MatchPoseConfig(topk=1, n_corrs=512).n_corrs == 512
    # the combinations that are refused say why
    with pytest.raises(ValueError, match="reverse ranks"):
        MatchPoseConfig(topk=2, mutual=True)
    with pytest.raises(ValueError, match="ratio test deletes"):
        MatchPoseConfig(topk=2, ratio=0.8)
    with pytest.raises(ValueError, match="first-stage subset"):
        MatchPoseConfig(topk=2, sample_first=1000)
    assert MatchPoseConfig(topk=1, mutual=True, ratio=0.8).topk == 1
    # n_cap follows K; a config changed afterwards is refused at run
    assert MatchPoseEngine(None, MatchPoseConfig(solver="ransac", n_corrs=200, topk=3)).n_cap == 640
    assert MatchPoseEngine(None, MatchPoseConfig(solver="ransac", n_corrs=200)).n_cap == 256
    from oryon_amd import engine
    cfg = MatchPoseConfig(topk=2)
    cfg.mutual = True
    with pytest.raises(ValueError, match="reverse ranks"):
        engine._check_topk(cfg)
    sys.path.insert(0, ROOT)
    import run_pose
    p = run_pose.parse(["--topk", "2", "--topk-radius", "3", "--topk-margin", "0.05"])
    assert p == ("pointdsc", []) and (p.topk, p.topk_radius, p.topk_margin) == (2, 3, 0.05)
    p = run_pose.parse(["--pairs", "4", "--topk", "3", "--solver", "ransac", "--mask", "oracle"])
    assert p == ("ransac", ["--pairs", "4", "--mask", "oracle"]) and (p.topk, p.topk_radius, p.topk_margin) == (3, 5, 0.1)
    p = run_pose.parse(["--solver", "ransac", "--pairs", "4"])
    assert p == ("ransac", ["--pairs", "4"]) and p.topk == 1 and p.ratio == 0.0 and not p.mutual
    for argv in (["--topk", "2", "--mutual"], ["--topk", "2", "--ratio", "0.8"], ["--topk", "7"], ["--topk", "2", "--topk-radius", "0"]):
        with pytest.raises(SystemExit):
            run_pose.main(argv + ["--solver", "ransac", "--pairs", "1"])
    assert engine.default_topk() == (1, 5, 0.1)                          # a refused value changes nothing
    sig = inspect.signature(pcd.nn_correspondences_topk)
    assert list(sig.parameters) == ["feats1", "feats2", "mask1", "mask2", "threshold", "max_corrs", "subsample_source", "corrs_device",
                                    "topk", "topk_radius", "topk_margin"]
    assert [sig.parameters[k].default for k in ("corrs_device", "topk", "topk_radius", "topk_margin")] == ["cuda", 1, 5, 0.1]
    sig = inspect.signature(pcd.match_presample)
    assert sig.parameters["topk"].default == 1 and sig.parameters["topk_radius"].default == 5
    assert list(inspect.signature(ops.match_next).parameters) == ["a_hat", "q_hat", "n_a", "n_q", "roi_q", "W_q", "radius", "prev_argmin", "out"]
    for kw in (dict(topk=0), dict(topk=5), dict(topk=2, topk_radius=0), dict(topk=2, mutual=True), dict(topk=2, ratio=0.5)):
        with pytest.raises(ValueError, match="topk"):
            pcd.match_presample(None, None, None, None, 0.25, **kw)
    with pytest.raises(ValueError, match="topk_margin"):
        pcd.nn_correspondences_topk(None, None, None, None, 0.25, 10, None, topk=2, topk_margin=-1.0)


def test_the_process_wide_default_reaches_config_and_args():
    """What run_pose.py --topk sets: MatchPoseConfig() and default_args() follow it, an explicit value still wins."""
    from oryon_amd import engine
    from oryon_amd.pipeline import default_args
    assert engine.default_topk() == (1, 5, 0.1)
    try:
        engine.set_default_topk(2, 3, 0.05)
        c = engine.MatchPoseConfig()
        assert (c.topk, c.topk_radius, c.topk_margin) == (2, 3, 0.05)
        t = default_args().test
        assert (t.topk, t.topk_radius, t.topk_margin) == (2, 3, 0.05)
        assert engine.MatchPoseConfig(topk=1).topk == 1 and default_args(**{"test.topk": 1}).test.topk == 1
        with pytest.raises(ValueError, match="reverse ranks"):
            engine.MatchPoseConfig(mutual=True)
        with pytest.raises(ValueError, match="topk"):
            engine.set_default_topk(9)
        assert engine.default_topk() == (2, 3, 0.05)
    finally:
        engine.set_default_topk(1, 5, 0.1)
    assert engine.MatchPoseConfig().topk == 1 and default_args().test.topk == 1
