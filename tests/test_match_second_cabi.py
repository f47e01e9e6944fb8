"""CPU tests of the ratio test with an exclusion disc (csrc/match_second.hip, test.ratio): the two symbols, every argument check of
oryon_match_second_f32 by name, the workspace refusals, the flags of the façade, the engine and the drivers, and the numpy statement
of the definition (tests/ratio_restatement.py) against a brute-force float64 all-pairs.  The device side is
tests/test_gpu_match_second.py and tests/test_gpu_ratio_routes.py."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ratio_restatement as rr  # noqa: E402

NAMES = ("oryon_match_second_workspace_bytes", "oryon_match_second_f32")


def test_symbols_are_declared_bound_and_exported():
    from oryon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "oryon_hip.h")).read()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert "match_second.hip" in open(os.path.join(ROOT, "oryon_amd", "csrc", "Makefile")).read()
    assert len(_lib._PROTOS["oryon_match_second_f32"][1]) == 22 and len(_lib._PROTOS["oryon_match_second_workspace_bytes"][1]) == 2
    assert "K1r" in hdr


def _args(**change):
    """A complete, acceptable argument list (fake non-null pointers: every check comes before any launch or dereference)."""
    a = dict(a_hat=0x1000, q_hat=0x1000, B=1, C=32, cap_a=256, cap_q=256, n_a=0x1000, n_q=0x1000, roi_q=0x1000, roi_stride_q=256, W_q=16,
             radius=5, min_dist=0x1000, argmin=0x1000, gate=0x1000, ratio=0.8, second_dist=0x1000, second_argmin=0x1000, keep=0x1000,
             workspace=0x1000, workspace_bytes=1 << 40, stream=None)
    a.update(change)
    return list(a.values())


@pytest.mark.parametrize("change,names", [
    (dict(a_hat=None), "a_hat"), (dict(q_hat=None), "q_hat"), (dict(n_a=None), "n_a"), (dict(n_q=None), "n_q"), (dict(roi_q=None), "roi_q"),
    (dict(min_dist=None), "min_dist"), (dict(argmin=None), "argmin"), (dict(second_dist=None), "second_dist"),
    (dict(second_argmin=None), "second_argmin"), (dict(keep=None), "keep"),
    (dict(radius=0), "radius >= 1"), (dict(radius=1025), "radius <= 1024"),
    (dict(ratio=0.0), "ratio > 0"), (dict(ratio=1.5), "ratio <= 1"), (dict(ratio=float("nan")), "ratio"),
    (dict(W_q=0), "W_q >= 1"), (dict(W_q=65536), "W_q <= 65535"), (dict(roi_stride_q=0), "roi_stride_q"),
    (dict(C=48), "C % BK"), (dict(C=0), "C > 0"), (dict(cap_a=200), "cap_a % MT"), (dict(cap_q=192 + 1), "cap_q % MT"),
    (dict(cap_q=128), "cap_q % 256"), (dict(B=-1), "B >= 0"), (dict(B=70000), "B <= 65535"),
])
def test_every_rejection_names_its_check(change, names):
    from oryon_amd import _lib
    L = _lib.lib()
    assert L.oryon_match_second_f32(*_args(**change)) == -1
    err = L.oryon_last_error().decode()
    assert "oryon_match_second_f32: invalid argument" in err and names in err, err


def test_workspace_refusals_and_the_no_op():
    from oryon_amd import _lib
    L = _lib.lib()
    need = L.oryon_match_second_workspace_bytes(1, 256)
    assert need > 0 and need <= L.oryon_match_workspace_bytes(1, 256) + 512          # K1's split buffers, each padded to 256 bytes
    assert L.oryon_match_second_workspace_bytes(0, 256) == 0 and L.oryon_match_second_workspace_bytes(4, 0) == 0
    for change in (dict(workspace=None), dict(workspace_bytes=0), dict(workspace_bytes=need - 1)):
        assert L.oryon_match_second_f32(*_args(**change)) != 0
        err = L.oryon_last_error().decode()
        assert "oryon_match_second_f32: workspace too small" in err, err
    # B == 0: nothing to do, nothing launched, no pointer looked at beyond the null checks; a NULL gate is allowed
    assert L.oryon_match_second_f32(*_args(B=0, workspace=None, workspace_bytes=0)) == 0
    assert L.oryon_match_second_f32(*_args(B=0, gate=None, workspace=None, workspace_bytes=0)) == 0


def test_flags_of_the_facade_the_engine_and_the_drivers():
    from oryon_amd import pcd
    from oryon_amd.engine import MatchPoseConfig
    from oryon_amd.pipeline import default_args
    import dataclasses
    assert MatchPoseConfig().ratio == 0.0 and MatchPoseConfig().ratio_radius == 5
    assert [f.name for f in dataclasses.fields(MatchPoseConfig)][-2:] == ["ratio", "ratio_radius"]      # appended
    assert default_args().test.ratio == 0.0 and default_args().test.ratio_radius == 5
    assert default_args(**{"test.ratio": 0.7}).test.ratio == 0.7
    with pytest.raises(ValueError, match="sample_first") as e:
        MatchPoseConfig(ratio=0.8, sample_first=1000)
    assert "ratio" in str(e.value)
    assert MatchPoseConfig(ratio=0.8, mutual=True, half_descriptors=True).ratio == 0.8                   # composes
    for bad in (dict(ratio=-0.1), dict(ratio=1.5), dict(ratio=float("nan")), dict(ratio=0.5, ratio_radius=0),
                dict(ratio=0.5, ratio_radius=1025)):
        with pytest.raises(ValueError, match="ratio"):
            MatchPoseConfig(**bad)
    sys.path.insert(0, ROOT)
    import run_pose
    p = run_pose.parse(["--ratio", "0.8", "--ratio-radius", "3", "--mutual"])
    assert p == ("pointdsc", []) and p.ratio == 0.8 and p.ratio_radius == 3 and p.mutual
    p = run_pose.parse(["--pairs", "4", "--ratio", "0.9", "--solver", "ransac"])
    assert p == ("ransac", ["--pairs", "4"]) and p.ratio == 0.9 and p.ratio_radius == 5 and not p.mutual
    p = run_pose.parse(["--solver", "ransac", "--pairs", "4"])
    assert p == ("ransac", ["--pairs", "4"]) and p.ratio == 0.0 and p.ratio_radius == 5
    sig = inspect.signature(pcd.nn_correspondences)
    assert list(sig.parameters) == ["feats1", "feats2", "mask1", "mask2", "threshold", "max_corrs", "subsample_source", "corrs_device", "mutual"]
    sig = inspect.signature(pcd.nn_correspondences_filtered)
    assert list(sig.parameters) == ["feats1", "feats2", "mask1", "mask2", "threshold", "max_corrs", "subsample_source", "corrs_device",
                                    "mutual", "ratio", "ratio_radius"]
    assert [sig.parameters[k].default for k in ("corrs_device", "mutual", "ratio", "ratio_radius")] == ["cuda", False, 0.0, 5]
    sig = inspect.signature(pcd.match_presample)
    assert sig.parameters["ratio"].default == 0.0 and sig.parameters["ratio_radius"].default == 5
    assert list(inspect.signature(__import__("oryon_amd.ops", fromlist=["x"]).match_second).parameters) == [
        "a_hat", "q_hat", "n_a", "n_q", "roi_q", "W_q", "radius", "min_dist", "argmin", "gate", "ratio"]


def test_the_process_wide_default_reaches_config_and_args():
    """What run_pose.py --ratio sets: MatchPoseConfig() and default_args() follow it, an explicit value still wins."""
    from oryon_amd import engine
    from oryon_amd.pipeline import default_args
    assert engine.default_ratio() == (0.0, 5)
    try:
        engine.set_default_ratio(0.8, 3)
        assert engine.default_ratio() == (0.8, 3)
        c = engine.MatchPoseConfig()
        assert (c.ratio, c.ratio_radius) == (0.8, 3) and (default_args().test.ratio, default_args().test.ratio_radius) == (0.8, 3)
        assert engine.MatchPoseConfig(ratio=0.0).ratio == 0.0 and default_args(**{"test.ratio": 0.0}).test.ratio == 0.0
        with pytest.raises(ValueError, match="sample_first"):
            engine.MatchPoseConfig(sample_first=1000)
        with pytest.raises(ValueError, match="ratio"):
            engine.set_default_ratio(1.5, 3)
        with pytest.raises(ValueError, match="ratio_radius"):
            engine.set_default_ratio(0.5, 0)
        assert engine.default_ratio() == (0.8, 3)                        # a refused value changes nothing
    finally:
        engine.set_default_ratio(0.0, 5)
    assert engine.MatchPoseConfig().ratio == 0.0 and default_args().test.ratio == 0.0 and engine.default_ratio() == (0.0, 5)


def test_an_engine_whose_config_was_changed_afterwards_still_refuses():
    from oryon_amd import engine
    cfg = engine.MatchPoseConfig(ratio=0.8)
    cfg.sample_first = 500
    with pytest.raises(ValueError, match="sample_first"):
        engine._check_ratio(cfg)
    cfg = engine.MatchPoseConfig()
    cfg.ratio = 2.0
    with pytest.raises(ValueError, match="ratio"):
        engine._check_ratio(cfg)


def test_the_facade_refuses_values_out_of_range_before_it_touches_a_device():
    from oryon_amd import pcd
    for kw in (dict(ratio=1.5), dict(ratio=-1.0), dict(ratio=float("nan")), dict(ratio=0.5, ratio_radius=0), dict(ratio=0.5, ratio_radius=2000)):
        with pytest.raises(ValueError, match="ratio"):
            pcd.match_presample(None, None, None, None, 0.25, **kw)


# ------------------------------------------------------------------------------------------------ the statement against the brute force
GAP = 1e-5       # float32 cosine distances of <= 16-channel rows differ from float64 by < 1e-6: a decision 1e-5 clear is the same in both


def _f32_dist(a, q):
    a32 = (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    q32 = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return (np.float32(0.5) - np.float32(0.5) * (a32 @ q32.T)).astype(np.float32)


@pytest.mark.parametrize("seed,n_a,n_q,W,C,r,ratio,thr", [
    (0, 1, 1, 1, 4, 1, 0.8, 0.6), (1, 7, 12, 4, 3, 1, 0.8, 0.6), (2, 5, 20, 5, 8, 2, 0.9, 0.5), (3, 12, 36, 6, 4, 3, 0.7, 0.4),
    (4, 6, 30, 6, 16, 5, 0.95, 0.6), (5, 9, 25, 5, 4, 64, 0.5, 0.6), (6, 8, 40, 8, 6, 2, 1.0, 0.3)])
def test_restatement_against_brute_force(seed, n_a, n_q, W, C, r, ratio, thr):
    rng = np.random.default_rng(seed)
    a, q = rng.normal(size=(n_a, C)), rng.normal(size=(n_q, C))
    roi = np.sort(rng.choice(W * ((n_q + W - 1) // W + 2), size=n_q, replace=False))      # a ragged ROI: distinct pixels, row-major
    bf = rr.brute_force(a, q, roi, W, r, ratio, thr)
    # the guaranteed gap, in float64: the nearest row, the nearest candidate, the threshold and the ratio cut are all decided by more
    # than GAP, so float32 arithmetic decides them the same way
    an, qn = a / np.linalg.norm(a, axis=1, keepdims=True), q / np.linalg.norm(q, axis=1, keepdims=True)
    d64 = 0.5 * (1.0 - an @ qn.T)
    y, x = roi // W, roi % W
    for i in range(n_a):
        row = np.sort(d64[i])
        assert n_q < 2 or row[1] - row[0] > GAP
        j0 = bf["argmin"][i]
        cand = np.sort(d64[i][(y - y[j0]) ** 2 + (x - x[j0]) ** 2 >= r * r])
        assert len(cand) < 2 or cand[1] - cand[0] > GAP
        assert abs(bf["min_dist"][i] - thr) > GAP
        assert np.isinf(bf["second_dist"][i]) or ratio == 1.0 or abs(bf["min_dist"][i] - ratio * bf["second_dist"][i]) > GAP
    d32 = _f32_dist(a, q)
    am = np.argmin(d32, axis=1)
    assert np.array_equal(am, bf["argmin"])
    gate = d32[np.arange(n_a), am] < np.float32(thr)
    second, sidx, keep = rr.second_and_keep(d32, roi, W, r, am, gate, ratio)
    assert second.dtype == np.float32
    assert np.array_equal(sidx, bf["second_argmin"]) and np.array_equal(np.isinf(second), np.isinf(bf["second_dist"]))
    fin = np.isfinite(second)
    assert np.allclose(second[fin], bf["second_dist"][fin], atol=2e-6, rtol=0)
    assert np.array_equal(keep, bf["keep"])
    assert (second >= d32[np.arange(n_a), am]).all()                     # a subset of the rows the minimum ran over
    if ratio == 1.0:
        assert np.array_equal(keep, gate)
    if r == 64 or n_q == 1:
        assert np.isinf(second).all() and not sidx.any() and np.array_equal(keep, gate)
    none = rr.second_and_keep(d32, roi, W, r, am, None, ratio)[2]
    assert np.array_equal(none & gate, keep)                             # the gate only ever removes rows


def test_restatement_edges():
    d = np.array([[0.1, 0.1, 0.3, 0.1]], dtype=np.float32)              # pixels 0, 1, 2 of row 0 and pixel 0 of row 5 (W = 4)
    roi = [0, 1, 2, 20]
    # r = 1: only the best pixel is excluded; the tie between rows 1 and 3 goes to the first
    s, j, k = rr.second_and_keep(d, roi, 4, 1, [0], [1], 0.99)
    assert s[0] == np.float32(0.1) and j[0] == 1 and not k[0]           # an exact copy outside the disc rejects the row at ratio < 1
    assert rr.second_and_keep(d, roi, 4, 1, [0], [1], 1.0)[2][0]
    # r = 2: pixel 1 is inside, pixel 2 (distance 2) is not: >= r^2 keeps the rim
    s, j, k = rr.second_and_keep(d, roi, 4, 2, [0], None, 0.5)
    assert j[0] == 3 and s[0] == np.float32(0.1)
    s, j, k = rr.second_and_keep(d[:, :3], roi[:3], 4, 2, [0], None, 0.5)
    assert j[0] == 2 and s[0] == np.float32(0.3) and k[0]               # 0.1 <= 0.15
    s, j, k = rr.second_and_keep(d[:, :3], roi[:3], 4, 3, [0], [0], 0.5)
    assert np.isinf(s[0]) and j[0] == 0 and not k[0]                    # no competitor keeps the row - the gate still rejects it
    assert rr.second_and_keep(d[:, :3], roi[:3], 4, 3, [0], [1], 0.5)[2][0]
    s, j, k = rr.second_and_keep(np.zeros((2, 0), dtype=np.float32), [], 4, 1, [0, 0], None, 0.5)
    assert np.isinf(s).all() and not j.any() and k.all()                 # inf <= inf
