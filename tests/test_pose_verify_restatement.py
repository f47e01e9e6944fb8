"""CPU tests of depth-consistency pose verification (g4): the numpy restatement of its definition (tests/pose_verify_restatement.py) on
the fixtures the GPU tests use - that every class occurs, that every discrete decision stands by a margin rounding cannot cross, that
the candidate nearest the truth is the one selected - the selection rule on hand-made tables, the C ABI of csrc/pose_verify.hip
(symbols, caps, the workspace formula and every argument check, which runs before any HIP call: 0x1000 stands for a non-NULL pointer
that is never dereferenced) and the flags of the layers above.  No GPU is touched."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_plane_restatement as P  # noqa: E402
import pose_verify_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9
FULL = (1, 2, 3, 4)                        # pair 5 holds five rows: too few for every class to occur
MAX_ROWS, MAX_POSES, CLASSES = 8192, 16, 7
T0, T_GT, FAR, NEAR = range(4)             # the order of R.candidates


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("k", FULL)
@pytest.mark.parametrize("tol", R.TOLS)
def test_every_class_occurs_at_the_start_pose(k, tol):
    c = R.restated(k, tol)["counts"]
    print(k, tol, c.tolist())
    assert (c[T0] >= 1).all()


@pytest.mark.parametrize("k", sorted(P.FIXTURES))
@pytest.mark.parametrize("tol", R.TOLS)
def test_margins_of_every_discrete_decision(k, tol):
    """u + .5 and v + .5 from an integer (pixels) and | |d| - tol | (metres), over the four candidates - and the sixteen."""
    for which in ("four", "sixteen"):
        r = R.restated(k, tol, which)
        print(k, tol, which, "frac_gap %.3e px, tol_gap %.3e m" % (r["frac_gap"], r["tol_gap"]))
        assert r["frac_gap"] >= MARGIN and r["tol_gap"] >= MARGIN


@pytest.mark.parametrize("k", FULL)
@pytest.mark.parametrize("tol", R.TOLS)
def test_the_true_pose_has_the_most_hits_and_the_shifted_ones_none(k, tol):
    c = R.restated(k, tol)["counts"]
    hits = c[:, R.HIT]
    print(k, tol, "hits", hits.tolist())
    assert hits[T_GT] > max(hits[T0], hits[FAR], hits[NEAR]) and hits[FAR] == 0 and hits[NEAR] == 0
    assert c[FAR, R.OCCLUDED] >= 250 and c[NEAR, R.VIOLATION] >= 80          # pushed behind the surface; pulled in front of it
    assert R.restated(k, tol)["best"] == T_GT
    if tol == 0.005:
        assert int(hits[T_GT]) == {1: 127, 2: 97, 3: 116, 4: 127}[k]
        assert max(hits[T0], hits[FAR], hits[NEAR]) <= {1: 12, 2: 45, 3: 28, 4: 20}[k]


@pytest.mark.parametrize("k", FULL)
def test_best_follows_the_true_pose_through_the_list(k):
    f = P.fixture(k)
    cand = R.candidates(f)
    for order in ([0, 1, 2, 3], [1, 0, 2, 3], [3, 2, 0, 1], [2, 3, 1, 0], [0, 2, 3, 1]):
        r = R.verify(f["src"], f["depth"], f["mask"], f["cam9"], cand[order], 0.005)
        assert r["best"] == order.index(T_GT)
        assert np.array_equal(r["counts"], R.restated(k, 0.005)["counts"][order])


@pytest.mark.parametrize("k", sorted(P.FIXTURES))
def test_the_loop_version_equals_the_vectorised_one_and_counts_sum_to_n(k):
    f = P.fixture(k)
    n = f["src"].shape[0]
    for tol in R.TOLS:
        r = R.restated(k, tol)
        loop = R.classify_loop(f["src"], f["depth"], f["mask"], f["cam9"], R.candidates(f), tol)
        assert np.array_equal(loop["cls"], r["cls"]) and np.array_equal(loop["counts"], r["counts"])
        assert (r["counts"].sum(axis=1) == n).all() and r["cls"].min() >= 0 and r["cls"].max() <= 6
        assert np.allclose(r["score"], r["counts"][:, R.HIT] / n)


def test_pairs_that_do_not_run_and_counts_beyond_the_capacity():
    f = P.fixture(2)
    cand = R.candidates(f)
    for r in (R.verify(f["src"], f["depth"], f["mask"], f["cam9"], cand, 0.01, status_in=2), R.verify(f["src"], f["depth"], f["mask"], f["cam9"], cand, 0.01, n_s=0)):
        assert not r["counts"].any() and r["best"] == 0 and (r["cls"] == -1).all() and not r["score"].any()
    r = R.verify(f["src"], f["depth"], f["mask"], f["cam9"], cand, 0.01, n_s=10 ** 6)
    assert np.array_equal(r["counts"], R.restated(2, 0.01)["counts"])
    r = R.verify(f["src"], f["depth"], f["mask"], f["cam9"], cand, 0.01, n_s=100)
    assert (r["counts"].sum(axis=1) == 100).all() and (r["cls"][:, 100:] == -1).all() and (r["cls"][:, :100] >= 0).all()


def test_a_nan_row_is_behind_and_a_nan_or_infinite_depth_is_unknown():
    f = P.fixture(4)
    src = f["src"].copy()
    src[7] = np.nan
    depth = f["depth"].copy()
    base = R.restated(4, 0.01)
    hit_rows = np.nonzero(base["cls"][T_GT] == R.HIT)[0]
    r = R.verify(src, depth, f["mask"], f["cam9"], R.candidates(f), 0.01)
    assert (r["cls"][:, 7] == R.BEHIND).all()
    depth[:] = np.where(f["depth"] > 0, np.float32(np.inf), np.float32(np.nan))
    r = R.verify(f["src"], depth, f["mask"], f["cam9"], R.candidates(f), 0.01)
    assert (r["cls"][T_GT][hit_rows] == R.UNKNOWN).all() and r["counts"][:, R.OCCLUDED:].sum() == 0


# ------------------------------------------------------------------------------------------------------------------ the selection rule
def table(*rows):
    """rows of (hit, behind, violation, off): the rest of a row's 100 points is OCCLUDED, which is neutral."""
    t = np.zeros((len(rows), CLASSES), dtype=np.int32)
    for k, (h, b, v, o) in enumerate(rows):
        t[k, R.HIT], t[k, R.BEHIND], t[k, R.VIOLATION], t[k, R.OFF] = h, b, v, o
        t[k, R.OCCLUDED] = 100 - h - b - v - o
    return t


def test_selection_rule_on_hand_made_tables():
    assert R.select(table((10, 0, 0, 0), (30, 50, 10, 10), (20, 0, 0, 0))) == 1           # hits first, whatever the bad count
    assert R.select(table((30, 5, 5, 5), (30, 4, 5, 5), (30, 5, 5, 4))) == 1              # a tie in hits: the fewest bad, then the first
    assert R.select(table((30, 0, 3, 0), (30, 1, 1, 1), (30, 3, 0, 0))) == 0              # behind, violation and off weigh the same
    assert R.select(table((30, 5, 5, 5), (30, 5, 5, 5), (30, 5, 5, 5))) == 0              # a full tie: the lower index
    assert R.select(table((5, 0, 0, 0), (30, 2, 2, 2), (30, 2, 2, 2), (30, 3, 2, 2))) == 1  # duplicated candidates: the first of them
    assert R.select(table((0, 100, 0, 0))) == 0 and R.select(table((0, 0, 0, 0), (0, 0, 0, 0))) == 0   # K = 1; nothing anywhere
    occluded = table((30, 1, 1, 1), (30, 1, 1, 1))
    occluded[1, R.OCCLUDED], occluded[1, R.UNKNOWN] = 0, 67                                # neutral classes do not break a tie
    assert R.select(occluded) == 0


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def Pt(v=0x1000):
    return ctypes.c_void_p(v)


def _lib():
    from oryon_amd import _lib
    return _lib.lib()


def _ok():
    return dict(src=Pt(), n_src=Pt(), cap_src=64, depth=Pt(), mask=Pt(), H=48, W=40, cam9=Pt(), B=2, poses=Pt(), K=4, tol=0.01, status_in=None,
                workspace=Pt(), workspace_bytes=1 << 20, counts=Pt(), best=Pt(), cls=None, stream=None)


def _call(**change):
    L = _lib()
    rc = L.oryon_pose_verify(*dict(_ok(), **change).values())
    return rc, L.oryon_last_error().decode()


def test_symbols_header_and_makefile():
    from oryon_amd import _lib, geo6d, ops
    for name in ("oryon_pose_verify_workspace_bytes", "oryon_pose_verify"):
        assert name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(_lib.lib(), name)
    assert callable(ops.pose_verify) and callable(geo6d.pose_depth_score)
    assert (ops.POSE_VERIFY_CLASSES, ops.POSE_VERIFY_MAX_POSES) == (CLASSES, MAX_POSES)
    header = open(os.path.join(ROOT, "include", "oryon_hip.h")).read()
    for line in (f"#define ORYON_POSE_VERIFY_CLASSES {CLASSES}", f"#define ORYON_POSE_VERIFY_MAX_POSES {MAX_POSES}",
                 "size_t oryon_pose_verify_workspace_bytes(int B, int cap_src, int K);", "int oryon_pose_verify("):
        assert line in header
    assert "pose_verify.hip" in open(os.path.join(ROOT, "oryon_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("key", ["src", "n_src", "depth", "mask", "cam9", "poses", "workspace", "counts", "best"])
def test_null_pointers_are_rejected(key):
    rc, err = _call(**{key: None})
    assert rc == -1 and "oryon_pose_verify: invalid argument" in err and key in err


def test_optional_pointers_may_be_null_and_b_zero_returns_ok():
    rc, err = _call(B=0)                                   # nothing to do: returns before any launch, status_in / cls NULL
    assert rc == 0, err
    rc, err = _call(B=0, H=(1 << 16) - 1, W=1 << 15)       # the largest map below 2^31 pixels passes the shape check
    assert rc == 0, err
    rc, err = _call(B=0, H=1, W=1, tol=0.0, K=MAX_POSES, cap_src=MAX_ROWS)
    assert rc == 0, err


@pytest.mark.parametrize("change,names", [
    (dict(K=0), "K >= 1"), (dict(K=MAX_POSES + 1), "K <="),
    (dict(cap_src=0), "cap_src"), (dict(cap_src=MAX_ROWS + 1), "cap_src"),
    (dict(B=-1), "B >= 0"), (dict(B=70000), "B <= 65535"),
    (dict(H=0), "H >= 1"), (dict(W=0), "W >= 1"), (dict(H=1 << 16, W=1 << 15), "H * W"),
    (dict(tol=-1.0), "tol >= 0"), (dict(tol=float("nan")), "tol >= 0"),
    (dict(src=Pt(0x1004)), "aligned8"), (dict(cam9=Pt(0x1002)), "aligned8"),
    (dict(workspace=Pt(0x1010)), "workspace"),
    (dict(workspace_bytes=0), "workspace_bytes"), (dict(workspace_bytes=16), "workspace_bytes"),
])
def test_bad_values_are_rejected_with_the_checks_name(change, names):
    rc, err = _call(**change)
    assert rc == -1 and "oryon_pose_verify: invalid argument" in err and names in err, err


def test_workspace_bytes_follows_the_documented_formula_and_one_byte_short_is_rejected():
    L = _lib()
    a256 = lambda x: (x + 255) // 256 * 256
    for B, cs, K in ((1, 1, 1), (2, 64, 4), (5, 255, 2), (5, 256, 2), (5, 257, 2), (7, 300, 4), (64, 2048, 2), (3, MAX_ROWS, MAX_POSES), (65535, 3, 1)):
        assert L.oryon_pose_verify_workspace_bytes(B, cs, K) == a256(B * ((cs + 255) // 256) * K * CLASSES * 4), (B, cs, K)
    for B, cs, K in ((0, 64, 2), (-1, 64, 2), (65536, 64, 2), (1, 0, 2), (1, MAX_ROWS + 1, 2), (1, 64, 0), (1, 64, MAX_POSES + 1)):
        assert L.oryon_pose_verify_workspace_bytes(B, cs, K) == 0, (B, cs, K)
    o = _ok()
    need = L.oryon_pose_verify_workspace_bytes(o["B"], o["cap_src"], o["K"])
    rc, err = _call(workspace_bytes=need - 1)
    assert rc == -1 and "workspace_bytes" in err
    rc, err = _call(workspace_bytes=need, B=0)
    assert rc == 0, err


def test_python_wrapper_names_the_failed_check_without_a_gpu():
    import torch
    from oryon_amd import ops
    src = torch.zeros(1, 8, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"pose_verify: src\.is_cuda"):
        ops.pose_verify(src, torch.tensor([8], dtype=torch.int32), torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int32),
                        torch.zeros(1, 9, dtype=torch.float64), torch.eye(4)[None])


# ------------------------------------------------------------------------------------------------------------------ flags
def test_pipeline_verify_flag_and_its_process_wide_default():
    from oryon_amd import pipeline
    from oryon_amd.pipeline import Pipeline, default_args
    assert pipeline.VERIFY_MODES == ("none", "score", "guard") and pipeline.default_verify() == ("none", 0.01)
    assert pipeline.REFINEMENTS == ("none", "icp", "icp_plane")                         # verification is not a fourth refinement
    args = default_args()
    assert args.test.verify == "none" and args.test.verify_tol == 0.01
    pl = Pipeline(default_args(**{"test.solver": "ransac"}))
    assert pl.verify_mode() == "none" and pl.verify_summary() == {} and pl.last_verify is None
    try:
        pipeline.set_default_verify("score", 0.02)
        a = default_args(**{"test.solver": "ransac"})
        assert (a.test.verify, a.test.verify_tol) == ("score", 0.02)
        assert (Pipeline(a).verify_mode(), Pipeline(a).verify_tol()) == ("score", 0.02)
        del a.test.verify, a.test.verify_tol                                            # arg objects without the flags: the default
        assert (Pipeline(a).verify_mode(), Pipeline(a).verify_tol()) == ("score", 0.02)
    finally:
        pipeline.set_default_verify("none")
    assert pipeline.default_verify() == ("none", 0.01) and default_args().test.verify == "none"
    a = default_args(**{"test.solver": "ransac"})
    del a.test.verify, a.test.verify_tol
    assert Pipeline(a).verify_mode() == "none"
    with pytest.raises(ValueError, match="nothing to choose from"):
        Pipeline(default_args(**{"test.verify": "guard", "test.solver": "ransac"}))
    for refine in ("icp", "icp_plane"):
        a = default_args(**{"test.verify": "guard", "test.solver": "ransac"})
        a.test.refine = refine
        assert Pipeline(a).verify_mode() == "guard"
    with pytest.raises(ValueError, match="Verification scores not implemented"):
        Pipeline(default_args(**{"test.verify": "scores", "test.solver": "ransac"}))
    with pytest.raises(ValueError):
        pipeline.set_default_verify("guards")
    with pytest.raises(ValueError, match="verify_tol"):
        Pipeline(default_args(**{"test.verify": "score", "test.verify_tol": -0.01, "test.solver": "ransac"}))
    assert pipeline.default_verify() == ("none", 0.01)


def test_verify_summary_of_the_pipeline_and_of_the_process():
    """What run_pose.py prints: the latest verifying pipeline's log reduced over its solved pairs (here filled by hand, on the host)."""
    import torch
    from oryon_amd import pipeline
    from oryon_amd.pipeline import Pipeline, default_args
    pipeline.set_default_verify("none")
    assert pipeline.verify_summary() == {}
    Pipeline(default_args(**{"test.solver": "ransac"}))
    assert pipeline.verify_summary() == {}                                              # a pipeline that does not verify leaves no trace
    a = default_args(**{"test.verify": "guard", "test.verify_tol": 0.02, "test.solver": "ransac"})
    a.test.refine = "icp"
    pl = Pipeline(a)
    assert pl.verify_summary() == pipeline.verify_summary() == {"verify": "guard", "verify_tol": 0.02, "verify_pairs": 0,
                                                               "verify_score_mean": None, "verify_refinements_kept": 0}
    pl._verify_log.append((torch.tensor([0, 1, 0]), torch.tensor([0.5, 0.0, 1.0], dtype=torch.float64), torch.tensor([1, 0, 0])))
    pl._verify_log.append((torch.tensor([0]), torch.tensor([0.25], dtype=torch.float64), torch.tensor([1])))
    want = {"verify": "guard", "verify_tol": 0.02, "verify_pairs": 3, "verify_score_mean": (0.5 + 1.0 + 0.25) / 3, "verify_refinements_kept": 2}
    assert pl.verify_summary() == pipeline.verify_summary() == want
    pipeline.set_default_verify("none")                                                 # a driver's new run starts empty
    assert pipeline.verify_summary() == {} and pl.verify_summary() == want


def test_match_pose_config_does_not_carry_the_flag():
    import dataclasses
    from oryon_amd.engine import MatchPoseConfig
    assert not any(f.name.startswith("verify") for f in dataclasses.fields(MatchPoseConfig))


def test_run_pose_parses_verify():
    sys.path.insert(0, ROOT)
    import run_pose
    p = run_pose.parse(["--verify", "guard", "--refine", "icp", "--solver", "ransac", "--pairs", "4"])
    assert p == ("ransac", ["--pairs", "4"]) and p.verify == "guard" and p.verify_tol == 0.01
    p = run_pose.parse(["--verify", "score", "--verify-tol", "0.005", "--pairs", "4"])
    assert p == ("pointdsc", ["--pairs", "4"]) and (p.verify, p.verify_tol) == ("score", 0.005)
    p = run_pose.parse([])
    assert p.verify == "none" and p.verify_tol == 0.01 and not p.mutual and p.ratio == 0.0
    with pytest.raises(SystemExit):
        run_pose.parse(["--verify", "guards"])
    with pytest.raises(SystemExit, match="nothing to choose from"):
        run_pose.main(["--verify", "guard", "--solver", "ransac"])
