"""CPU tests of the RANSAC solver's ground truth and plumbing: the float64 restatement (tests/ransac_restatement.py) reproduces the
reference's recorded poses (tests/golden/ransac_*.npz, written by tools/gen_goldens.py gen_ransac from utils/geo6d.py:75-120), the
Python restatement of the device's index formula gives the values the library's own rng_u32 gives, and the new configuration fields
exist on every layer."""
import ctypes
import glob
import os

import numpy as np
import pytest

import ransac_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ransac_*.npz")))
NAMES = [os.path.basename(f)[len("ransac_"):-len(".npz")] for f in FIXTURES]


def load(path):
    z = np.load(path)
    return dict(A=z["A"], B=z["B"], idx=z["idx"], max_iter=int(z["max_iter"]), match_err=float(z["match_err"]),
                fix_percent=float(z["fix_percent"]), pose=z["pose"], seed=int(z["seed"]), state_words=z["state_words"],
                state_pos=int(z["state_pos"]))


def test_all_seven_fixtures_are_present():
    assert NAMES == ["1_best_of_k", "2_exit_sampled", "3_exit_at_0", "4_n37", "5_all_zero", "6_n3", "7_workload"]


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_restatement_reproduces_the_reference(path):
    """All 12 entries of the pose within 1e-5 (the bar of PointDSC's seed transforms; measured: <= 1e-18 - both are
    float64 numpy over the same rows); the zero fixtures exactly zero."""
    f = load(path)
    r = rr.restate(f["A"], f["B"], f["idx"], f["max_iter"], f["match_err"], f["fix_percent"])
    d = float(np.abs(r["pose"] - f["pose"]).max())
    print(f"{os.path.basename(path)}: winner {r['winner']}, exited {r['exited']}, |restatement - reference| = {d:.3e}")
    assert r["pose"].shape == (3, 4) and d <= 1e-5
    if os.path.basename(path) in ("ransac_5_all_zero.npz", "ransac_6_n3.npz"):
        assert r["winner"] == -1 and not r["pose"].any() and not f["pose"].any()


def test_fixtures_meet_their_conditions():
    """What gen_ransac asserted when it drew the seeds still holds for the committed files."""
    want = {"1_best_of_k": dict(exited=False, min_count=20), "2_exit_sampled": dict(exited=True, k_pos=True, min_count=20),
            "3_exit_at_0": dict(exited=True, k_zero=True), "4_n37": dict(min_count=20), "5_all_zero": dict(distinct4=True), "6_n3": {},
            "7_workload": dict(min_count=20)}
    for path, name in zip(FIXTURES, NAMES):
        f, w = load(path), want[name]
        r = rr.restate(f["A"], f["B"], f["idx"], f["max_iter"], f["match_err"], f["fix_percent"])
        K = f["max_iter"]
        if f["A"].shape[0] >= 4:
            bad = rr.rank_deficient(f["idx"], K)
            print(f"{name}: {int(bad.sum())} of {K} hypotheses are rank-deficient (fewer than 3 distinct rows) and excluded")
            assert bad.sum() <= (0.02 if name == "7_workload" else 0.10) * K
            assert not (np.abs(r["err"][~bad] - f["match_err"]) < rr.G).any()
            assert r["winner"] <= 0 or not bad[r["winner"]]
        if "exited" in w:
            assert r["exited"] == w["exited"]
        if w.get("k_pos"):
            assert r["winner"] > 0
        if w.get("k_zero"):
            assert r["winner"] == 0
        if "min_count" in w:
            assert r["counts"][r["winner"]] >= w["min_count"]
        if w.get("distinct4"):
            assert all(len(set(row.tolist())) == 4 for row in f["idx"]) and r["counts"].max() == 0


def test_index_formula_restatement():
    """rng_u32 / mix64 of csrc/common.h in Python against values of the C functions themselves (computed once on the host from the
    header; mix64(0) is also splitmix64's published first output for state 0)."""
    assert rr.mix64(0) == 16294208416658607535 == 0xE220A8397B1DCDAF and rr.mix64(1) == 10451216379200822465
    # (seed, key, counter i, n) -> (rng_u32(seed, key, 3, i), (u32 * n) >> 32)
    table = {(1, 0, 0, 500): (424537328, 49), (1, 0, 1, 500): (905662151, 105), (1, 7, 5, 500): (1281741625, 149),
             (12345, 63, 39995, 500): (3487884484, 406), (1, 0, 2, 37): (2971725469, 25), (2**64 - 1, 1 << 40, 3, 2048): (460405459, 219)}
    for (seed, key, i, n), (u32, idx) in table.items():
        assert rr.rng_u32(seed, key, 3, i) == u32 and (u32 * n) >> 32 == idx
    t = rr.device_sample_idx(1, 0, 500, 2)
    assert t.shape == (2, 4) and t[0, 0] == 49 and t[0, 1] == 105
    assert rr.device_sample_idx(1, 7, 500, 2)[1, 1] == 149          # counter 4 k + j = 5


def test_new_configuration_fields():
    from oryon_amd import _lib
    from oryon_amd.engine import MatchPoseConfig
    cfg = MatchPoseConfig()
    assert cfg.solver == "pointdsc" and cfg.ransac_max_iter == 10000 and cfg.ransac_match_err == 0.001 and cfg.ransac_fix_percent == 0.9999
    assert "oryon_ransac_register" in _lib.EXPORTS and "oryon_ransac_workspace_bytes" in _lib.EXPORTS
    tail = _lib.EngineConfig._fields_[-4:]
    assert [f[0] for f in tail] == ["solver", "ransac_max_iter", "ransac_match_err", "ransac_fix_percent"]
    assert [f[1] for f in tail] == [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    assert _lib.EngineConfig().solver == 0                            # a zeroed struct keeps today's behaviour


def test_ransac_entry_points_validate_their_arguments():
    from oryon_amd import _lib
    L = _lib.lib()
    assert L.oryon_ransac_workspace_bytes(64, 512, 10000) > 0
    assert L.oryon_ransac_workspace_bytes(64, 2048, 10000) > 0 and L.oryon_ransac_workspace_bytes(64, 2049, 10000) == 0
    assert L.oryon_ransac_workspace_bytes(0, 512, 10000) == 0 and L.oryon_ransac_workspace_bytes(1, 512, 0) == 0
    # more than 2048 rows per pair: ORYON_ERR_INVALID_ARG before anything is launched
    assert L.oryon_ransac_register(None, None, None, 1, 2176, 16, 0.001, 0.9999, None, 1, None, None, None, 0, None, None, None, None,
                                   None, None) == -1
    assert b"2048" in L.oryon_last_error()
    assert L.oryon_ransac_register(None, None, None, 1, 512, 16, 0.001, 0.9999, None, 1, None, None, None, 0, None, None, None, None,
                                   None, None) == -1
    # the engine sizes its arena without a PointDSC handle only for the RANSAC solver
    kw = dict(B=2, C=32, FH=16, FW=16, HA=16, WA=16, HQ=16, WQ=16, layout=0, dist_th=0.25, n_corrs=500, src_sampling=5000, seed=1, round_f16=0,
              n_slots=6, overlap=2, gather_sets=2, reg_streams=2, reg_lag=0, screen=1, sample_first=0, x3_prefetch=1, stream_roles=0)
    ransac = _lib.EngineConfig(solver=1, ransac_max_iter=10000, ransac_match_err=0.001, ransac_fix_percent=0.9999, **kw)
    assert L.oryon_engine_arena_bytes(ctypes.byref(ransac), None) > 0
    assert L.oryon_engine_arena_bytes(ctypes.byref(_lib.EngineConfig(**kw)), None) == 0
    bad = _lib.EngineConfig(solver=1, ransac_max_iter=0, ransac_match_err=0.001, ransac_fix_percent=0.9999, **kw)
    assert L.oryon_engine_arena_bytes(ctypes.byref(bad), None) == 0
    assert L.oryon_engine_arena_bytes(ctypes.byref(_lib.EngineConfig(solver=2, **kw)), None) == 0


def test_solver_names_are_checked_on_the_host():
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    MatchPoseEngine(None, MatchPoseConfig(solver="ransac"))           # no PointDSC model needed
    with pytest.raises(ValueError):
        MatchPoseEngine(None, MatchPoseConfig())
    with pytest.raises(ValueError):
        MatchPoseEngine(None, MatchPoseConfig(solver="icp"))


def test_default_solver_setting_and_driver_arguments(capsys):
    """run_pose.py --solver: parsed, rejected when unknown, handed on as the process-wide default that default_args() and
    MatchPoseConfig() read; everything else is left for run_test.py."""
    import sys
    sys.path.insert(0, ROOT)
    import run_pose
    from oryon_amd import engine
    from oryon_amd.pipeline import default_args
    assert run_pose.parse([]) == ("pointdsc", [])
    assert run_pose.parse(["--pairs", "8", "--solver", "ransac", "--per-sample"]) == ("ransac", ["--pairs", "8", "--per-sample"])
    with pytest.raises(SystemExit):
        run_pose.parse(["--solver", "icp"])
    capsys.readouterr()
    assert engine.default_solver() == "pointdsc" and default_args().test.solver == "pointdsc"
    try:
        engine.set_default_solver("ransac")
        assert default_args().test.solver == "ransac" and engine.MatchPoseConfig().solver == "ransac"
        assert engine.MatchPoseConfig(solver="pointdsc").solver == "pointdsc" and default_args(**{"test.solver": "pointdsc"}).test.solver == "pointdsc"
        with pytest.raises(ValueError):
            engine.set_default_solver("icp")
        assert engine.default_solver() == "ransac"
    finally:
        engine.set_default_solver("pointdsc")
    assert engine.MatchPoseConfig().solver == "pointdsc"
