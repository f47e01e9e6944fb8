"""CPU tests of the mutual nearest-neighbour matcher (csrc/match_mutual.hip, test.mutual): the two symbols, every argument check of
oryon_match_mutual_f32 by name, the workspace bound of the header, the flags of the façade and the drivers, and the numpy statement
of `mutual` (tests/mutual_restatement.py) against a brute-force float64 all-pairs.  The device side is tests/test_gpu_match_mutual.py."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutual_restatement as mr  # noqa: E402

NAMES = ("oryon_match_mutual_workspace_bytes", "oryon_match_mutual_f32")


def test_symbols_are_declared_bound_and_exported():
    from oryon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "oryon_hip.h")).read()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert "match_mutual.hip" in open(os.path.join(ROOT, "oryon_amd", "csrc", "Makefile")).read()
    assert len(_lib._PROTOS["oryon_match_mutual_f32"][1]) == 18 and len(_lib._PROTOS["oryon_match_mutual_workspace_bytes"][1]) == 3


def _args(**change):
    """A complete, acceptable argument list (fake non-null pointers: every check comes before any launch or dereference)."""
    a = dict(a_hat=0x1000, q_hat=0x1000, B=1, C=32, cap_a=256, cap_q=256, n_a=0x1000, n_q=0x1000, threshold=0.25, min_dist=0x1000,
             argmin=0x1000, valid=0x1000, rev_min_dist=0x1000, rev_argmin=0x1000, mutual=0x1000, workspace=0x1000, workspace_bytes=1 << 40,
             stream=None)
    a.update(change)
    return list(a.values())


@pytest.mark.parametrize("change,names", [
    (dict(a_hat=None), "a_hat"), (dict(q_hat=None), "q_hat"), (dict(n_a=None), "n_a"), (dict(n_q=None), "n_q"),
    (dict(min_dist=None), "min_dist"), (dict(argmin=None), "argmin"), (dict(valid=None), "valid"),
    (dict(rev_min_dist=None), "rev_min_dist"), (dict(rev_argmin=None), "rev_argmin"), (dict(mutual=None), "mutual"),
    (dict(C=48), "C % BK"), (dict(C=0), "C > 0"), (dict(cap_a=200), "cap_a % MT"), (dict(cap_a=0), "cap_a > 0"),
    (dict(cap_q=192 + 1), "cap_q % MT"), (dict(cap_q=128), "cap_q % 256"), (dict(B=-1), "B >= 0"), (dict(B=70000), "B <= 65535"),
])
def test_every_rejection_names_its_check(change, names):
    from oryon_amd import _lib
    L = _lib.lib()
    assert L.oryon_match_mutual_f32(*_args(**change)) == -1
    err = L.oryon_last_error().decode()
    assert "oryon_match_mutual_f32: invalid argument" in err and names in err, err


def test_workspace_refusals_and_the_no_op():
    from oryon_amd import _lib
    L = _lib.lib()
    need = L.oryon_match_mutual_workspace_bytes(1, 256, 256)
    assert need > 0
    for change in (dict(workspace=None), dict(workspace_bytes=0), dict(workspace_bytes=need - 1)):
        assert L.oryon_match_mutual_f32(*_args(**change)) != 0
        err = L.oryon_last_error().decode()
        assert "oryon_match_mutual_f32: workspace too small" in err, err
    # B == 0: nothing to do, nothing launched, no pointer looked at beyond the null checks
    assert L.oryon_match_mutual_f32(*_args(B=0, workspace=None, workspace_bytes=0)) == 0


def test_workspace_is_one_key_word_per_query_row_plus_k1s_split():
    """include/oryon_hip.h: ORYON_MATCH_MUTUAL_KEY_WORDS (a design constant: ONE 64-bit (distance, index) key per query row, no
    per-panel slab) 8-byte words per query row + oryon_match_workspace_bytes."""
    from oryon_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "oryon_hip.h")).read()
    words = int(re.search(r"#define ORYON_MATCH_MUTUAL_KEY_WORDS (\d+)", hdr).group(1))
    assert words == 1
    assert L.oryon_match_mutual_workspace_bytes(0, 5120, 50176) == 0 and L.oryon_match_mutual_workspace_bytes(4, 0, 256) == 0
    for B, cap_a, cap_q in ((1, 256, 256), (3, 512, 768), (9, 256, 1024), (64, 5120, 50176), (512, 2048, 256), (2, 5120, 147456)):
        got = L.oryon_match_mutual_workspace_bytes(B, cap_a, cap_q)
        assert 0 < got <= words * B * cap_q * 8 + L.oryon_match_workspace_bytes(B, cap_a), (B, cap_a, cap_q, got)
        assert got >= B * cap_q * 8
    assert L.oryon_match_mutual_workspace_bytes(64, 5120, 50176) < 2 * 64 * 50176 * 8 + L.oryon_match_workspace_bytes(64, 5120)


def test_flags_of_the_facade_and_the_drivers():
    from oryon_amd.engine import MatchPoseConfig
    from oryon_amd.pipeline import default_args
    assert MatchPoseConfig().mutual is False and MatchPoseConfig(mutual=True).mutual is True
    assert default_args().test.mutual is False and default_args(**{"test.mutual": True}).test.mutual is True
    with pytest.raises(ValueError, match="sample_first"):
        MatchPoseConfig(mutual=True, sample_first=1000)
    assert MatchPoseConfig(mutual=True, sample_first=0, half_descriptors=True).half_descriptors       # composes
    sys.path.insert(0, ROOT)
    import run_pose
    p = run_pose.parse(["--mutual"])
    assert p.mutual and p == ("pointdsc", [])                            # taken out, like --refine: it becomes the process-wide default
    p = run_pose.parse(["--pairs", "4", "--mutual", "--solver", "ransac"])
    assert p.mutual and p == ("ransac", ["--pairs", "4"])
    p = run_pose.parse(["--solver", "ransac", "--pairs", "4"])
    assert not p.mutual and p == ("ransac", ["--pairs", "4"])
    import inspect
    from oryon_amd import pcd
    sig = inspect.signature(pcd.nn_correspondences)
    assert list(sig.parameters)[:8] == ["feats1", "feats2", "mask1", "mask2", "threshold", "max_corrs", "subsample_source", "corrs_device"]
    assert list(sig.parameters)[8:] == ["mutual"] and sig.parameters["mutual"].default is False
    assert inspect.signature(pcd.match_presample).parameters["mutual"].default is False


def test_the_process_wide_default_reaches_config_and_args():
    """What run_pose.py --mutual sets: MatchPoseConfig() and default_args() follow it, an explicit value still wins."""
    from oryon_amd import engine
    from oryon_amd.pipeline import default_args
    assert engine.default_mutual() is False
    try:
        engine.set_default_mutual(True)
        assert engine.MatchPoseConfig().mutual is True and default_args().test.mutual is True
        assert engine.MatchPoseConfig(mutual=False).mutual is False and default_args(**{"test.mutual": False}).test.mutual is False
        with pytest.raises(ValueError, match="sample_first"):
            engine.MatchPoseConfig(sample_first=1000)
    finally:
        engine.set_default_mutual(False)
    assert engine.MatchPoseConfig().mutual is False and default_args().test.mutual is False


def test_an_engine_whose_config_was_changed_afterwards_still_refuses():
    from oryon_amd import engine
    cfg = engine.MatchPoseConfig(mutual=True)
    cfg.sample_first = 500
    with pytest.raises(ValueError, match="sample_first"):
        engine._check_mutual(cfg)


@pytest.mark.parametrize("seed,n_a,n_q,C,thr", [(0, 1, 1, 4, 0.25), (1, 7, 5, 3, 0.25), (2, 5, 9, 8, 0.1), (3, 12, 12, 2, 0.6), (4, 6, 6, 4, 0.0)])
def test_restatement_against_brute_force(seed, n_a, n_q, C, thr):
    rng = np.random.default_rng(seed)
    a, q = rng.normal(size=(n_a, C)), rng.normal(size=(n_q, C))
    if seed == 3:                                                        # exact duplicates: ties in both directions
        a[5] = a[2]
        a[9] = a[2]
        q[7] = q[1]
    bf = mr.brute_force(a, q, thr)
    got = mr.mutual_flags(bf["argmin"], bf["valid"], bf["rev_argmin"])
    assert np.array_equal(got, bf["mutual"])
    assert got.sum() <= min(n_a, n_q) and len(set(bf["argmin"][got].tolist())) == int(got.sum())      # pairwise distinct
    assert np.array_equal(bf["rev_min_dist"][bf["argmin"][got]], bf["min_dist"][got])
    if thr == 0.0:
        assert not got.any()
    if seed == 3:
        assert not got[5] and not got[9]                                 # a later duplicate never wins the reverse tie


def test_restatement_of_degenerate_pairs():
    assert mr.mutual_flags([], [], [0, 0]).shape == (0,)
    assert not mr.mutual_flags([0, 0], [0, 0], []).any()
    assert mr.mutual_flags([0, 0, 0], [1, 1, 1], [0]).tolist() == [True, False, False]
