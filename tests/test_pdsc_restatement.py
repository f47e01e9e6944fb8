"""Pins tests/pdsc_restatement.py (the float64 statement the size sweep of the GPU solver is judged by) to recorded reference results:
the ten g4_pointdsc_* fixtures at the bars tests/test_oracle_goldens.py uses for the fp32 oracle, and the fp32 oracle itself on the
sweep's own inputs above 512 rows."""
import glob
import os

import numpy as np
import pytest
import torch

import pdsc_restatement as rs
import pdsc_sizes_cases as cases
from oracle import oryon_oracle as orc

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NAMES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "g4_pointdsc_*.npz")))
CFG = dict(num_iterations=10, ratio=0.1, sigma_d=0.1, k=40, nms_radius=0.1, inlier_threshold=0.1)


def test_fixtures_are_present():
    assert len(NAMES) == 10


@pytest.mark.parametrize("name", NAMES)
def test_reproduces_the_reference_fixtures(name):
    g = dict(np.load(os.path.join(GOLD, name), allow_pickle=False))
    n = int(g["n"])
    S = int(n * CFG["ratio"])
    sd = rs.seeds(g["src"], g["confidence"], CFG["nms_radius"], S)
    assert np.array_equal(sd["local_max"], g["is_local_max"].astype(bool))
    m = min(int(g["n_pos_max"]), S)       # the strictly positive local maxima are order-defined, the zero-key tail is not
    assert np.array_equal(sd["seeds"][:m], g["seeds"][:m].astype(np.int64))
    seeds = g["seeds"].astype(np.int64)
    hyp = rs.hypotheses(seeds, g["feat"], g["src"], g["tgt"], 1.0, CFG["sigma_d"], CFG["k"], CFG["num_iterations"], CFG["inlier_threshold"])
    ref_knn = g["knn_all"].astype(np.int64)[seeds]
    same = [set(a.tolist()) == set(b.tolist()) for a, b in zip(hyp["knn"], ref_knn)]
    assert np.mean(same) > 0.9
    np.testing.assert_allclose(hyp["fitness"], g["seed_fitness"], atol=2.5 / n)
    ok = np.abs(hyp["T"] - g["seed_trans"]).reshape(len(seeds), -1).max(1) < 1e-3
    assert ok.mean() > 0.9
    tight = hyp["kgap"] >= 1e-5           # where the neighbour list is decided, float64 and the reference agree to fp32 round-off
    assert np.abs(hyp["T"] - g["seed_trans"])[tight].max() < 1e-5
    ref = rs.refine(g["init_trans"], g["src"], g["tgt"], CFG["inlier_threshold"])
    np.testing.assert_allclose(ref["T"], g["final_trans"], atol=2e-5)


@pytest.mark.parametrize("n", [640, 1152])
def test_agrees_with_the_fp32_oracle_above_512_rows(n):
    c = cases.make_case(n)
    src, tgt, feat, conf = (torch.from_numpy(c[k]) for k in ("src", "tgt", "feat", "conf"))
    S = cases.seed_count(n, CFG["ratio"])
    sd = rs.seeds(c["src"], c["conf"], CFG["nms_radius"], S)
    assert sd["gap"] >= cases.GAP
    assert 0 < sd["local_max"].sum() < n                           # the NMS decides something
    o_seeds = orc.pick_seeds(orc.pairwise_norm(src), conf, CFG["nms_radius"], S).numpy()
    assert np.array_equal(sd["seeds"], o_seeds)
    hyp = rs.hypotheses(sd["seeds"], c["feat"], c["src"], c["tgt"], 1.0, CFG["sigma_d"], CFG["k"], CFG["num_iterations"], CFG["inlier_threshold"])
    o = orc.seed_hypotheses(torch.from_numpy(sd["seeds"]), torch.nn.functional.normalize(feat, p=2, dim=-1), src, tgt, 1.0, CFG["sigma_d"],
                            CFG["k"], CFG["num_iterations"], CFG["inlier_threshold"])
    tight = hyp["kgap"] >= 1e-5
    assert (~tight).mean() <= 0.03
    assert all(abs(m) >= 1e-6 for m in hyp["margins"])
    for s in np.nonzero(tight)[0]:
        assert set(hyp["knn"][s].tolist()) == set(o["knn_idx"][s].tolist())
    assert np.abs(hyp["T"] - o["seed_trans"].numpy())[tight].max() < 1e-5
    assert hyp["near"].max() <= 2
    assert (np.abs(hyp["fitness"] - o["fitness"].numpy()) <= hyp["near"] / n + 1e-6).all()
    T0 = cases.perturbed(c["T_gt"], n)
    ref = rs.refine(T0, c["src"], c["tgt"], CFG["inlier_threshold"])
    assert ref["iterations"] >= 1 and ref["near"] <= 2
    np.testing.assert_allclose(ref["T"], orc.post_refinement(torch.from_numpy(T0), src, tgt, CFG["inlier_threshold"]).numpy(), atol=2e-5)
    np.testing.assert_allclose(ref["T"], c["T_gt"], atol=5e-3)    # and the refinement finds the pose the pair was made with


def test_duplicates_and_ties_are_in_the_inputs():
    c = cases.make_case(640)
    for a, b in c["dup"]:
        assert all(np.array_equal(c[k][a], c[k][b]) for k in ("src", "tgt", "feat", "conf"))
    vals, counts = np.unique(c["conf"], return_counts=True)
    assert counts.max() > 1 and (c["conf"] == 0).any() and (c["conf"] < 0).any()
