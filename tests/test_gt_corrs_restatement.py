"""CPU tests of the ground-truth correspondence routine: the numpy restatement of its definition (tests/gt_corrs_restatement.py)
against the reference's recorded results (tests/golden/gtcorr_*.npz, written by `tools/gen_goldens.py gt_corrs`), the C ABI's argument
checks (no launch is reached), the Python entry points' checks and the driver's defaults."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gt_corrs_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_restatement_equals_the_reference_on_the_goldens(name):
    g = np.load(os.path.join(GOLDEN, f"gtcorr_{name}.npz"))
    seed, n1, n2, threshold, max_corrs, tseed = R.GOLDEN_CASES[name]
    assert (int(g["numpy_seed"]), int(g["n1"]), int(g["n2"]), float(g["threshold"]), int(g["max_corrs"]), int(g["torch_seed"])) == \
        (seed, n1, n2, threshold, max_corrs, tseed)
    f1, f2 = R.golden_clouds(name)
    saved = torch.get_rng_state()
    try:
        torch.manual_seed(tseed)
        i1, i2 = R.pcd_correspondences(f1, f2, threshold, max_corrs)
        state = torch.get_rng_state().numpy()
    finally:
        torch.set_rng_state(saved)
    assert np.array_equal(i1.numpy(), g["idx1"]) and np.array_equal(i2.numpy(), g["idx2"])       # indices, kept set, order, draws
    assert np.array_equal(state, g["rng_state"]), "the generator is not where the reference leaves it"
    assert i1.shape[0] == min(int(g["n_kept"]), max_corrs)


def test_golden_cases_cover_what_they_claim():
    kept = {n: int(np.load(os.path.join(GOLDEN, f"gtcorr_{n}.npz"))["n_kept"]) for n in R.GOLDEN_CASES}
    assert R.GOLDEN_CASES["exact20000"][1] == R.SAMPLE and R.GOLDEN_CASES["small"][1] < R.SAMPLE
    assert kept["overmax"] > R.GOLDEN_CASES["overmax"][4] and kept["nokeep"] == 0 and kept["single"] == 1 and 0 < kept["small"] < 3000


def test_lift_restatement_is_the_reference_expression_in_torch():
    """utils/pcd.py:66-73 as toyl.get_pcd calls it: float32 pixel maps, a float64 depth channel and 0-dim float64 camera entries;
    torch's promotion keeps `xmap - cx` in float32.  The restatement's explicit roundings must give the same bits."""
    H, W = 21, 34
    rng = np.random.default_rng(5)
    depth = rng.integers(0, 1500, (H, W)).astype(np.float32)
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.5704, 242.0489], [0.0, 0.0, 1.0]])
    cam = torch.tensor(K).flatten()
    xs, ys = torch.linspace(0, W - 1, steps=W), torch.linspace(0, H - 1, steps=H)
    xmap, ymap = torch.meshgrid(xs, ys, indexing="xy")
    xmap, ymap = xmap.flatten().to(torch.float32), ymap.flatten().to(torch.float32)
    pt2 = torch.tensor(depth.astype(np.float64)).flatten()
    pt0 = (xmap - cam[2]) * pt2 / cam[0]
    pt1 = (ymap - cam[5]) * pt2 / cam[4]
    want = (torch.stack((pt0, pt1, pt2), dim=1) / 1000.).numpy()
    assert want.dtype == np.float64
    xyz, yx = R.lift(depth, np.arange(H * W), K)
    assert np.array_equal(xyz, want)
    assert np.array_equal(yx[:, 0], np.arange(H * W) // W) and np.array_equal(yx[:, 1], np.arange(H * W) % W)
    all64 = (np.arange(H * W) % W - K[0, 2]) * depth.reshape(-1).astype(np.float64) / K[0, 0] / 1000.0
    assert 0 < np.abs(all64 - xyz[:, 0]).max() < 1e-7              # the all-float64 lift is a different function


def test_nearest_restatement_first_minimiser_and_edges():
    dst = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0]])
    idx, d2 = R.nearest(np.array([[0.9, 0, 0], [0.1, 0, 0], [0.5, 0, 0]]), dst)
    assert idx.tolist() == [1, 0, 0] and d2[2] == 0.25
    idx, d2 = R.nearest(np.zeros((2, 3)), np.zeros((0, 3)))
    assert idx.tolist() == [-1, -1] and np.isinf(d2).all()
    assert R.keep(np.array([0.002 * 0.002, 4.0000001e-6]), 0.002).tolist() == [True, False]          # <=: a row AT the threshold is kept


def test_symbols_are_present():
    from oryon_amd import _lib, ops, pairs
    L = _lib.lib()
    for name in ("oryon_gtc_lift", "oryon_pcd_nearest_f64", "oryon_gt_corrs_workspace_bytes", "oryon_gt_corrs"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    for fn in ("pcd_nearest", "gt_corrs", "gtc_lift"):
        assert callable(getattr(ops, fn))
    for fn in ("pcd_correspondences", "lift_object", "pair_correspondences", "make_fixed_split"):
        assert callable(getattr(pairs, fn))


def test_c_abi_rejects_bad_arguments_before_any_launch():
    from oryon_amd import _lib
    L = _lib.lib()
    P = lambda v=0x10000: ctypes.c_void_p(v)       # never dereferenced: every call below fails an argument check first
    err = lambda: L.oryon_last_error().decode()
    # the nearest stage
    assert L.oryon_pcd_nearest_f64(None, P(), P(), P(), 1, 4, 4, P(), P(), None) == -1 and "oryon_pcd_nearest_f64: invalid argument" in err()
    assert L.oryon_pcd_nearest_f64(P(), P(), P(), P(), 1, 4, 4, P(), None, None) == -1
    assert L.oryon_pcd_nearest_f64(P(0x10004), P(), P(), P(), 1, 4, 4, P(), P(), None) == -1 and "aligned" in err()       # unaligned float64
    assert L.oryon_pcd_nearest_f64(P(), P(), P(), P(), 1, 4, 4, P(), P(0x10004), None) == -1 and "aligned" in err()
    assert L.oryon_pcd_nearest_f64(P(), P(), P(), P(), 1, 0, 4, P(), P(), None) == -1 and "cap_src" in err()
    assert L.oryon_pcd_nearest_f64(P(), P(), P(), P(), -1, 4, 4, P(), P(), None) == -1
    # the lift
    assert L.oryon_gtc_lift(None, 1, 4, 4, P(), P(), 4, P(), None, P(), P(), None) == -1 and "oryon_gtc_lift" in err()
    assert L.oryon_gtc_lift(P(), 1, 4, 4, P(), P(), 4, P(0x10002), None, P(), P(), None) == -1 and "aligned" in err()
    assert L.oryon_gtc_lift(P(), 1, 4, 4, P(), P(), 0, P(), None, P(), P(), None) == -1
    # the whole routine
    ok = dict(depth_a=P(), depth_q=P(), B=1, HA=4, WA=4, HQ=4, WQ=4, pix_a=P(), n_a=P(), cap_a=8, pix_q=P(), n_q=P(), cap_q=8, cam_a=P(),
              cam_q=P(), pose_aq=P(), threshold=0.002, status_in=None, workspace=P(), workspace_bytes=1 << 20, corrs=P(), n_corr=P(),
              idx=None, d2=None, stream=None)
    for key in ("depth_a", "depth_q", "pix_a", "n_a", "pix_q", "n_q", "cam_a", "cam_q", "pose_aq", "workspace", "corrs", "n_corr"):
        assert L.oryon_gt_corrs(*dict(ok, **{key: None}).values()) == -1, key
        assert "oryon_gt_corrs: invalid argument" in err()
    for bad in (dict(threshold=-1e-9), dict(threshold=float("nan")), dict(cap_a=0), dict(cap_q=-3), dict(cam_a=P(0x10004)),
                dict(pose_aq=P(0x10001)), dict(d2=P(0x10004)), dict(workspace=P(0x10010)), dict(HA=0), dict(B=70000),
                dict(workspace_bytes=16)):
        assert L.oryon_gt_corrs(*dict(ok, **bad).values()) == -1, bad
    assert L.oryon_gt_corrs(*dict(ok, threshold=-1.0).values()) == -1 and "threshold" in err()
    need = L.oryon_gt_corrs_workspace_bytes(1, 8, 8)
    assert need > 0 and need % 256 == 0 and L.oryon_gt_corrs_workspace_bytes(2, 8, 8) > need
    assert L.oryon_gt_corrs_workspace_bytes(0, 8, 8) == 0 and L.oryon_gt_corrs_workspace_bytes(1, 0, 8) == 0
    assert L.oryon_gt_corrs_workspace_bytes(1, 20000, 20000) == 20000 * (24 + 24 + 8 + 8 + 8 + 4) + \
        sum(-x % 256 for x in (480000, 480000, 160000, 160000, 160000, 80000))


def test_python_entry_points_reject_a_count_above_the_capacity():
    """Counts given on the host are checked before anything touches the GPU (the kernels clamp a device count to the capacity)."""
    from oryon_amd import ops
    a, q = torch.zeros(1, 4, 3, dtype=torch.float64), torch.zeros(1, 6, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="cap"):
        ops.pcd_nearest(a, q, n_src=[5])
    with pytest.raises(ValueError, match="cap"):
        ops.pcd_nearest(a, q, n_dst=torch.tensor([7]))
    with pytest.raises(ValueError):
        ops.pcd_nearest(a, q, n_src=[-1])
    with pytest.raises(ValueError):
        ops.pcd_nearest(a, torch.zeros(2, 6, 3, dtype=torch.float64))
    d, pix, cam = torch.zeros(1, 4, 4), torch.zeros(1, 8, dtype=torch.int32), torch.eye(3, dtype=torch.float64)[None]
    with pytest.raises(ValueError, match="cap"):
        ops.gt_corrs(d, d, pix, [9], pix, [8], cam, cam, torch.eye(4, dtype=torch.float64)[None], 0.002)
    with pytest.raises(ValueError, match="threshold"):
        ops.gt_corrs(d, d, pix, [8], pix, [8], cam, cam, torch.eye(4, dtype=torch.float64)[None], -0.002)
    with pytest.raises(ValueError, match="cap"):
        ops.gtc_lift(d, pix, [9], cam)


def test_make_split_parse_defaults():
    sys.path.insert(0, ROOT)
    import make_split
    a = make_split.parse([])
    assert (a.kind, a.src_split, a.dest_split, a.pairs, a.seed) == ("toyl", "test", "overfit_self", 5, 1)
    assert (a.threshold, a.max_corrs, a.min_corrs, a.data_root) == (0.002, 10000, 100, None)
    b = make_split.parse(["--kind", "nocs", "--data-root", "d", "--pairs", "2000", "--threshold", "0.01", "--max-corrs", "500", "--min-corrs", "7",
                          "--dest-split", "x", "--seed", "9"])
    assert (b.kind, b.src_split, b.data_root, b.pairs, b.threshold, b.max_corrs, b.min_corrs, b.dest_split, b.seed) == \
        ("nocs", "real_test", "d", 2000, 0.01, 500, 7, "x", 9)
    with pytest.raises(SystemExit):
        make_split.main([])
