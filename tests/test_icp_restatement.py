"""CPU tests of the ICP definition: its numpy restatement (tests/icp_restatement.py) against the reference's recorded results
(tests/golden/icp_*.npz, written by `tools/gen_goldens.py icp` from the reference's own `icp`), and the cases the reference cannot
run (unequal sizes, max_dist, too few rows, NaN beyond the counts)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restatement as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    g = np.load(os.path.join(GOLDEN, f"icp_{name}.npz"))
    init = g["init_pose"] if int(g["has_init"]) else None
    return g, init


@pytest.mark.parametrize("tag", ["", "_coarse", "_fine"], ids=["own_tolerance", "tolerance_1e-3", "tolerance_1e-6"])
@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_restatement_equals_the_reference_on_the_goldens(name, tag):
    g, init = load(name)
    A, B, init2, tol = R.golden_case(name)
    assert np.array_equal(A, g["A"]) and np.array_equal(B, g["B"]) and float(g["tolerance"]) == tol       # the fixture is the seeded case
    assert (init is None) == (init2 is None) and (init is None or np.array_equal(init, init2))
    tol = float(g["tolerance" + tag])
    assert tol == {"": R.GOLDEN_CASES[name]["tolerance"], "_coarse": R.TOLERANCE, "_fine": R.FINE_TOLERANCE}[tag]
    r = R.icp(g["A"], g["B"], init, int(g["max_iterations"]), tol)
    gap = float(np.abs(r["T"][:3] - g["T" + tag]).max())
    print(f"icp_{name} at tolerance {tol:g}: iters {r['iters']}, |T - T_ref| = {gap:.2e}")
    assert r["iters"] == int(g["iters" + tag])
    assert gap <= 1e-12
    # the margins the generator asserted, so that indices and iteration count are determined beyond rounding
    assert r["nn_gap"] >= 1e-9 and r["conv_gap"] >= 1e-9 and r["sv_ratio"] >= 1e-2
    assert len(r["idx_seq"]) == r["iters"] and np.array_equal(r["idx_seq"][-1], r["idx"])


def test_golden_cases_cover_what_they_claim():
    it = {n: int(load(n)[0]["iters"]) for n in R.GOLDEN_CASES}
    assert it["all20"] == R.MAX_ITER and it["identity"] < R.MAX_ITER and all(1 <= v <= R.MAX_ITER for v in it.values())
    assert float(load("all20")[0]["tolerance"]) == R.FINE_TOLERANCE == 1e-6
    A, B, init, tol = R.golden_case("mirrored")
    assert R.icp(A, B, init, R.MAX_ITER, tol)["det_negative"] >= 1                      # the det(V U^T) = -1 branch of a dT
    assert R.golden_case("near")[2] is not None and all(R.golden_case(n)[2] is None for n in R.GOLDEN_CASES if n != "near")
    g = load("permuted")[0]
    assert not np.array_equal(R.icp(g["A"], g["B"], None, 1, 1e-3)["idx"], np.arange(g["A"].shape[0]))       # rows really are shuffled
    sizes = sorted(R.GOLDEN_CASES[n]["n"] for n in R.GOLDEN_CASES)
    assert sizes[0] == 64 and sizes[-1] == 700


def test_best_fit_is_the_reference_formula():
    """R = V diag(1, 1, det(V U^T)) U^T equals the reference's `Vt[2] *= -1` branch; t = cB - R cA."""
    rng = np.random.default_rng(3)
    A = R.object_cloud(rng, 50)
    Rt = R._rot([0.2, -0.5, 1.0], 0.7)
    B = A @ Rt.T + np.array([0.01, 0.02, -0.03])
    T = R.best_fit_transform_icp(A, B)
    assert np.abs(T[:3, :3] - Rt).max() < 1e-12 and np.abs(T[:3, 3] - np.array([0.01, 0.02, -0.03])).max() < 1e-12
    Bm = B * np.array([1.0, 1.0, -1.0])                                  # a mirror image: the best ORTHOGONAL fit is a reflection
    Tm, S, d = R.best_fit_transform_icp(A, Bm, want_svd=True)
    assert d < 0 and abs(np.linalg.det(Tm[:3, :3]) - 1.0) < 1e-12
    H = (A - A.mean(0)).T @ (Bm - Bm.mean(0))
    U, _, Vt = np.linalg.svd(H)
    Vt[2, :] *= -1
    assert np.abs(Tm[:3, :3] - Vt.T @ U.T).max() < 1e-12


def test_unequal_sizes_and_max_dist():
    rng = np.random.default_rng(4)
    A = R.object_cloud(rng, 90)
    Rt = R._rot([1.0, 0.3, 0.2], 0.05)
    c = A.mean(0)
    B = np.concatenate([(A - c) @ Rt.T + c + 0.002, R.object_cloud(rng, 37)])          # 127 target rows for 90 source rows
    r = R.icp(A, B, None, 20, 1e-6)
    assert r["iters"] >= 2 and r["n_kept"] == 90 and r["idx"].max() < 127
    assert np.abs(r["T"][:3, :3] - Rt).max() < 1e-3
    far = np.concatenate([A, A[:5] + 0.5])                                # five source rows half a metre away
    r_all = R.icp(far, B, None, 20, 1e-6)
    r_cut = R.icp(far, B, None, 20, 1e-6, max_dist=0.05)
    assert r_all["n_kept"] == 95 and r_cut["n_kept"] == 90                # max_dist drops exactly the far rows
    assert np.abs(r_cut["T"] - r["T"]).max() < 1e-12 and np.abs(r_all["T"] - r["T"]).max() > 1e-3


def test_too_few_rows_and_empty_clouds_return_the_start():
    rng = np.random.default_rng(5)
    A, B = R.object_cloud(rng, 40), R.object_cloud(rng, 40)
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, 0.0, -0.01]
    T0 = T0.astype(np.float32).astype(np.float64)
    for n_s in (0, 1, 2):
        r = R.icp(A[:n_s], B, T0)
        assert r["iters"] == 0 and np.array_equal(r["T"], T0) and r["idx"].shape == (n_s,) and r["n_kept"] == 0
    r = R.icp(A, B[:0], T0)
    assert r["iters"] == 0 and np.array_equal(r["T"], T0) and (r["idx"] == -1).all()
    r = R.icp(A, B, T0, status_in=2)
    assert r["iters"] == 0 and np.array_equal(r["T"], T0)
    # m < 3: two source rows near the target, the rest beyond max_dist -> the first iteration ends the pair, T_0 stays
    src = np.concatenate([B[:2] + 1e-4, B[2:10] + 1.0])
    r = R.icp(src, B, None, max_dist=0.01)
    assert r["iters"] == 0 and r["n_kept"] == 2 and np.array_equal(r["T"], np.eye(4)) and len(r["idx_seq"]) == 1


def test_nan_rows_beyond_the_counts_are_never_read():
    """What lies beyond a count does not matter, and a count above its capacity is the capacity.  A NaN row INSIDE the counts never
    wins a neighbour search, and a NaN source row has no neighbour and is dropped."""
    rng = np.random.default_rng(6)
    A, B = R.object_cloud(rng, 30), R.object_cloud(rng, 45)
    base = R.icp(A, B, None, 5, 1e-9)
    pad = lambda x, k: np.concatenate([x, np.full((k, 3), np.nan)])
    r = R.icp(pad(A, 7), pad(B, 4), None, 5, 1e-9, n_s=30, n_d=45)
    assert np.array_equal(r["T"], base["T"]) and np.array_equal(r["idx"], base["idx"]) and r["iters"] == base["iters"]
    r = R.icp(A, B, None, 5, 1e-9, n_s=99, n_d=1000)
    assert np.array_equal(r["T"], base["T"])
    Bn = np.concatenate([B, np.full((3, 3), np.nan)])
    withnan = R.icp(A, Bn, None, 5, 1e-9)
    assert np.array_equal(withnan["T"], base["T"]) and np.array_equal(withnan["idx"], base["idx"])       # NaN target rows never win
    An = np.concatenate([A, np.full((2, 3), np.nan)])
    r = R.icp(An, B, None, 5, 1e-9)
    assert r["n_kept"] == 30 and (r["idx"][30:] == -1).all() and np.array_equal(r["T"], base["T"])
