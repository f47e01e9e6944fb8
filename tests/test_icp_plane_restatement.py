"""CPU tests of point-to-plane ICP on the depth map (g3): the numpy restatement of its definition (tests/icp_plane_restatement.py) on
the fixtures the GPU tests use - that every branch of the definition is taken, that every discrete decision stands by a margin
rounding cannot cross, that the method converges - and the C ABI of csrc/icp_plane.hip: symbols, caps, the workspace formula and every
argument check, which runs before any HIP call (0x1000 stands for a non-NULL pointer that is never dereferenced).  No GPU is touched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_plane_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9
STARTED = (1, 2, 3, 4)                     # pair 5 holds five rows and never starts
MAX_ROWS, MAX_ITER, STATE_BYTES, REC = 8192, 1000, 136, 29


@pytest.fixture(scope="module")
def runs():
    """The restatement of every fixture at the two tolerances the GPU test uses, computed once."""
    out = {}
    for k in R.FIXTURES:
        f = R.fixture(k)
        out[k] = {tol: R.icp_plane(f["src"], f["depth"], f["mask"], f["cam9"], f["T0"], 20, tol) for tol in (1e-5, 0.0)}
    return out


def test_fixture_shapes_are_the_ones_the_kernel_branches_on():
    assert {k: (f[0], f[1], f[2]) for k, f in R.FIXTURES.items()} == {1: (48, 48, 300), 2: (40, 56, 257), 3: (56, 40, 256), 4: (48, 48, 255),
                                                                      5: (48, 48, 5)}
    for k in R.FIXTURES:
        f = R.fixture(k)
        H, W, n, _ = R.FIXTURES[k]
        assert f["src"].shape == (n, 3) and f["depth"].shape == (H, W) == f["mask"].shape and f["depth"].dtype == np.float32
        assert f["T0"].dtype == np.float32 and ((f["mask"] == 0) & (f["depth"] > 0)).any() and ((f["mask"] == 1) & (f["depth"] == 0)).any()


@pytest.mark.parametrize("k", STARTED)
def test_every_drop_class_occurs(k, runs):
    f = R.fixture(k)
    r = runs[k][1e-5]
    print(k, r["drops"], r["n_kept_seq"])
    for name in ("behind", "outside", "mask", "normal", "dist"):
        assert r["drops"][name] >= 1, name
    assert r["drops"]["behind"] == r["iters"]                     # the hand-placed row, at every iteration
    # no normal AT THE STEP: a row left at the normal test on a pixel one of whose x-neighbours lies across x = 0.7 W
    a = R.associate(r["T"], f["src"], f["depth"], f["mask"], f["cam9"], r["origin"])
    at_step = (a["stage"] == 4) & (a["px"] - 1 <= 0.7 * f["W"]) & (a["px"] + 1 > 0.7 * f["W"])
    assert at_step.any()
    assert set(np.unique(a["stage"])) >= {0, 1, 2, 4, 6}


def test_the_no_depth_class_occurs_on_some_fixture(runs):
    assert sum(runs[k][1e-5]["drops"]["depth"] for k in STARTED) >= 1


@pytest.mark.parametrize("k", STARTED)
@pytest.mark.parametrize("tol", [1e-5, 0.0])
def test_margins_of_every_discrete_decision(k, tol, runs):
    """Each >= 1e-9 in its own unit: pixels, metres, millimetres, metres, a ratio, rows.  At tolerance 0 the convergence test
    |prev - mean| < 0 is false for every float, so it has no margin to assert."""
    r = runs[k][tol]
    print(k, tol, {g: r[g] for g in ("frac_gap", "dist_gap", "jump_gap", "conv_gap", "pivot_gap", "rows_gap")}, "cond %.2e" % r["cond"])
    assert r["frac_gap"] >= MARGIN and r["dist_gap"] >= MARGIN and r["jump_gap"] >= MARGIN
    assert r["pivot_gap"] >= MARGIN and r["rows_gap"] >= MARGIN and min(r["n_kept_seq"]) >= 6
    if tol > 0:
        assert r["conv_gap"] >= MARGIN
    else:
        assert r["iters"] == 20
    assert r["cond"] <= 1e4


@pytest.mark.parametrize("k", STARTED)
def test_converges_to_a_tenth_of_the_start_error_or_better(k, runs):
    f, r = R.fixture(k), runs[k][1e-5]
    a0, t0 = R.pose_error(f["T0"], f["T_gt"], f["centre"])
    a1, t1 = R.pose_error(r["T"], f["T_gt"], f["centre"])
    print(f"pair {k}: {a0:.3f} deg, {t0 * 1e3:.2f} mm -> {a1:.4f} deg, {t1 * 1e3:.4f} mm in {r['iters']} iterations")
    assert 3.9 <= a0 <= 4.1 and t0 >= 5e-3
    assert a1 <= a0 / 10 and t1 <= t0 / 10 and 2 <= r["iters"] < 20


def test_pairs_that_never_start_return_t0():
    f = R.fixture(5)
    r = R.icp_plane(f["src"], f["depth"], f["mask"], f["cam9"], f["T0"])
    assert r["iters"] == 0 and np.array_equal(r["T"], f["T0"][:3].astype(np.float64)) and (r["idx"] == -1).all() and r["n_kept"] == 0
    f = R.fixture(2)
    r = R.icp_plane(f["src"], f["depth"], f["mask"], f["cam9"], f["T0"], status_in=2)
    assert r["iters"] == 0 and np.array_equal(r["T"], f["T0"][:3].astype(np.float64))
    r = R.icp_plane(f["src"], f["depth"], np.zeros_like(f["mask"]), f["cam9"], f["T0"])           # an empty mask: executed once, m = 0
    assert r["iters"] == 0 and r["n_kept_seq"] == [0] and (r["idx"] == -1).all()
    r = R.icp_plane(f["src"], f["depth"], f["mask"], f["cam9"], f["T0"], max_iter=3)
    assert r["iters"] == 3 and len(r["n_kept_seq"]) == 3


def test_one_gauss_newton_step_is_the_least_squares_solution():
    for k in STARTED:
        f = R.fixture(k)
        T = f["T0"][:3].astype(np.float64)
        a = R.associate(T, f["src"], f["depth"], f["mask"], f["cam9"], R.origin_of(T, f["src"]))
        A, g, _ = R.normal_equations(a["J"], a["r"])
        x, ratio = R.cholesky_solve(A, g)
        ls = np.linalg.lstsq(a["J"], -a["r"], rcond=None)[0]
        print(k, "rows", a["J"].shape[0], "|x - lstsq|", np.abs(x - ls).max(), "pivot ratio", ratio)
        assert np.abs(x - ls).max() <= 1e-10
        assert np.abs(A - a["J"].T @ a["J"]).max() <= 1e-12 * np.abs(A).max()


def test_a_failed_pivot_ends_the_solve():
    J = np.random.default_rng(3).normal(size=(40, 6))
    J[:, 5] = J[:, 4]                                              # two equal columns: A is singular
    A, g, _ = R.normal_equations(J, np.ones(40))
    x, ratio = R.cholesky_solve(A, g)
    assert x is None and ratio <= R.PIVOT_FLOOR


def test_cayley_is_a_rotation_and_agrees_with_the_rotation_vector_to_second_order(runs):
    ws = [np.array(w) for w in ([0.0, 0.0, 0.0], [0.07, -0.02, 0.03], [1.5, -2.0, 0.7], [1e-9, 0.0, 0.0])]
    ws += [x[:3] for k in STARTED for x in runs[k][1e-5]["x_seq"]]
    for w in ws:
        Rm = R.cayley(w)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(Rm) - 1.0) <= 1e-14
    w = np.array([0.01, -0.02, 0.015])
    assert np.abs(R.cayley(w) - R.rot(w, np.linalg.norm(w))).max() <= np.linalg.norm(w) ** 3
    assert np.array_equal(R.cayley(np.zeros(3)), np.eye(3))


def test_the_sign_of_the_normal_does_not_matter():
    """J J^T, J r and |r| are even in n: a transposed map (x and y swapped: the cross product changes sign) gives the same pose."""
    f = R.fixture(2)
    r = R.icp_plane(f["src"], f["depth"], f["mask"], f["cam9"], f["T0"])
    K = f["cam9"]
    swap = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])              # (x, y, z) -> (y, x, z): a reflection
    camT = np.array([K[4], 0.0, K[5], 0.0, K[0], K[2], 0.0, 0.0, 1.0])
    S4 = np.eye(4)
    S4[:3, :3] = swap
    T0 = S4 @ f["T0"].astype(np.float64)
    # T_0 is handed over in float64 here (the entry would round it to fp32; its values are a permutation of fp32 values: exact)
    rt = R.icp_plane(f["src"], np.ascontiguousarray(f["depth"].T), np.ascontiguousarray(f["mask"].T), camT, T0)
    assert rt["iters"] == r["iters"] and rt["n_kept_seq"] == r["n_kept_seq"]
    assert np.abs(swap @ rt["T"] - r["T"]).max() <= 1e-9


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def P(v=0x1000):
    return ctypes.c_void_p(v)


def _lib():
    from oryon_amd import _lib
    return _lib.lib()


def _ok():
    return dict(src=P(), n_src=P(), cap_src=64, depth=P(), mask=P(), H=48, W=40, cam9=P(), B=2, T_init=P(), max_iter=20, tolerance=1e-5,
                max_dist=0.02, normal_jump=0.02, status_in=None, workspace=P(), workspace_bytes=1 << 20, T=P(), T64=None, iters=P(),
                mean_err=P(), n_kept=P(), idx=None, status_out=P(), stream=None)


def _call(**change):
    L = _lib()
    rc = L.oryon_icp_plane_refine(*dict(_ok(), **change).values())
    return rc, L.oryon_last_error().decode()


def test_symbols_and_header_caps():
    from oryon_amd import _lib, geo6d, ops
    for name in ("oryon_icp_plane_workspace_bytes", "oryon_icp_plane_refine"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert callable(ops.icp_plane_refine) and callable(geo6d.icp_point_to_plane)
    header = open(os.path.join(ROOT, "include", "oryon_hip.h")).read()
    for line in (f"#define ORYON_ICP_MAX_ROWS {MAX_ROWS}", f"#define ORYON_ICP_MAX_ITER {MAX_ITER}", f"#define ORYON_ICP_STATE_BYTES {STATE_BYTES}",
                 f"#define ORYON_ICP_PLANE_REC {REC}", "size_t oryon_icp_plane_workspace_bytes(int B, int cap_src);", "int oryon_icp_plane_refine("):
        assert line in header
    assert "icp_plane.hip" in open(os.path.join(ROOT, "oryon_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("key", ["src", "n_src", "depth", "mask", "cam9", "T_init", "workspace", "T", "iters", "mean_err", "n_kept", "status_out"])
def test_null_pointers_are_rejected(key):
    rc, err = _call(**{key: None})
    assert rc == -1 and "oryon_icp_plane_refine: invalid argument" in err and key in err


def test_optional_pointers_may_be_null_and_b_zero_returns_ok():
    rc, err = _call(B=0)                                   # nothing to do: returns before any launch, T64 / idx / status_in NULL
    assert rc == 0, err


@pytest.mark.parametrize("change,names", [
    (dict(max_iter=0), "max_iter"), (dict(max_iter=MAX_ITER + 1), "max_iter"),
    (dict(tolerance=-1e-9), "tolerance"), (dict(tolerance=float("nan")), "tolerance"),
    (dict(max_dist=-1.0), "max_dist"), (dict(max_dist=float("nan")), "max_dist"),
    (dict(normal_jump=-1.0), "normal_jump"), (dict(normal_jump=float("nan")), "normal_jump"),
    (dict(cap_src=MAX_ROWS + 1), "cap_src"), (dict(cap_src=0), "cap_src"),
    (dict(B=-1), "B"), (dict(B=65536), "B"),
    (dict(H=2), "H >= 3"), (dict(W=2), "W >= 3"), (dict(H=1 << 16, W=1 << 15), "H * W"),
    (dict(src=P(0x1004)), "aligned8"), (dict(cam9=P(0x1002)), "aligned8"), (dict(T64=P(0x1004)), "aligned8"), (dict(mean_err=P(0x1001)), "aligned8"),
    (dict(workspace=P(0x1010)), "workspace"),
    (dict(workspace_bytes=16), "workspace_bytes"), (dict(workspace_bytes=0), "workspace_bytes"),
])
def test_bad_values_are_rejected_with_the_checks_name(change, names):
    rc, err = _call(**change)
    assert rc == -1 and "oryon_icp_plane_refine: invalid argument" in err and names in err, err


def test_the_largest_map_below_2_to_the_31_passes_the_shape_check():
    rc, err = _call(H=(1 << 16) - 1, W=1 << 15, B=0)
    assert rc == 0, err


def test_workspace_bytes_follows_the_documented_formula_and_one_byte_short_is_rejected():
    L = _lib()
    a256 = lambda x: (x + 255) // 256 * 256
    for B, cs in ((1, 1), (2, 64), (5, 256), (5, 257), (64, 2048), (3, MAX_ROWS), (65535, 3)):
        assert L.oryon_icp_plane_workspace_bytes(B, cs) == a256(B * STATE_BYTES) + a256(B * ((cs + 255) // 256) * REC * 8), (B, cs)
    for B, cs in ((0, 64), (-1, 64), (65536, 64), (1, 0), (1, MAX_ROWS + 1), (1, -5)):
        assert L.oryon_icp_plane_workspace_bytes(B, cs) == 0, (B, cs)
    need = L.oryon_icp_plane_workspace_bytes(2, 64)
    rc, err = _call(workspace_bytes=need - 1)
    assert rc == -1 and "workspace_bytes" in err


def test_python_wrapper_names_the_failed_check_without_a_gpu():
    from oryon_amd import ops
    src = torch.zeros(1, 8, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"icp_plane_refine: src\.is_cuda"):
        ops.icp_plane_refine(src, torch.tensor([8], dtype=torch.int32), torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int32),
                             torch.zeros(1, 9, dtype=torch.float64), torch.eye(4)[None])


def test_pipeline_refine_flag_and_its_mode_dependent_defaults():
    from oryon_amd import pipeline
    from oryon_amd.pipeline import Pipeline, default_args
    assert pipeline.REFINEMENTS == ("none", "icp", "icp_plane")
    args = default_args()
    args.test.refine = "icp_plane"
    assert Pipeline(args).refine_mode() == "icp_plane"
    assert pipeline.REFINE_DEFAULTS == {"icp": dict(tolerance=1e-3, max_dist=float("inf")),
                                        "icp_plane": dict(tolerance=1e-5, max_dist=0.02, normal_jump=0.02)}
    try:
        pipeline.set_default_refine("icp_plane")
        assert Pipeline(default_args()).refine_mode() == "icp_plane"
    finally:
        pipeline.set_default_refine("none")
    args.test.refine = "icp_planes"
    with pytest.raises(RuntimeError, match="Refinement icp_planes not implemented"):
        Pipeline(args)


def test_run_pose_parses_refine_icp_plane():
    sys.path.insert(0, ROOT)
    import run_pose
    assert run_pose.parse(["--refine", "icp_plane", "--pairs", "4"]) == ("pointdsc", ["--pairs", "4"])
    assert run_pose.take_refine(["--solver", "ransac", "--refine", "icp_plane", "--pairs", "4"]) == ("icp_plane", ["--solver", "ransac", "--pairs", "4"])
    assert run_pose.take_refine(["--refine", "icp"])[0] == "icp" and run_pose.take_refine([])[0] == "none"
    with pytest.raises(SystemExit):
        run_pose.take_refine(["--refine", "plane"])
