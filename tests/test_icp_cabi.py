"""CPU tests of the ICP entries' C ABI (include/oryon_hip.h, g2): every argument check runs before any HIP call and names the failed
check, and the workspace size follows its documented formula.  No GPU is touched: 0x1000 stands for a non-NULL pointer that is never
dereferenced."""
import ctypes

import pytest
import torch

MAX_ROWS, MAX_ITER, STATE_BYTES = 8192, 1000, 136          # ORYON_ICP_MAX_ROWS, ORYON_ICP_MAX_ITER, ORYON_ICP_STATE_BYTES


def P(v=0x1000):
    return ctypes.c_void_p(v)


def _lib():
    from oryon_amd import _lib
    return _lib.lib()


def _ok():
    return dict(src=P(), n_src=P(), cap_src=64, dst=P(), n_dst=P(), cap_dst=64, B=2, T_init=P(), max_iter=20, tolerance=1e-3,
                max_dist=float("inf"), status_in=None, workspace=P(), workspace_bytes=1 << 20, T=P(), T64=None, iters=P(), mean_err=P(),
                n_kept=P(), idx=None, status_out=P(), stream=None)


def _call(**change):
    L = _lib()
    rc = L.oryon_icp_refine(*dict(_ok(), **change).values())
    return rc, L.oryon_last_error().decode()


def test_symbols_and_header_caps():
    import os
    from oryon_amd import _lib, geo6d, ops
    for name in ("oryon_icp_workspace_bytes", "oryon_icp_refine", "oryon_icp_best_fit"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert callable(ops.icp_refine) and callable(ops.icp_best_fit) and callable(geo6d.icp) and callable(geo6d.best_fit_transform_icp)
    assert (ops.ICP_MAX_ROWS, ops.ICP_MAX_ITER) == (MAX_ROWS, MAX_ITER)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "oryon_hip.h")).read()
    for line in (f"#define ORYON_ICP_MAX_ROWS {MAX_ROWS}", f"#define ORYON_ICP_MAX_ITER {MAX_ITER}", f"#define ORYON_ICP_STATE_BYTES {STATE_BYTES}"):
        assert line in header


@pytest.mark.parametrize("key", ["src", "n_src", "dst", "n_dst", "T_init", "workspace", "T", "iters", "mean_err", "n_kept", "status_out"])
def test_null_pointers_are_rejected(key):
    rc, err = _call(**{key: None})
    assert rc == -1 and "oryon_icp_refine: invalid argument" in err and key in err


def test_optional_pointers_may_be_null_and_b_zero_returns_ok():
    rc, err = _call(B=0)                                   # nothing to do: returns before any launch, T64 / idx / status_in NULL
    assert rc == 0, err


@pytest.mark.parametrize("change,names", [
    (dict(max_iter=0), "max_iter"), (dict(max_iter=-3), "max_iter"), (dict(max_iter=MAX_ITER + 1), "max_iter"),
    (dict(tolerance=-1e-9), "tolerance"), (dict(tolerance=float("nan")), "tolerance"),
    (dict(max_dist=-1.0), "max_dist"), (dict(max_dist=float("nan")), "max_dist"),
    (dict(cap_src=MAX_ROWS + 1), "cap_src"), (dict(cap_dst=MAX_ROWS + 1), "cap_dst"), (dict(cap_src=0), "cap_src"), (dict(cap_dst=-1), "cap_dst"),
    (dict(B=-1), "B"), (dict(B=70000), "B"),
    (dict(src=P(0x1004)), "aligned8"), (dict(dst=P(0x1002)), "aligned8"), (dict(T64=P(0x1004)), "aligned8"), (dict(mean_err=P(0x1001)), "aligned8"),
    (dict(workspace=P(0x1010)), "workspace"),
    (dict(workspace_bytes=16), "workspace_bytes"), (dict(workspace_bytes=0), "workspace_bytes"),
])
def test_bad_values_are_rejected_with_the_checks_name(change, names):
    rc, err = _call(**change)
    assert rc == -1 and "oryon_icp_refine: invalid argument" in err and names in err, err


def test_a_workspace_one_byte_short_is_rejected_and_the_exact_size_passes_the_check():
    L = _lib()
    need = L.oryon_icp_workspace_bytes(2, 64, 64)
    rc, err = _call(workspace_bytes=need - 1)
    assert rc == -1 and "workspace_bytes" in err


def test_workspace_bytes_follows_the_documented_formula():
    L = _lib()
    a256 = lambda x: (x + 255) // 256 * 256
    for B, cs, cd in ((1, 1, 1), (2, 64, 64), (5, 256, 300), (5, 257, 1), (64, 2048, 2048), (3, MAX_ROWS, MAX_ROWS), (65535, 3, 3)):
        want = a256(B * STATE_BYTES) + a256(B * ((cs + 255) // 256) * 17 * 8)
        assert L.oryon_icp_workspace_bytes(B, cs, cd) == want, (B, cs, cd)
    assert L.oryon_icp_workspace_bytes(64, 2048, 2048) == L.oryon_icp_workspace_bytes(64, 2048, 7)       # the target's size does not enter
    for B, cs, cd in ((0, 64, 64), (-1, 64, 64), (65536, 64, 64), (1, 0, 64), (1, 64, 0), (1, MAX_ROWS + 1, 64), (1, 64, MAX_ROWS + 1), (1, -5, 64)):
        assert L.oryon_icp_workspace_bytes(B, cs, cd) == 0, (B, cs, cd)


def test_best_fit_rejections():
    L = _lib()
    err = lambda: L.oryon_last_error().decode()
    ok = dict(A=P(), Bp=P(), n=P(), cap=16, B=1, workspace=P(), workspace_bytes=1 << 16, T=P(), T64=None, fitted=P(), mean_err=P(), stream=None)
    for key in ("A", "Bp", "n", "workspace", "T", "fitted", "mean_err"):
        assert L.oryon_icp_best_fit(*dict(ok, **{key: None}).values()) == -1 and "oryon_icp_best_fit: invalid argument" in err(), key
    for bad in (dict(cap=0), dict(cap=MAX_ROWS + 1), dict(B=-1), dict(A=P(0x1004)), dict(workspace=P(0x1008)), dict(workspace_bytes=8)):
        assert L.oryon_icp_best_fit(*dict(ok, **bad).values()) == -1, bad
    assert L.oryon_icp_best_fit(*dict(ok, B=0).values()) == 0


def test_python_wrapper_names_the_failed_check_without_a_gpu():
    """ops.icp_refine converts nothing: a tensor that is not a contiguous device tensor of the stated dtype is rejected by name."""
    from oryon_amd import ops
    src = torch.zeros(1, 8, 3, dtype=torch.float64)
    n = torch.tensor([8], dtype=torch.int32)
    with pytest.raises(ValueError, match=r"icp_refine: src\.is_cuda"):
        ops.icp_refine(src, src, n, n, torch.eye(4)[None])


def test_pipeline_refine_flag_is_checked_like_the_solver():
    from oryon_amd.pipeline import Pipeline, default_args
    args = default_args()
    assert not hasattr(args.test, "refine") and Pipeline(args).refine_mode() == "none"
    args.test.refine = "none"
    assert Pipeline(args).refine_mode() == "none"
    args.test.refine = "icp"
    assert Pipeline(args).refine_mode() == "icp"
    args.test.refine = "teaser"
    with pytest.raises(RuntimeError, match="Refinement teaser not implemented"):
        Pipeline(args)


def test_run_pose_parses_refine():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_pose
    assert run_pose.parse(["--refine", "icp", "--pairs", "4"]) == ("pointdsc", ["--pairs", "4"])          # run_test.py never sees the flag
    assert run_pose.parse(["--solver", "ransac", "--refine", "none"]) == ("ransac", [])
    assert run_pose.take_refine(["--refine", "icp", "--pairs", "4"]) == ("icp", ["--pairs", "4"])
    assert run_pose.take_refine(["--pairs", "4"]) == ("none", ["--pairs", "4"])
    with pytest.raises(SystemExit):
        run_pose.parse(["--refine", "teaser"])
    with pytest.raises(SystemExit):
        run_pose.take_refine(["--refine", "teaser"])


def test_the_process_wide_default_refinement_reaches_pipelines_that_name_none():
    from oryon_amd import pipeline
    from oryon_amd.pipeline import Pipeline, default_args
    assert pipeline.default_refine() == "none"
    try:
        pipeline.set_default_refine("icp")
        assert Pipeline(default_args()).refine_mode() == "icp"
        args = default_args()
        args.test.refine = "none"                       # what the args say wins
        assert Pipeline(args).refine_mode() == "none"
        with pytest.raises(ValueError, match="Refinement teaser not implemented"):
            pipeline.set_default_refine("teaser")
    finally:
        pipeline.set_default_refine("none")
    assert Pipeline(default_args()).refine_mode() == "none"
