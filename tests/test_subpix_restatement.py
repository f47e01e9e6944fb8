"""CPU tests of the sub-pixel refinement (csrc/match_subpix.hip, test.subpixel): the numpy statement (tests/subpix_restatement.py) on
exact quadratics and on the shifted-field experiment, the lift's statement against the integer lift's arithmetic, the two symbols,
every argument check of the two entry points by name, and the flags of the façade, the engine and the drivers.  The device side is
tests/test_gpu_subpix.py."""
import dataclasses
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plumbing_restatement as pr  # noqa: E402
import subpix_restatement as sr  # noqa: E402

NAMES = ("oryon_subpix_refine", "oryon_lift_pairs_subpix")
SHIFT = (0.3, -0.2)


# ------------------------------------------------------------------------------------------------ the fit on exact quadratics
def _quadratic(y0, x0, hyy, hxx, hxy, f0=0.2):
    """f(i, j) = f0 + 0.5 (hyy (i - y0)^2 + 2 hxy (i - y0)(j - x0) + hxx (j - x0)^2) on the 3 x 3 stencil."""
    i, j = np.meshgrid(np.array([-1.0, 0.0, 1.0]), np.array([-1.0, 0.0, 1.0]), indexing="ij")
    return f0 + 0.5 * (hyy * (i - y0) ** 2 + 2.0 * hxy * (i - y0) * (j - x0) + hxx * (j - x0) ** 2)


@pytest.mark.parametrize("y0,x0,hyy,hxx,hxy", [(0.0, 0.0, 0.1, 0.1, 0.0), (0.3, -0.2, 0.05, 0.02, 0.01), (-0.45, 0.45, 0.3, 0.1, -0.12),
                                               (0.49, 0.01, 0.002, 0.004, 0.0005), (-0.1, -0.3, 1.0, 1.0, 0.9)])
def test_fit_returns_the_minimum_of_an_exact_quadratic(y0, x0, hyy, hxx, hxy):
    flag, (dy, dx), (g_curv, g_far) = sr.facet_fit(_quadratic(y0, x0, hyy, hxx, hxy), 1e-4)
    assert flag == 0 and abs(dy - y0) <= 1e-12 and abs(dx - x0) <= 1e-12
    lmin = (hxx + hyy) / 2 - np.sqrt((hxx - hyy) ** 2 / 4 + hxy ** 2)
    assert abs(g_curv - (lmin - 1e-4)) <= 1e-12 and abs(g_far - (1 - max(abs(y0), abs(x0)))) <= 1e-12


def test_fit_flags_and_the_clamp():
    assert sr.facet_fit(_quadratic(0.1, 0.1, -0.1, -0.1, 0.0), 1e-4)[0] == 2                  # a maximum
    assert sr.facet_fit(_quadratic(0.1, 0.1, 0.1, -0.1, 0.0), 1e-4)[0] == 2                   # a saddle
    assert sr.facet_fit(np.full((3, 3), 0.25), 1e-4)[0] == 2                                  # a constant patch
    assert sr.facet_fit(np.full((3, 3), 0.25), 0.0)[0] == 3                                   # ... with no curvature floor: 0 / 0 is outside
    assert sr.facet_fit(_quadratic(0.0, 0.0, 5e-5, 5e-5, 0.0), 1e-4)[0] == 2                  # a minimum, but flatter than the floor
    assert sr.facet_fit(_quadratic(1.5, 0.0, 0.1, 0.1, 0.0), 1e-4)[0:2] == (3, (0.0, 0.0))    # a minimum more than one pixel away
    assert sr.facet_fit(_quadratic(0.0, -1.01, 0.1, 0.1, 0.0), 1e-4)[0] == 3
    flag, (dy, dx), _ = sr.facet_fit(_quadratic(0.9, -0.7, 0.1, 0.1, 0.0), 1e-4)              # inside one pixel: accepted, clamped
    assert flag == 0 and (dy, dx) == (0.5, -0.5)
    for bad in (2, 3):
        assert sr.facet_fit(_quadratic(1.5, 0.0, 0.1 if bad == 3 else -0.1, 0.1, 0.0), 1e-4)[1] == (0.0, 0.0)


def test_refine_border_rows_and_the_eps_clamp():
    rng = np.random.default_rng(3)
    fa, fq = rng.normal(size=(8, 6, 7)).astype(np.float32), rng.normal(size=(8, 6, 7)).astype(np.float32)
    fa[:, 2, 2] = 0.0                                                     # an all-zero anchor: every distance 0.5, a constant patch
    fq[:, 3, 3] = 0.0                                                     # an all-zero neighbour
    corrs = [(1, 1, 0, 3), (1, 1, 5, 3), (1, 1, 3, 0), (1, 1, 3, 6), (1, 1, 0, 0), (1, 1, 5, 6), (2, 2, 2, 2), (1, 1, 2, 2), (1, 1, 1, 1),
             (-1, 1, 2, 2), (1, 7, 2, 2)]
    off, fl, gates = sr.refine(fa, fq, corrs, 1e-4)
    assert fl[:6].tolist() == [1] * 6 and fl[9:].tolist() == [1, 1] and fl[6] == 2 and np.isfinite(off).all()
    assert not off[fl != 0].any() and (np.abs(off) <= 0.5).all() and off.dtype == np.float32
    assert np.array_equal(sr.counts(fl, len(fl)), np.bincount(fl, minlength=4)) and sr.counts(fl, 0).tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the shifted-field experiment
def test_refinement_at_least_halves_the_error_on_shifted_fields():
    """C = 32, 24 x 24, shift (0.3, -0.2), interior anchors, exhaustive nearest neighbours.  The condition (shortest period 32 px):
    refined RMS position error <= half the integer one.  Measured: 0.246 / 0.079 / 0.042 at periods 16 / 32 / 64."""
    ratios = {}
    for period in (16.0, 32.0, 64.0):
        fa, fq = sr.shifted_fields(32, 24, 24, period, SHIFT)
        corrs = sr.nearest_rows(fa, fq)
        off, fl, _ = sr.refine(fa, fq, corrs, 1e-4)
        e0, e1 = sr.position_rms(corrs, None, SHIFT), sr.position_rms(corrs, off, SHIFT)
        ratios[period] = e1 / e0
        print(f"period {period:g}: rows {len(corrs)}, flags {np.bincount(fl, minlength=4).tolist()}, integer RMS {e0:.4f} px, "
              f"refined RMS {e1:.4f} px, ratio {e1 / e0:.3f}")
    assert ratios[32.0] <= 0.5


# ------------------------------------------------------------------------------------------------ the lift
def test_lift_statement_is_the_integer_lift_where_nothing_is_interpolated():
    """Zero offsets, scale 1: f_y = f_x = 0, so wherever the bilinear branch is not taken the arithmetic is lift_pairs' (and where it
    is taken with zero fractions, 1 * z00 + 0 * z01 is z00 as well: all rows agree)."""
    rng = np.random.default_rng(5)
    H, W = 12, 15
    da = (600.0 + 300.0 * rng.random((H, W))).astype(np.float32)          # jumps of up to 300 mm: the bilinear branch is mostly refused
    dq = (600.0 + 300.0 * rng.random((H, W))).astype(np.float32)
    dq[4, 4] = 0.0
    cam = np.array([600.0, 0, 7.3, 0, 590.0, 5.9, 0, 0, 1], dtype=np.float32)
    corrs = np.stack([rng.integers(0, H, 60), rng.integers(0, W, 60), rng.integers(0, H, 60), rng.integers(0, W, 60)], axis=1).astype(np.int32)
    corrs[0] = (3, 3, 4, 4)
    corrs[1] = (H - 1, W - 1, H - 1, 0)
    pa, pq, keep, ba, bq = sr.lift_pairs_subpix(corrs, None, (H, W), da, dq, cam, cam, 20.0)
    ra, rq, rkeep = pr.lift_pairs(corrs, (H, W), da, dq, cam, cam)
    assert keep.all() and np.array_equal(keep, rkeep) and (~ba).any() and (~bq).any()
    assert np.array_equal(pa.view(np.uint32), ra.view(np.uint32)) and np.array_equal(pq.view(np.uint32), rq.view(np.uint32))
    z = np.zeros((60, 2), np.float32)
    pa0, pq0, _, _, _ = sr.lift_pairs_subpix(corrs, z, (H, W), da, dq, cam, cam, 20.0)
    assert np.array_equal(pa0.view(np.uint32), pa.view(np.uint32)) and np.array_equal(pq0.view(np.uint32), pq.view(np.uint32))


def test_lift_statement_branches():
    d = np.full((4, 5), 600.0, np.float32)
    d[1, 1:3], d[2, 1:3] = (600.0, 610.0), (620.0, 630.0)
    cam = np.array([600.0, 0, 0, 0, 600.0, 0, 0, 0, 1], dtype=np.float32)
    row = np.array([[1, 1, 1, 1]], np.int32)
    off = np.array([[0.5, 0.25]], np.float32)
    pa, pq, keep, ba, bq = sr.lift_pairs_subpix(row, off, (4, 5), d, d, cam, cam, 30.0)
    assert keep[0] and ba[0] and bq[0] and pq[0, 2] == np.float32(np.float32(0.5 * 602.5 + 0.5 * 622.5) / np.float32(1000))
    assert pa[0, 2] == np.float32(0.6)                                     # the anchor side has no offset: f = 0, z00
    assert pq[0, 0] == np.float32(np.float32(np.float32(np.float32(1.25) * np.float32(612.5)) / np.float32(600)) / np.float32(1000))
    assert not sr.lift_pairs_subpix(row, off, (4, 5), d, d, cam, cam, 29.5)[4][0]      # max - min = 30 > 29.5: the pixel K2 reads
    d2 = d.copy()
    d2[2, 2] = 0.0
    pq2, bq2 = sr.lift_pairs_subpix(row, off, (4, 5), d, d2, cam, cam, 1e9)[1::3]
    assert not bq2[0] and pq2[0, 2] == np.float32(0.6)                     # a hole among the four
    edge = np.array([[0, 0, 3, 4]], np.int32)                              # i0 + 1 = H, j0 + 1 = W
    assert not sr.lift_pairs_subpix(edge, np.array([[0.25, 0.25]], np.float32), (4, 5), d, d, cam, cam, 1e9)[4][0]
    out = np.array([[0, 0, 3, 4], [0, 0, 0, 0], [1, 1, 1, 1]], np.int32)   # pushed out of the image / to a negative coordinate / NaN
    offs = np.array([[0.5, 1.0], [-0.25, 0.0], [np.nan, 0.0]], np.float32)
    assert sr.lift_pairs_subpix(out, offs, (4, 5), d, d, cam, cam, 30.0)[2].tolist() == [False, False, False]


# ------------------------------------------------------------------------------------------------ the device tests' inputs
def test_the_device_cases_meet_their_conditions():
    """tests/test_gpu_subpix.py compares the device with the statement on these inputs; what that comparison rests on - planted rows with
    the flags they were planted for, every gate quantity at least 1e-6 from its threshold, both lift branches taken - holds on the host."""
    import subpix_cases as sc
    for C in sc.FIT_CHANNELS:
        assert sc.fit_conditions(sc.fit_case(C))
    for q, a in ((sc.LIFT_SIZES[0], sc.LIFT_SIZES[1]), (sc.LIFT_SIZES[1], sc.LIFT_SIZES[0])):
        assert sc.lift_conditions(sc.lift_case(q, a))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_declared_bound_and_exported():
    from oryon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "oryon_hip.h")).read()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert "match_subpix.hip" in open(os.path.join(ROOT, "oryon_amd", "csrc", "Makefile")).read()
    assert len(_lib._PROTOS["oryon_subpix_refine"][1]) == 16 and len(_lib._PROTOS["oryon_lift_pairs_subpix"][1]) == 21
    assert len(_lib._PROTOS["oryon_lift_pairs_subpix"][1]) == len(_lib._PROTOS["oryon_lift_pairs"][1]) + 2


def _fit_args(**change):
    """A complete, acceptable argument list (fake non-null pointers: every check comes before any launch or dereference)."""
    a = dict(feat_a=0x1000, feat_q=0x1000, B=1, C=32, FH=24, FW=24, layout=0, corrs=0x1000, n_corr=None, status=None, n_cap=128,
             curv_min=1e-4, offsets=0x1000, flags=0x1000, counts=0x1000, stream=None)
    a.update(change)
    return list(a.values())


def _lift_args(**change):
    a = dict(corrs=0x1000, offsets=None, n_corr=None, B=1, n_cap=128, FH=24, FW=24, depth_a=0x1000, HA=48, WA=64, depth_q=0x1000, HQ=48,
             WQ=64, cam_a=0x1000, cam_q=0x1000, status=None, depth_jump_mm=20.0, pcd_a=0x1000, pcd_q=0x1000, n_out=0x1000, stream=None)
    a.update(change)
    return list(a.values())


@pytest.mark.parametrize("change,names", [
    (dict(feat_a=None), "feat_a"), (dict(feat_q=None), "feat_q"), (dict(corrs=None), "corrs"), (dict(offsets=None), "offsets"),
    (dict(flags=None), "flags"), (dict(counts=None), "counts"), (dict(C=513), "C <= 512"), (dict(C=0), "C >= 1"),
    (dict(layout=2), "layout == ORYON_LAYOUT_NCHW"), (dict(layout=-1), "layout == ORYON_LAYOUT_NCHW"),
    (dict(curv_min=-1e-6), "curv_min >= 0"), (dict(curv_min=float("nan")), "curv_min"), (dict(n_cap=0), "n_cap >= 1"),
    (dict(FH=0), "FH >= 1"), (dict(B=-1), "B >= 0"), (dict(B=70000), "B <= 65535")])
def test_every_rejection_of_the_fit_names_its_check(change, names):
    from oryon_amd import _lib
    L = _lib.lib()
    assert L.oryon_subpix_refine(*_fit_args(**change)) == -1
    err = L.oryon_last_error().decode()
    assert "oryon_subpix_refine: invalid argument" in err and names in err, err


@pytest.mark.parametrize("change,names", [
    (dict(corrs=None), "corrs"), (dict(depth_a=None), "depth_a"), (dict(depth_q=None), "depth_q"), (dict(cam_a=None), "cam_a"),
    (dict(cam_q=None), "cam_q"), (dict(pcd_a=None), "pcd_a"), (dict(pcd_q=None), "pcd_q"), (dict(n_out=None), "n_out"),
    (dict(depth_jump_mm=-1.0), "depth_jump_mm >= 0"), (dict(depth_jump_mm=float("nan")), "depth_jump_mm"), (dict(n_cap=0), "n_cap > 0"),
    (dict(HQ=0), "HQ > 0"), (dict(B=-1), "B >= 0")])
def test_every_rejection_of_the_lift_names_its_check(change, names):
    from oryon_amd import _lib
    L = _lib.lib()
    assert L.oryon_lift_pairs_subpix(*_lift_args(**change)) == -1
    err = L.oryon_last_error().decode()
    assert "oryon_lift_pairs_subpix: invalid argument" in err and names in err, err


def test_the_no_op_and_the_optional_arguments():
    from oryon_amd import _lib
    L = _lib.lib()
    # B == 0: nothing to do, nothing launched; NULL n_corr / status / offsets are allowed, an infinite jump as well
    assert L.oryon_subpix_refine(*_fit_args(B=0)) == 0 and L.oryon_subpix_refine(*_fit_args(B=0, curv_min=0.0, C=512, layout=1)) == 0
    assert L.oryon_lift_pairs_subpix(*_lift_args(B=0)) == 0 and L.oryon_lift_pairs_subpix(*_lift_args(B=0, depth_jump_mm=float("inf"))) == 0


# ------------------------------------------------------------------------------------------------ the flags
def test_flags_of_the_facade_the_engine_and_the_drivers():
    from oryon_amd import engine, ops, pcd
    from oryon_amd.engine import MatchPoseConfig
    from oryon_amd.pipeline import Pipeline, default_args
    c = MatchPoseConfig()
    assert (c.subpixel, c.subpixel_curv_min, c.subpixel_depth_jump) == (False, 1e-4, 0.02)
    names = [f.name for f in dataclasses.fields(MatchPoseConfig)]
    assert names[names.index("subpixel"):names.index("subpixel") + 3] == ["subpixel", "subpixel_curv_min", "subpixel_depth_jump"]
    t = default_args().test
    assert (t.subpixel, t.subpixel_curv_min, t.subpixel_depth_jump) == (False, 1e-4, 0.02)
    assert default_args(**{"test.subpixel": True}).test.subpixel is True
    # composes with every match route's flag
    assert MatchPoseConfig(subpixel=True, topk=2).subpixel and MatchPoseConfig(subpixel=True, mutual=True, ratio=0.8).subpixel
    assert MatchPoseConfig(subpixel=True, ratio=0.8, half_descriptors=True, match_mode="exact", solver="spectral").subpixel
    assert MatchPoseConfig(subpixel=True, subpixel_curv_min=0.0, subpixel_depth_jump=float("inf")).subpixel_curv_min == 0.0
    for bad, word in ((dict(subpixel_curv_min=-1e-3), "subpixel_curv_min"), (dict(subpixel_curv_min=float("nan")), "subpixel_curv_min"),
                      (dict(subpixel_curv_min=float("inf")), "subpixel_curv_min"), (dict(subpixel_depth_jump=-0.01), "subpixel_depth_jump"),
                      (dict(subpixel_depth_jump=float("nan")), "subpixel_depth_jump")):
        with pytest.raises(ValueError, match=word):
            MatchPoseConfig(subpixel=True, **bad)
    cfg = MatchPoseConfig(subpixel=True)
    cfg.subpixel_curv_min = -1.0
    with pytest.raises(ValueError, match="subpixel_curv_min"):
        engine._check_subpixel(cfg)
    # the pipeline reads the keys with getattr: args without them keep working, and a bad value raises when the pipeline is built
    args = default_args(**{"test.solver": "ransac"})
    for k in ("subpixel", "subpixel_curv_min", "subpixel_depth_jump"):
        delattr(args.test, k)
    p = Pipeline(args)
    assert p.subpixel_cfg() == (False, 1e-4, 0.02) and p.subpixel_summary() == {}
    with pytest.raises(ValueError, match="subpixel_depth_jump"):
        Pipeline(default_args(**{"test.solver": "ransac", "test.subpixel": True, "test.subpixel_depth_jump": -1.0}))
    on = Pipeline(default_args(**{"test.solver": "ransac", "test.subpixel": True}))
    assert on.subpixel_summary() == dict(subpixel_rows=0, subpixel_refined=0, subpixel_border=0, subpixel_flat=0, subpixel_outside=0,
                                         subpixel_offset_mean=None)
    assert ops.SUBPIX_FLAGS == ("refined", "border", "flat", "outside")
    sys.path.insert(0, ROOT)
    import run_pose
    q = run_pose.parse(["--subpixel", "--subpixel-curv-min", "1e-3", "--subpixel-depth-jump", "0.05", "--solver", "ransac", "--pairs", "4"])
    assert q == ("ransac", ["--pairs", "4"]) and (q.subpixel, q.subpixel_curv_min, q.subpixel_depth_jump) == (True, 1e-3, 0.05)
    q = run_pose.parse(["--solver", "ransac", "--topk", "2", "--subpixel"])
    assert q == ("ransac", []) and q.subpixel and q.topk == 2 and (q.subpixel_curv_min, q.subpixel_depth_jump) == (1e-4, 0.02)
    q = run_pose.parse(["--ratio", "0.8", "--mutual"])
    assert q == ("pointdsc", []) and not q.subpixel and q.ratio == 0.8 and q.mutual
    assert list(inspect.signature(pcd.subpixel_offsets).parameters) == ["feats1", "feats2", "corrs", "curv_min"]
    assert inspect.signature(pcd.subpixel_offsets).parameters["curv_min"].default == 1e-4
    lift, lift_sp = inspect.signature(ops.lift_pairs), inspect.signature(ops.lift_pairs_subpix)
    assert list(lift_sp.parameters) == list(lift.parameters) + ["offsets", "depth_jump"]
    assert lift_sp.parameters["depth_jump"].default == 0.02 and lift_sp.parameters["offsets"].default is None
    assert list(inspect.signature(ops.subpix_refine).parameters) == ["feat_a", "feat_q", "corrs", "n_corr", "status", "curv_min"]
    assert inspect.signature(Pipeline.get_pose).parameters["offsets"].default is None


def test_the_process_wide_default_reaches_config_and_args():
    """What run_pose.py --subpixel sets: MatchPoseConfig() and default_args() follow it, an explicit value still wins."""
    from oryon_amd import engine
    from oryon_amd.pipeline import default_args
    assert engine.default_subpixel() == (False, 1e-4, 0.02)
    try:
        engine.set_default_subpixel(True, 1e-3, 0.05)
        assert engine.default_subpixel() == (True, 1e-3, 0.05)
        c, t = engine.MatchPoseConfig(), default_args().test
        assert (c.subpixel, c.subpixel_curv_min, c.subpixel_depth_jump) == (True, 1e-3, 0.05)
        assert (t.subpixel, t.subpixel_curv_min, t.subpixel_depth_jump) == (True, 1e-3, 0.05)
        assert engine.MatchPoseConfig(subpixel=False).subpixel is False and default_args(**{"test.subpixel": False}).test.subpixel is False
        with pytest.raises(ValueError, match="subpixel_curv_min"):
            engine.set_default_subpixel(True, -1.0)
        with pytest.raises(ValueError, match="subpixel_depth_jump"):
            engine.set_default_subpixel(True, 1e-4, -0.5)
        assert engine.default_subpixel() == (True, 1e-3, 0.05)              # a refused value changes nothing
    finally:
        engine.set_default_subpixel(False)
    assert engine.default_subpixel() == (False, 1e-4, 0.02) and engine.MatchPoseConfig().subpixel is False
