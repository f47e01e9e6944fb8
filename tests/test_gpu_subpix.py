"""test.subpixel on the device (csrc/match_subpix.hip): the fit against the float64 statement and the lift against the float32 one bit
for bit (tests/subpix_restatement.py on the inputs of tests/subpix_cases.py, whose conditions tests/test_subpix_restatement.py asserts
on the host), bit stability over batch position and runs, the chain match -> select -> refine -> lift -> Kabsch on the shifted-field
pair, and the engine, the pipeline's two routes and the per-sample façade."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subpix_cases as sc  # noqa: E402
import subpix_restatement as sr  # noqa: E402
from test_gpu_ransac import _batch  # noqa: E402  (the two-sided batch dict of Pipeline.test_step on the synthetic pairs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
OFFSET_TOL = 1.2e-7          # two fp32 ulps at 0.5: float64 sums of <= 512 terms err by <~ 1e-13, / l_min >= 1e-4 -> <~ 3e-9; the store adds <= 6e-8


def _t(x, dtype=None):
    """a device copy of a (read-only, shared) host array"""
    return torch.tensor(np.asarray(x), device=DEV) if dtype is None else torch.tensor(np.asarray(x), device=DEV, dtype=dtype)


def _maps(case, layout):
    fa, fq = _t(case["feat_a"]), _t(case["feat_q"])
    if layout == "nhwc":
        fa, fq = fa.contiguous(memory_format=torch.channels_last), fq.contiguous(memory_format=torch.channels_last)
    return fa, fq


# ------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("C", sc.FIT_CHANNELS)
def test_fit_against_the_statement(C, layout):
    from oryon_amd import ops
    case = sc.fit_case(C)
    assert sc.fit_conditions(case)                       # planted flags, every gate >= 1e-6 from its threshold: no row is left out
    fa, fq = _maps(case, layout)
    assert ops.map_layout(fa)[1] == (ops.LAYOUT_NHWC if layout == "nhwc" else ops.LAYOUT_NCHW)
    corrs, n_corr = _t(case["corrs"]), _t(case["n_corr"])
    for status in (None, [0, 2, 0], [1, 0, 0]):          # a failure status: that pair does no work, zeros, not counted
        st = None if status is None else torch.tensor(status, dtype=torch.int32, device=DEV)
        out = ops.subpix_refine(fa, fq, corrs, n_corr, st, sc.CURV_MIN)
        torch.cuda.synchronize()
        off, fl, cnt = sc.expected_fit(case, status)
        got_off, got_fl, got_cnt = out["offsets"].cpu().numpy(), out["flags"].cpu().numpy(), out["counts"].cpu().numpy()
        assert got_off.dtype == np.float32 and got_fl.dtype == np.uint8 and got_cnt.dtype == np.int32
        assert np.array_equal(got_fl, fl), np.argwhere(got_fl != fl)[:8]
        assert np.array_equal(got_cnt, cnt), (got_cnt, cnt)
        assert np.isfinite(got_off).all()
        err = np.abs(got_off.astype(np.float64) - off.astype(np.float64))
        print(f"C {C} {layout} status {status}: max |offset - statement| {err.max():.3e}, counts {got_cnt.tolist()}")
        assert err.max() <= OFFSET_TOL
        assert not got_off[fl != 0].any() and (np.abs(got_off) <= 0.5).all()
    # n_corr = NULL: n_cap rows each; counts outside [0, n_cap] are clamped
    full = ops.subpix_refine(fa, fq, corrs, None, None, sc.CURV_MIN)
    wild = ops.subpix_refine(fa, fq, corrs, torch.tensor([500, -3, 128], dtype=torch.int32, device=DEV), None, sc.CURV_MIN)
    assert np.array_equal(full["flags"].cpu().numpy(), case["flags"])
    assert full["counts"].sum(1).tolist() == [sc.FIT_CAP] * 3 and wild["counts"].sum(1).tolist() == [sc.FIT_CAP, 0, sc.FIT_CAP]
    assert torch.equal(wild["offsets"][0], full["offsets"][0]) and not wild["offsets"][1].any()


def test_fit_layouts_agree_and_other_curvature_floors():
    """The channel sums run in one order whatever the layout: the bytes agree.  A floor of 0 keeps every minimum, a large one none."""
    from oryon_amd import ops
    case = sc.fit_case(200)
    corrs = _t(case["corrs"])
    a = ops.subpix_refine(*_maps(case, "nchw"), corrs, None, None, sc.CURV_MIN)
    b = ops.subpix_refine(*_maps(case, "nhwc"), corrs, None, None, sc.CURV_MIN)
    assert torch.equal(a["offsets"].view(torch.int32), b["offsets"].view(torch.int32)) and torch.equal(a["flags"], b["flags"])
    lo = ops.subpix_refine(*_maps(case, "nchw"), corrs, None, None, 0.0)
    hi = ops.subpix_refine(*_maps(case, "nchw"), corrs, None, None, 10.0)
    assert int(hi["counts"][:, 0].sum()) == 0 and int(hi["counts"][:, 3].sum()) == 0 and not hi["offsets"].any()
    assert (lo["counts"][:, 2] <= a["counts"][:, 2]).all() and torch.isfinite(lo["offsets"]).all()
    assert torch.equal(lo["counts"][:, 1], a["counts"][:, 1])


# ------------------------------------------------------------------------------------------------ the lift
def _lift(case, offsets=True, status=None, n_corr=True):
    from oryon_amd import ops
    st = None if status is None else torch.tensor(status, dtype=torch.int32, device=DEV)
    return ops.lift_pairs_subpix(_t(case["corrs"]), _t(case["n_corr"]) if n_corr else None, sc.LIFT_FEAT, _t(case["depth_a"]),
                                 _t(case["depth_q"]), _t(case["cam_a"]), _t(case["cam_q"]), st,
                                 offsets=_t(case["offsets"]) if offsets else None, depth_jump=sc.JUMP_MM / 1000.0)


@pytest.mark.parametrize("q_size,a_size", [(sc.LIFT_SIZES[1], sc.LIFT_SIZES[0]), (sc.LIFT_SIZES[0], sc.LIFT_SIZES[1])])
def test_lift_against_the_statement_bit_for_bit(q_size, a_size):
    case = sc.lift_case(q_size, a_size)
    assert sc.lift_conditions(case)                      # rows pushed out, a hole, the jump under and over, i0 + 1 = H, both branches
    for status in (None, [0, 2, 0]):
        pa, pq, n_out = _lift(case, status=status)
        torch.cuda.synchronize()
        pa, pq, n_out = pa.cpu().numpy(), pq.cpu().numpy(), n_out.cpu().numpy()
        for p, n in enumerate(sc.LIFT_COUNTS):
            wa, wq, keep, _, _ = case["want"][p]
            m = 0 if status is not None and status[p] != 0 else int(keep.sum())
            assert n_out[p] == m, (p, n_out[p], m)
            assert np.array_equal(pa[p, :m].view(np.uint32), wa[:m].view(np.uint32)), p          # compacted, in order, every bit
            assert np.array_equal(pq[p, :m].view(np.uint32), wq[:m].view(np.uint32)), p
            assert not pa[p, m:].any() and not pq[p, m:].any()                                    # the zero tail


def test_lift_without_offsets_is_lift_pairs_where_nothing_is_interpolated():
    """offsets = NULL, depth at the feature size, depths constant over each 2 x 2 block: inside a block the bilinear read returns the
    block's value, across blocks either that or the pixel itself - the bytes of ops.lift_pairs."""
    from oryon_amd import ops
    rng = np.random.default_rng(9)
    B, H, W, cap = 3, 24, 24, 256
    blocks = (500.0 + 400.0 * rng.random((B, H // 2, W // 2))).astype(np.float32)
    blocks[:, 3, 4] = 0.0
    depth = _t(np.repeat(np.repeat(blocks, 2, axis=1), 2, axis=2))
    corrs = _t(np.stack([rng.integers(0, H, (B, cap)), rng.integers(0, W, (B, cap)), rng.integers(0, H, (B, cap)), rng.integers(0, W, (B, cap))],
                        axis=2).astype(np.int32))
    n_corr = torch.tensor([256, 77, 0], dtype=torch.int32, device=DEV)
    cam = _t(np.array([[600.0, 0, 11.7, 0, 595.0, 12.2, 0, 0, 1]] * B, np.float32))
    for jump in (0.0, 0.02, float("inf")):
        got = ops.lift_pairs_subpix(corrs, n_corr, (H, W), depth, depth, cam, cam, None, offsets=None, depth_jump=jump)
        want = ops.lift_pairs(corrs, n_corr, (H, W), depth, depth, cam, cam, None)
        zero = ops.lift_pairs_subpix(corrs, n_corr, (H, W), depth, depth, cam, cam, None, offsets=torch.zeros((B, cap, 2), device=DEV),
                                     depth_jump=jump)
        for g, z, w in zip(got, zero, want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)) and torch.equal(z.view(torch.int32), w.view(torch.int32))


# ------------------------------------------------------------------------------------------------ bit stability
def test_both_kernels_are_bit_stable_over_batch_position_and_runs():
    from oryon_amd import ops
    case = sc.fit_case(256)
    order = [0, 1, 0]                                                     # the same pair at batch positions 0 and 2
    for layout in ("nchw", "nhwc"):
        fa, fq = _maps(dict(feat_a=case["feat_a"][order], feat_q=case["feat_q"][order]), layout)
        corrs = _t(case["corrs"][order])
        n = torch.tensor([128, 37, 128], dtype=torch.int32, device=DEV)
        first = ops.subpix_refine(fa, fq, corrs, n, None, sc.CURV_MIN)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            again = ops.subpix_refine(fa, fq, corrs, n, None, sc.CURV_MIN)
        torch.cuda.synchronize()
        for k in ("offsets", "flags", "counts"):
            assert first[k][0].cpu().numpy().tobytes() == first[k][2].cpu().numpy().tobytes(), (layout, k)
            assert first[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), (layout, k)
    lc = sc.lift_case(sc.LIFT_SIZES[1], sc.LIFT_SIZES[0])
    twice = {k: (v[order] if isinstance(v, np.ndarray) and v.shape[0] == 3 and k != "n_corr" else v) for k, v in lc.items()}
    twice["n_corr"] = np.array([128, 100, 128], np.int32)
    one, two = _lift(twice), _lift(twice)
    torch.cuda.synchronize()
    for a, b in zip(one, two):
        assert a[0].cpu().numpy().tobytes() == a[2].cpu().numpy().tobytes() and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ the chain
SHIFT = (0.3, -0.2)


@pytest.mark.parametrize("scale", [1, 2])
def test_chain_at_least_halves_the_translation_error(scale):
    """The shifted-field pair (C = 32, 24 x 24, shortest period 32 px), both sides on a fronto-parallel plane at 600 mm with f = 600 px:
    one depth pixel is one millimetre.  match -> select_corrs -> subpix_refine -> lift_pairs_subpix -> kabsch_batched against the same
    chain through lift_pairs: the translation error against the known shift at most half.  Measured: see the print."""
    from oryon_amd import ops
    FH = FW = 24
    fa_np, fq_np = sr.shifted_fields(32, FH, FW, 32.0, SHIFT)
    fa, fq = _t(fa_np)[None], _t(fq_np)[None]
    mask_a = torch.zeros((1, FH, FW), dtype=torch.int32, device=DEV)
    mask_a[:, 3:FH - 3, 3:FW - 3] = 1                                     # interior anchors
    mask_q = torch.ones((1, FH, FW), dtype=torch.int32, device=DEV)
    roi_a, n_a = ops.roi_compact(mask_a)
    roi_q, n_q = ops.roi_compact(mask_q)
    cap = ops.round_up(FH * FW, ops.ROW_PAD)
    a_hat, q_hat = ops.gather_normalise(fa, roi_a, n_a, cap), ops.gather_normalise(fq, roi_q, n_q, cap)
    md, am, valid = ops.match(a_hat, q_hat, n_a, n_q, 0.25)
    corrs, n_valid, n_sel, status = ops.select_corrs(roi_a, roi_q, n_a, n_q, am, valid, FW, 200, 1)
    assert status.tolist() == [0] and n_valid.tolist() == [(FH - 6) * (FW - 6)] and n_sel.tolist() == [200]
    sub = ops.subpix_refine(fa, fq, corrs, n_sel, status, 1e-4)
    HD = FH * scale
    depth = torch.full((1, HD, HD), 600.0, dtype=torch.float32, device=DEV)
    cam = torch.tensor([[600.0, 0, HD / 2, 0, 600.0, HD / 2, 0, 0, 1]], dtype=torch.float32, device=DEV)
    t_true = np.array([SHIFT[1] * scale, SHIFT[0] * scale, 0.0]) / 1000.0   # the anchor's pixel (y, x) lies at (y + sy, x + sx)
    err = {}
    for name, (pa, pq, n) in (("integer", ops.lift_pairs(corrs, n_sel, (FH, FW), depth, depth, cam, cam, status)),
                              ("subpixel", ops.lift_pairs_subpix(corrs, n_sel, (FH, FW), depth, depth, cam, cam, status,
                                                                 offsets=sub["offsets"], depth_jump=0.02))):
        assert n.tolist() == [200]
        T = ops.kabsch_batched(pa, pq).cpu().numpy().astype(np.float64)[0]
        err[name] = float(np.linalg.norm(T[:3, 3] - t_true)) * 1000.0
    print(f"scale {scale}: translation error {err['integer']:.4f} mm through lift_pairs, {err['subpixel']:.4f} mm refined, ratio "
          f"{err['subpixel'] / err['integer']:.3f}, flags {sub['counts'].tolist()}")
    assert err["subpixel"] <= 0.5 * err["integer"]


# ------------------------------------------------------------------------------------------------ engine, pipeline, façade
H, C, B = 48, 32, 4


@pytest.fixture(scope="module")
def mb():
    from oryon_amd.synth import make_batch
    return make_batch(40, B, H, H, C, device=DEV)


def _run(mb, **cfg):
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    eng = MatchPoseEngine(None, MatchPoseConfig(solver="ransac", n_corrs=200, **cfg))
    key = torch.arange(40, 40 + B, dtype=torch.int64, device=DEV)
    out = eng.run(mb["feat_a"], mb["feat_q"], mb["mask_a"], mb["mask_q"], mb["depth_a"], mb["depth_q"], mb["camera"].to(DEV),
                  mb["camera"].to(DEV), key, keep=True)
    torch.cuda.synchronize()
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


@pytest.mark.parametrize("cfg", [dict(), dict(topk=2), dict(mutual=True)], ids=["plain", "topk2", "mutual"])
def test_engine_refines_the_rows_it_selected_anyway(mb, cfg):
    from oryon_amd import ops
    off, on = _run(mb, **cfg), _run(mb, subpixel=True, **cfg)
    new = {"subpix_offsets", "subpix_flags", "subpix_counts"}
    assert new.isdisjoint(off) and new <= set(on)                          # off: no new key (the plain run is the native step's)
    assert torch.equal(on["n_valid"], off["n_valid"]) and on["status"].tolist() == off["status"].tolist() == [0] * B
    n_rows = on["n_rows"] if "n_rows" in on else torch.full((B,), 200, dtype=torch.int32, device=DEV)
    if "n_rows" in on:
        assert torch.equal(on["n_rows"], off["n_rows"])
    for b, n in enumerate(n_rows.tolist()):                                # which rows the solver sees does not change
        assert torch.equal(on["corrs"][b, :n], off["corrs"][b, :n])
        assert torch.equal(on["pcd_a"][b, :n], off["pcd_a"][b, :n])       # the anchor side has no offset: whole pixels, f = 0
    assert torch.equal(on["n_lifted"], off["n_lifted"])
    assert on["subpix_counts"].sum(1).tolist() == n_rows.tolist() and int(on["subpix_counts"][:, 0].sum()) > 0
    # the keys are the two entry points on the selected rows
    ref = ops.subpix_refine(mb["feat_a"], mb["feat_q"], on["corrs"], n_rows, on["status"], 1e-4)
    for k in ("offsets", "flags", "counts"):
        assert torch.equal(on["subpix_" + k], ref[k]), k
    cam = mb["camera"].to(DEV).reshape(B, 9).to(torch.float32).contiguous()
    pa, pq, n = ops.lift_pairs_subpix(on["corrs"], n_rows, (H, H), mb["depth_a"], mb["depth_q"], cam, cam, on["status"],
                                      offsets=ref["offsets"], depth_jump=0.02)
    assert torch.equal(pq, on["pcd_q"]) and torch.equal(pa, on["pcd_a"]) and torch.equal(n, on["n_lifted"])
    assert not torch.equal(on["pcd_q"], off["pcd_q"])


def _pipeline(**over):
    from oryon_amd.pipeline import Pipeline, default_args
    args = default_args(**{"test.mask": "oracle", "test.solver": "ransac", "model.image_encoder.img_size": [H, H], "dataset.img_size": [H, H],
                           "test.n_corrs": 200, **over})
    return Pipeline(args, pointdsc_solver=None)


def test_pipeline_runs_both_routes_and_sums_up_the_rows():
    from oryon_amd.pipeline import subpixel_summary
    pl = _pipeline(**{"test.subpixel": True})
    batch, _ = _batch(3, 2)
    torch.manual_seed(1)
    saved = np.random.get_state()
    try:
        np.random.seed(1)
        recs = pl.test_step(batch, 0)
    finally:
        np.random.set_state(saved)
    assert [r["status"] for r in recs] == [0, 0] and pl.last_subpixel is not None and pl.last_subpixel[0].shape == (200, 2)
    s = pl.subpixel_summary()
    assert s["subpixel_rows"] == 400 == s["subpixel_refined"] + s["subpixel_border"] + s["subpixel_flat"] + s["subpixel_outside"]
    assert s["subpixel_refined"] > 0 and 0.0 < s["subpixel_offset_mean"] <= 0.5 ** 0.5
    out = pl.test_step_batched(batch, first_pair_index=3)
    torch.cuda.synchronize()
    assert out["status"].tolist() == [0, 0] and pl._engine._native is None and out["subpix_counts"].sum(1).tolist() == [200, 200]
    s2 = pl.subpixel_summary()
    assert s2["subpixel_rows"] == 800 == s2["subpixel_refined"] + s2["subpixel_border"] + s2["subpixel_flat"] + s2["subpixel_outside"]
    assert s2["subpixel_refined"] == s["subpixel_refined"] + int(out["subpix_counts"][:, 0].sum())
    assert subpixel_summary() == s2                                       # what a driver around the pipeline reads
    # off: no launch, no key, no summary; the per-sample route hands get_pose no offsets
    plain = _pipeline()
    out0 = plain.test_step_batched(batch, first_pair_index=3)
    assert not any(k.startswith("subpix") for k in out0) and plain.subpixel_summary() == {}
    for o in (out, out0):
        assert o["status"].tolist() == [0, 0] and bool(torch.isfinite(o["pose"]).all())
    for r in recs:
        assert bool(torch.isfinite(r["pred_pose_rel"]).all()) and r["pred_pose_rel"][3].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_per_sample_facade_equals_the_batched_entry(mb):
    from oryon_amd import ops, pcd
    on = _run(mb, subpixel=True)
    for b in (0, 3):
        corrs = on["corrs"][b, :200]
        off, fl = pcd.subpixel_offsets(mb["feat_a"][b], mb["feat_q"][b], corrs.to(torch.int64))
        assert off.shape == (200, 2) and fl.shape == (200,) and off.dtype == torch.float32 and fl.dtype == torch.uint8
        assert torch.equal(off, on["subpix_offsets"][b, :200]) and torch.equal(fl, on["subpix_flags"][b, :200])
    off, fl = pcd.subpixel_offsets(mb["feat_a"][0], mb["feat_q"][0], torch.zeros((0, 4), dtype=torch.int64, device=DEV))
    assert off.shape == (0, 2) and fl.shape == (0,)
