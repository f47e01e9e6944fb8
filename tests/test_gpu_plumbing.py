"""GPU sweep of the kernels that feed the matcher and score its output - the K-1 resizes (csrc/preproc.hip, csrc/roi.hip), roi_compact
(csrc/roi.hip), the K2 lifts (csrc/post.hip) and the pose metrics (csrc/evaluate.hip) - against the numpy statements of
tests/plumbing_restatement.py on the seeded cases of tests/plumbing_cases.py.  tests/test_plumbing_restatement.py checks the statements
against independent references and the cases' premises on the CPU.

Bars (e = 2^-24):
  rgb              |got - want64| <= e |want64| + 1e-15: one float32 rounding of a float64 value (1e-15: the float64 evaluation order);
                   an all-0 image gives exactly 0, an all-255 image exactly 1.0, a constant image a constant.
  depth            |got - want64| <= 4e (WI S_x + HI S_y + M) per pixel (plumbing_restatement.depth_bar carries the derivation).
  depth, rounded   outside the band |frac(want64) - 0.5| <= bar: got == rint(want64) exactly; inside: an integer within 0.5 + bar.  At most
                   5 % of a case's pixels lie in the band (asserted on the CPU from the statement).
  dyadic           the unrounded output IS the float64 statement, the rounded one np.rint of it (half to even) on every pixel, ties included.
  mask, roi_compact, lift_pairs, lift_points     equal, bit for bit; lift_pairs rows at or past n_out exactly 0.0 over a NaN pre-fill.
  ADD, ADD-S       |got - want| <= (16 + M/256) e want against the float64 statistic of the half-transformed clouds (the kernel's documented
                   rule): the float32 roundings of one distance, eight reduction levels, ceil(M/256) atomic adds of non-negative terms, the
                   division.  Equal poses: exactly 0.
  rotation, translation error     |got - want| <= 2^-23 max(|want|, 1) against evaluation.compute_RT_distances.

What each of these mistakes would fail (reasoned from the code, not run): no upper clamp on the tap (`i1 = i0 + 1`): the up-sampling cases,
whose three images differ; sx and sy swapped: every non-square ratio; a wrong HWC -> CHW stride: rgb, whose channels differ; roundf
for rintf: the dyadic ties at even k; `base += total` dropped in roi_compact: HW >= 8193; the 16-byte path on a misaligned map: 31x37;
`base` not carried between lift chunks: n_cap = 1300 mixed; zero_from starting at the wrong row: the NaN pre-fill; an off-by-one in
`blockIdx.x * 256 >= M`: M = 256; in the tile limit `lim`: ADD-S at M = 1024 and 1025.

Measured on the MI355X (worst error / bar over all cases, printed by the tests): rgb 0.999 (a correctly rounded value can sit on the bar),
depth 0.656 (up8_5x3_to_40x56_n70, float-valued; 0.461 on integer depths), ADD 0.093, ADD-S 0.133, rotation / translation 0.371.  Rounded
depth: 0 to 162 pixels per case differ from rint(want64), every one inside the band; band shares 0.00 % to 2.89 % (production size).
Before move_f16 pinned its fp32 sum (evaluate.hip) M = 2500 missed the ADD bar 14.9 times and the ADD-S bar 28.4 times over: one point of
the 2500 sat on a rounding tie of the half grid and the fused conversion rounded the exact sum instead."""
import numpy as np
import pytest
import torch

import plumbing_cases as pc
import plumbing_restatement as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = 2.0 ** -24


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)                 # a copy: the cases are read-only


# ------------------------------------------------------------------------------------------------------------------ K-1 resizes
@pytest.mark.parametrize("name", list(pc.RESIZE))
def test_rgb_resize_against_the_float64_statement(name):
    from oryon_amd import ops
    (HI, WI), out_hw, n, _ = pc.RESIZE[name]
    u8 = pc.rgb_images(name)
    got = ops.rgb_resize_bilinear(dev(u8), out_hw).cpu().numpy()
    want = pr.rgb64(u8, out_hw)
    assert got.shape == want.shape and got.dtype == np.float32
    ratio = np.abs(got - want) / (E * np.abs(want) + 1e-15)
    print(name, f"rgb worst err/bar {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    const = np.zeros((3, HI, WI, 3), dtype=np.uint8)
    const[1], const[2, ..., 0], const[2, ..., 1], const[2, ..., 2] = 255, 7, 130, 201
    out = ops.rgb_resize_bilinear(dev(const), out_hw).cpu().numpy()
    assert (out[0] == 0.0).all() and (out[1] == 1.0).all()
    for c in range(3):
        assert (out[2, c] == out[2, c, 0, 0]).all() and abs(out[2, c, 0, 0] - (7, 130, 201)[c] / 255.0) <= E


@pytest.mark.parametrize("kind", ["float", "int"])
@pytest.mark.parametrize("name", list(pc.RESIZE))
def test_depth_resize_unrounded_within_the_derived_bar(name, kind):
    from oryon_amd import ops
    _, out_hw, _, _ = pc.RESIZE[name]
    x = pc.depth_float(name) if kind == "float" else pc.depth_int(name)
    got = ops.resize_bilinear(dev(x), out_hw).cpu().numpy().astype(np.float64)
    want, tol = pr.bilinear64(x, out_hw), pr.depth_bar(x, out_hw)
    err = np.abs(got - want)
    ratio = np.where(err == 0.0, 0.0, err / np.maximum(tol, 1e-300))                  # inside a hole the bar is 0 and so is the output
    print(name, kind, f"depth worst err/bar {ratio.max():.3f}")
    assert got.shape == want.shape and ratio.max() <= 1.0


@pytest.mark.parametrize("name", list(pc.RESIZE))
def test_depth_resize_rounded(name):
    from oryon_amd import ops
    _, out_hw, _, _ = pc.RESIZE[name]
    x = pc.depth_int(name)
    got = ops.resize_bilinear(dev(x), out_hw, round_output=True).cpu().numpy().astype(np.float64)
    want, tol = pr.bilinear64(x, out_hw), pr.depth_bar(x, out_hw)
    band = pc.band(want, tol)
    off = got != np.rint(want)
    print(name, f"band share {100 * band.mean():.2f} %, pixels off rint(want64): {int(off.sum())} (all inside the band: {not (off & ~band).any()})")
    assert band.mean() <= pc.BAND_CAP
    assert not (off & ~band).any()
    assert np.array_equal(got, np.rint(got)) and (np.abs(got - want)[band] <= 0.5 + tol[band]).all()


@pytest.mark.parametrize("name", list(pc.DYADIC))
def test_depth_resize_dyadic_is_exact_and_rounds_half_to_even(name):
    from oryon_amd import ops
    _, out_hw, _, _ = pc.DYADIC[name]
    x = pc.dyadic_depth(name)
    want = pr.bilinear64(x, out_hw)
    got = ops.resize_bilinear(dev(x), out_hw).cpu().numpy().astype(np.float64)
    assert np.array_equal(got, want)
    rounded = ops.resize_bilinear(dev(x), out_hw, round_output=True).cpu().numpy().astype(np.float64)
    assert np.array_equal(rounded, np.rint(want))


@pytest.mark.parametrize("name", list(pc.RESIZE))
def test_mask_resize_nearest_equals_the_statement(name):
    from oryon_amd import ops
    _, out_hw, _, _ = pc.RESIZE[name]
    m = pc.masks(name)
    got = ops.mask_resize_nearest(dev(m), out_hw)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), pr.nearest(m, out_hw))


# ------------------------------------------------------------------------------------------------------------------ roi_compact
@pytest.mark.parametrize("name", list(pc.COMPACT))
def test_roi_compact_equals_the_statement(name):
    """The list is compared up to `count`; entries past it are unspecified."""
    from oryon_amd import ops
    m = pc.compact_masks(name)
    roi, count = ops.roi_compact(dev(m))
    roi, count = roi.cpu().numpy(), count.cpu().numpy()
    for i, want in enumerate(pr.compact(m)):
        assert count[i] == len(want), (i, count[i], len(want))
        assert np.array_equal(roi[i, :count[i]], want), i


# ------------------------------------------------------------------------------------------------------------------ K2 lifts
def run_lift_pairs(corrs, n_corr, status, feat_hw, s, B):
    """The C entry on NaN-filled outputs -> (pcd_a, pcd_q [B,n_cap,3], n_out [B]) as numpy."""
    from oryon_amd import _lib
    cap = corrs.shape[1]
    c, nc, st = dev(corrs[:B]), dev(n_corr), dev(status)
    da, dq, ca, cq = (dev(s[k][:B]) for k in ("depth_a", "depth_q", "cam_a", "cam_q"))
    pa = torch.full((B, cap, 3), float("nan"), dtype=torch.float32, device=DEV)
    pq = torch.full((B, cap, 3), float("nan"), dtype=torch.float32, device=DEV)
    n_out = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _lib.require_gpu(DEV)
    _lib.check(_lib.lib().oryon_lift_pairs(_lib.ptr(c), _lib.ptr(nc), B, cap, feat_hw[0], feat_hw[1], _lib.ptr(da), da.shape[1], da.shape[2],
                                           _lib.ptr(dq), dq.shape[1], dq.shape[2], _lib.ptr(ca), _lib.ptr(cq), _lib.ptr(st), _lib.ptr(pa),
                                           _lib.ptr(pq), _lib.ptr(n_out), _lib.stream_ptr(DEV)), "oryon_lift_pairs")
    torch.cuda.synchronize()
    return pa.cpu().numpy(), pq.cpu().numpy(), n_out.cpu().numpy()


def check_lift_pair(tag, got, p, want, n, ok):
    """Pair p of a call against the statement on its first n rows (none when its status is not 0)."""
    pa, pq, n_out = got
    wa, wq, keep = want
    m = int(keep[:n].sum()) if ok else 0
    assert n_out[p] == m, (tag, p, n_out[p], m)
    assert np.array_equal(pa[p, :m], wa[:m]) and np.array_equal(pq[p, :m], wq[:m]), (tag, p)       # bit for bit: no NaN among them
    for cloud in (pa, pq):
        tail = cloud[p, m:]
        assert (tail == 0.0).all() and not np.signbit(tail).any(), (tag, p)                          # NaN fails ==


@pytest.mark.parametrize("name", list(pc.LIFT))
def test_lift_pairs_against_the_statement(name):
    grid, cap, _ = pc.LIFT[name]
    s, corrs, want = pc.lift_scene(grid), pc.lift_corrs(name), pc.lift_want(name)
    for n_corr, status in pc.lift_counts(cap):
        got = run_lift_pairs(corrs, n_corr, status, pc.LIFT_GRIDS[grid][0], s, pc.LIFT_B)
        for p in range(pc.LIFT_B):
            check_lift_pair(name, got, p, want[p], int(n_corr[p]), status[p] == 0)


@pytest.mark.parametrize("name", ["g192_cap300_mixed", "g48_cap513_mixed"])
def test_lift_pairs_clamps_the_row_count(name):
    """Pair 0 of 3 claims n_cap + 7 rows: its result is the n_cap one, and pairs 1 and 2 are untouched.  (Unclamped, the kernel read seven
    rows of pair 1's correspondences and wrote up to seven rows into pair 1's clouds - inside the batch's allocations.)"""
    grid, cap, _ = pc.LIFT[name]
    s, corrs, want = pc.lift_scene(grid), pc.lift_corrs(name), pc.lift_want(name)
    n_corr, status = np.array([cap + 7, cap // 2, cap], dtype=np.int32), np.zeros(3, dtype=np.int32)
    got = run_lift_pairs(corrs, n_corr, status, pc.LIFT_GRIDS[grid][0], s, 3)
    for p in range(3):
        check_lift_pair(name, got, p, want[p], min(int(n_corr[p]), cap), True)
    neg = run_lift_pairs(corrs, np.array([-5, cap, 1], dtype=np.int32), status, pc.LIFT_GRIDS[grid][0], s, 3)
    for p, n in enumerate((0, cap, 1)):
        check_lift_pair(name, neg, p, want[p], n, True)


@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("n", pc.LIFT_POINTS_N)
def test_lift_points_against_the_statement(n, idx_dtype):
    from oryon_amd import ops
    d, cam, x, y = pc.lift_points_case(n)
    got = ops.lift_points(dev(d), dev(cam), dev(x).to(idx_dtype), dev(y).to(idx_dtype))
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3)
    assert np.array_equal(got.cpu().numpy(), pr.lift_points(d, cam, x, y))


# ------------------------------------------------------------------------------------------------------------------ pose metrics
def check_pose(tag, out, want_stats, M_of_pair):
    theta, shift = pc.rt_want()
    assert out.shape == (len(pc.POSE_PAIRS), 4) and out.dtype == np.float32 and np.isfinite(out).all()
    worst = {"ADD": 0.0, "ADD-S": 0.0, "R/t": 0.0}
    for i in range(out.shape[0]):
        for k, key in ((0, "ADD"), (1, "ADD-S")):
            want = want_stats[i, k]
            if want == 0.0:
                assert out[i, k] == 0.0, (tag, i, key)
            else:
                worst[key] = max(worst[key], abs(out[i, k] - want) / ((16 + M_of_pair[i] / 256.0) * E * want))
        for k, want in ((2, theta[i]), (3, shift[i])):
            worst["R/t"] = max(worst["R/t"], abs(out[i, k] - want) / (2.0 ** -23 * max(abs(want), 1.0)))
    print(tag, "worst err/bar:", {k: f"{v:.3f}" for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, (tag, worst)
    eq = pc.POSE_PAIRS.index("equal")
    assert out[eq, 0] == 0.0 and out[eq, 1] == 0.0 and out[eq, 3] == 0.0
    assert out[eq, 2] == np.float32(np.arccos(1 - 1e-12) * 180 / np.pi)


@pytest.mark.parametrize("M", pc.POSE_M)
def test_pose_metrics_against_the_half_transform_statement(M):
    from oryon_amd import ops
    pred, gt = pc.pose_pairs()
    out = ops.pose_metrics(dev(pred), dev(gt), dev(pc.model(M))).cpu().numpy()
    check_pose(f"M={M}", out, pc.pose_want(M), [M] * len(pc.POSE_PAIRS))


def test_pose_metrics_many_models_in_one_call():
    """Models of 2500, 1, 300 and 0 points behind one offset table: the blocks past a small model return early, the empty model gives 0, 0."""
    from oryon_amd import ops
    pred, gt = pc.pose_pairs()
    models = [pc.model(M, salt=1) for M in pc.MULTI_SIZES]
    off = np.concatenate([[0], np.cumsum(pc.MULTI_SIZES)]).astype(np.int32)
    which = np.array(pc.MULTI_MODEL_OF_PAIR, dtype=np.int32)
    out = ops.pose_metrics(dev(pred), dev(gt), dev(np.concatenate(models)), dev(off), dev(which)).cpu().numpy()
    want = np.array([pc.pose_want(pc.MULTI_SIZES[m], 1)[i] for i, m in enumerate(which)])
    empty = [i for i, m in enumerate(which) if pc.MULTI_SIZES[m] == 0]
    assert empty and (want[empty] == 0).all() and (out[empty, :2] == 0.0).all()
    check_pose("multi", out, want, [pc.MULTI_SIZES[m] for m in which])
