"""The inputs of tests/test_gpu_subpix.py, built on the host so that their conditions can be asserted without a device
(tests/test_subpix_restatement.py does): the fit's batch with its planted rows, and the lift's rows, offsets and depth maps."""
import functools

import numpy as np

import subpix_restatement as sr

F32 = np.float32

# ------------------------------------------------------------------------------------------------ the fit
FIT_B, FIT_H, FIT_W, FIT_CAP = 3, 24, 20, 128
FIT_COUNTS = (128, 37, 0)
FIT_CHANNELS = (32, 200, 256)
CURV_MIN = 1e-4
GATE_MARGIN = 1e-6
# planted rows: name -> index among the first rows of every pair (all below the smallest non-zero count)
PLANTED = dict(edge_top=0, edge_bottom=1, edge_left=2, edge_right=3, corner_00=4, corner_01=5, corner_10=6, corner_11=7, constant=8,
               maximum=9, far_minimum=10, zero_anchor=11, zero_neighbour=12, duplicate_a=13, duplicate_b=14, anchor_outside=15)
WANT = dict(edge_top=1, edge_bottom=1, edge_left=1, edge_right=1, corner_00=1, corner_01=1, corner_10=1, corner_11=1, constant=2, maximum=2,
            far_minimum=3, zero_anchor=2, anchor_outside=1)


def _fit_pair(C, seed):
    """One pair: smooth maps (the query map is the anchor field shifted by a fraction of a pixel), 128 rows - the planted ones first,
    exhaustive nearest neighbours of interior anchors behind them.  Planted anchor descriptors sit at pixels of the outer band, which
    no nearest-neighbour row uses; planted query pixels change the stencils of the rows around them, which the statement sees too."""
    H, W = FIT_H, FIT_W
    fa, fq = sr.shifted_fields(C, H, W, 16.0, (0.3, -0.2), seed=seed)
    nn = sr.nearest_rows(fa, fq, margin=3)
    rows = np.zeros((FIT_CAP, 4), np.int32)
    P = PLANTED
    rows[P["edge_top"]], rows[P["edge_bottom"]] = (5, 5, 0, 7), (5, 5, H - 1, 7)
    rows[P["edge_left"]], rows[P["edge_right"]] = (5, 5, 9, 0), (5, 5, 9, W - 1)
    rows[P["corner_00"]], rows[P["corner_01"]], rows[P["corner_10"]], rows[P["corner_11"]] = (5, 5, 0, 0), (5, 5, 0, W - 1), (5, 5, H - 1, 0), (5, 5, H - 1, W - 1)
    rows[P["anchor_outside"]] = (H, 5, 9, 9)
    fq[:, 3:6, 3:6] = fq[:, 4, 4][:, None, None]                    # a constant patch around query pixel (4, 4)
    rows[P["constant"]] = (4, 4, 4, 4)
    fa[:, 0, 1] = -fq[:, 12, 9]                                     # the opposite descriptor: distance 1 at the centre, a maximum
    rows[P["maximum"]] = (0, 1, 12, 9)
    fa[:, 0, 2] = fq[:, 16, 12]                                     # the descriptor of a pixel three columns away: a steep monotone
    rows[P["far_minimum"]] = (0, 2, 16, 9)                          # patch whose fitted minimum lies more than a pixel to the right
    fa[:, 0, 3] = 0.0                                               # eps clamp: every distance 0.5
    rows[P["zero_anchor"]] = (0, 3, 19, 6)
    fq[:, 20, 15] = 0.0                                             # ... and one stencil value 0.5 among ordinary ones
    rows[P["zero_neighbour"]] = (20, 14, 20, 14)
    rows[P["duplicate_a"]] = rows[P["duplicate_b"]] = nn[40]
    n0 = len(PLANTED)
    rows[n0:] = nn[np.arange(FIT_CAP - n0) * 2 % len(nn)]
    return fa, fq, rows


@functools.lru_cache(maxsize=None)
def fit_case(C):
    """-> dict(feat_a, feat_q [B,C,H,W] float32, corrs [B,128,4] int32, n_corr [B], and the restatement per pair over ALL 128 rows:
    offsets [B,128,2], flags [B,128], gates [B,128,2]).  Computed once per C and shared: read-only."""
    pairs = [_fit_pair(C, 11 + 7 * p) for p in range(FIT_B)]
    ref = [sr.refine(fa, fq, rows, CURV_MIN) for fa, fq, rows in pairs]
    out = dict(feat_a=np.stack([p[0] for p in pairs]), feat_q=np.stack([p[1] for p in pairs]), corrs=np.stack([p[2] for p in pairs]),
               n_corr=np.array(FIT_COUNTS, np.int32), offsets=np.stack([r[0] for r in ref]), flags=np.stack([r[1] for r in ref]),
               gates=np.stack([r[2] for r in ref]))
    for v in out.values():
        v.setflags(write=False)
    return out


def fit_conditions(case):
    """What the comparison with the device rests on: the planted rows carry the flags they were planted for, every flag value occurs,
    and no row's gate quantity lies within GATE_MARGIN of its threshold (so float64 sums in another order decide every gate alike)."""
    for p in range(FIT_B):
        fl, gates = case["flags"][p], case["gates"][p]
        for name, want in WANT.items():
            assert fl[PLANTED[name]] == want, (p, name, int(fl[PLANTED[name]]))
        assert fl[PLANTED["duplicate_a"]] == fl[PLANTED["duplicate_b"]] == 0
        assert set(fl[:37].tolist()) == {0, 1, 2, 3} and np.isfinite(case["offsets"][p]).all()
        ev = fl != 1
        assert (np.abs(gates[ev, 0]) >= GATE_MARGIN).all(), (p, np.abs(gates[ev, 0]).min())
        open_ = ev & (fl != 2)
        assert (np.abs(gates[open_, 1]) >= GATE_MARGIN).all(), (p, np.abs(gates[open_, 1]).min())
    return True


def expected_fit(case, status=None):
    """(offsets, flags, counts) as the device must return them: rows past the count and pairs with a failure status zeroed."""
    off, fl = case["offsets"].copy(), case["flags"].copy()
    cnt = np.zeros((FIT_B, 4), np.int32)
    for p in range(FIT_B):
        n = 0 if status is not None and status[p] != 0 else int(case["n_corr"][p])
        off[p, n:], fl[p, n:] = 0, 0
        cnt[p] = sr.counts(fl[p], n)
    return off, fl, cnt


# ------------------------------------------------------------------------------------------------ the lift
LIFT_FEAT = (24, 24)
LIFT_SIZES = ((30, 41), (48, 64))
LIFT_CAP = 128
LIFT_COUNTS = (128, 100, 0)
JUMP_MM = 20.0
# special rows (query side): name -> (row index, (y_q, x_q), (dy, dx) per query size)
LIFT_SPECIAL = dict(out_right=3, out_negative=7, last_row_col=11, hole=15, jump_under=19, jump_over=23, nan_offset=27)


def _plane(H, W):
    """a slanted plane with a 100 mm step edge down the middle, millimetres"""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return (600.0 + 1.5 * x + 0.7 * y + 100.0 * (x > W / 2)).astype(F32)


def _cell(y2, x2, dy, dx, size):
    """(i0, j0) of the query pixel after the offset, in the float32 arithmetic of the lift"""
    sy, sx = F32(F32(size[0]) / F32(LIFT_FEAT[0])), F32(F32(size[1]) / F32(LIFT_FEAT[1]))
    return int(F32(F32(F32(y2) + F32(dy)) * sy)), int(F32(F32(F32(x2) + F32(dx)) * sx))


@functools.lru_cache(maxsize=None)
def lift_case(q_size, a_size):
    """-> dict(corrs [B,128,4], offsets [B,128,2], n_corr, status, depth_a [B,Ha,Wa], depth_q [B,Hq,Wq], cam_a, cam_q [B,9]) with the
    special rows planted on the query side of every pair, and `want`: per pair the restatement (pcd_a, pcd_q, keep, bil_a, bil_q)
    over the pair's counted rows."""
    B = 3
    rng = np.random.default_rng(q_size[0] * 100 + a_size[0])
    FH, FW = LIFT_FEAT
    corrs = np.stack([rng.integers(0, FH, (B, LIFT_CAP)), rng.integers(0, FW, (B, LIFT_CAP)), rng.integers(0, FH, (B, LIFT_CAP)),
                      rng.integers(0, FW, (B, LIFT_CAP))], axis=2).astype(np.int32)
    offsets = rng.uniform(-0.5, 0.5, (B, LIFT_CAP, 2)).astype(F32)
    depth_a = np.stack([_plane(*a_size) + F32(3 * p) for p in range(B)])
    depth_q = np.stack([_plane(*q_size) + F32(5 * p) for p in range(B)])
    S = LIFT_SPECIAL
    need_y, need_x = (q_size[0] - 1) / (q_size[0] / FH) - (FH - 1), (q_size[1] - 1) / (q_size[1] / FW) - (FW - 1)
    for p in range(B):
        corrs[p, S["out_right"], 2:], offsets[p, S["out_right"]] = (10, FW - 1), (0.0, 1.0)              # x' = W: not inside
        corrs[p, S["out_negative"], 2:], offsets[p, S["out_negative"]] = (0, 10), (-0.25, 0.0)           # y' < 0
        corrs[p, S["last_row_col"], 2:], offsets[p, S["last_row_col"]] = (FH - 1, FW - 1), (need_y + 0.01, need_x + 0.01)
        corrs[p, S["nan_offset"], 2:], offsets[p, S["nan_offset"]] = (9, 9), (np.nan, 0.0)
        for name, yx, z11 in (("hole", (5, 6), 0.0), ("jump_under", (12, 4), 720.0 - 0.002), ("jump_over", (17, 5), 720.0 + 0.002)):
            corrs[p, S[name], 2:], offsets[p, S[name]] = yx, (0.25, 0.125)
            i0, j0 = _cell(*yx, 0.25, 0.125, q_size)
            depth_q[p, i0:i0 + 2, j0:j0 + 2] = 700.0
            depth_q[p, i0 + 1, j0 + 1] = z11
    cam = np.array([[600.0 + p, 0, q_size[1] / 2 + 0.3, 0, 590.0 - p, q_size[0] / 2 - 0.7, 0, 0, 1] for p in range(B)], F32)
    cam_a = np.array([[580.0 + p, 0, a_size[1] / 2 - 0.4, 0, 585.0, a_size[0] / 2 + 0.2, 0, 0, 1] for p in range(B)], F32)
    want = [sr.lift_pairs_subpix(corrs[p, :n], offsets[p, :n], LIFT_FEAT, depth_a[p], depth_q[p], cam_a[p], cam[p], JUMP_MM)
            for p, n in enumerate(LIFT_COUNTS)]
    out = dict(corrs=corrs, offsets=offsets, n_corr=np.array(LIFT_COUNTS, np.int32), depth_a=depth_a, depth_q=depth_q, cam_a=cam_a, cam_q=cam,
               want=want)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def lift_conditions(case):
    """The special rows do what they were planted for, and both branches are taken on both sides."""
    S = LIFT_SPECIAL
    for p, n in enumerate(LIFT_COUNTS):
        if n == 0:
            continue
        pa, pq, keep, bil_a, bil_q = case["want"][p]
        for name in ("out_right", "out_negative", "nan_offset"):
            assert not keep[S[name]], (p, name)
        at = np.cumsum(keep) - 1                                       # compacted position of every kept row
        for name, taken in (("last_row_col", False), ("hole", False), ("jump_under", True), ("jump_over", False)):
            assert keep[S[name]] and bool(bil_q[at[S[name]]]) == taken, (p, name)
        assert bil_a.any() and (~bil_a).any() and bil_q.sum() > 10 and (~bil_q).sum() >= 3
        assert keep.sum() < n and len(pa) == keep.sum()
    return True
