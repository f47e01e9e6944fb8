"""Hand-over work folded into the neighbouring kernels (csrc/match_corrs.hip, screen_mx6.hip, post.hip, roi.hip, gather8.hip, engine.hip):
  - the cascades' probe, open-row and sampled-row screens read their rows in place through the list (match_mx6_screen_w4_list_kernel;
    no compaction launch),
  - the open rows of the default route's cascade are merged by match_decide_lite_kernel from the slot match_dc_settle_rows_kernel left
    them (no scatter launch),
  - the second level's list of the sampled ambiguous rows is built by select_corrs_kernel and by match_decide_sampled_kernel
    (list_sampled_amb, match_common.h; no list launch),
  - the engine compacts both mask sets with one roi_compact launch whose workgroups also clear the error norms of the two gathers behind
    it (the gathers run without a fill of their own).
Nothing of this may change a result: the matcher through `ops` against the C oracle's exact fp32 scan and the restated draw, the engine
with the cascade against the plain full screen (knob 0) bit for bit, the cascade's counters against what the generator's geometry says.

Shape: 48 x 64 maps (HW = 3072 = cap_a, three 1024-row panels: the cascade's shape gate), C = 256, B = 3, 500 correspondences, 1500 query
rows (12 tiles, the last one partial).  Anchor row i matches query row i // 4 where it has a counterpart: a panel's matches span two
tiles, its band (two tiles of slack at either end) at most six - half of the pair's tiles, the widest a learned band may be."""
import numpy as np
import pytest
import torch

from test_gpu_match_chain import OK, NO_MASK, keys_np, smallest_in_order

pytestmark = pytest.mark.gpu

FH, FW, C = 48, 64, 256
HW = FH * FW
N_Q = 1500
MAX_CORRS, CORR_ROWS, THR, STRIDE = 500, 512, 0.25, 10
SEED = 1                            # MatchPoseConfig's: the engine and the `ops` call draw the same rows
_cache = {}


def _local_pair(index, n_a, share):
    """Anchor rows = the first n_a pixels, query rows = the first N_Q.  A random `share` of the anchors (every probe row of the cascade
    among them: rows 0, 10, 20, ..) carries the descriptor of query row i // 4 plus 5 % noise; the others are independent Gaussians -
    no counterpart (their best cosine over 1500 queries stays below 6 sigma = 0.375 < 0.5).  -> pair dict and `has` [n_a]."""
    from oryon_amd.synth import intrinsics
    g = torch.Generator(device="cpu")
    g.manual_seed(4200 + index)
    fq = torch.randn(C, HW, generator=g)
    fa = torch.randn(C, HW, generator=g)
    rows = torch.arange(n_a)
    has = (torch.rand(n_a, generator=g) < share) | (rows % STRIDE == 0)
    fa[:, rows[has]] = fq[:, rows[has] // 4] + 0.05 * torch.randn(C, int(has.sum()), generator=g)
    mask_a, mask_q = torch.zeros(HW, dtype=torch.int32), torch.zeros(HW, dtype=torch.int32)
    mask_a[:n_a] = 1
    mask_q[:N_Q] = 1
    yy, xx = torch.meshgrid(torch.arange(FH, dtype=torch.float32), torch.arange(FW, dtype=torch.float32), indexing="ij")
    depth = 800.0 + 60.0 * torch.sin(xx / 9.0) + 40.0 * torch.cos(yy / 7.0)
    dev = "cuda"
    pair = dict(feat_a=fa.view(C, FH, FW).to(dev), feat_q=fq.view(C, FH, FW).to(dev), mask_a=mask_a.view(FH, FW).to(dev),
                mask_q=mask_q.view(FH, FW).to(dev), depth_a=depth.to(dev), depth_q=depth.clone().to(dev), camera=intrinsics(FH, FW))
    return pair, has.numpy()


def _case(name):
    """-> (pairs, has per pair, pair keys)"""
    if name not in _cache:
        if name == "mixed":
            # 3000 anchors, ~40 % without a counterpart (more than two 512-row panels of open rows); 2100 anchors, every one with a
            # counterpart (no open row); an empty anchor mask
            made = [_local_pair(0, 3000, 0.6), _local_pair(1, 2100, 1.0), _local_pair(2, 2500, 0.8)]
            made[2][0]["mask_a"] = torch.zeros_like(made[2][0]["mask_a"])
            made[2] = (made[2][0], np.zeros(0, bool))
        elif name == "few_valid":
            # fewer valid rows than correspondences asked for: the draw is with replacement, rows repeat in sel_rows
            made = [_local_pair(10, 2200, 0.05), _local_pair(11, 3000, 0.02), _local_pair(12, 2100, 1.0)]
        else:
            raise KeyError(name)
        _cache[name] = ([m[0] for m in made], [m[1] for m in made], [4200 + 17 * i for i in range(len(made))])
    return _cache[name]


def _smooth_case():
    if "smooth" not in _cache:
        from oryon_amd.synth import make_pair
        _cache["smooth"] = ([make_pair(700, 96, 96, C, device="cuda", smooth=0.02), make_pair(701, 96, 96, C, device="cuda", smooth=0.02),
                             make_pair(902, 96, 96, C, device="cuda")], None, [700, 701, 902])
    return _cache["smooth"]


def _ops_match(pairs, keys):
    """oryon_match_corrs_mx6_araw (cascade on, by shape) on K0's operands of these pairs"""
    from oryon_amd import ops
    st = lambda k: torch.stack([p[k] for p in pairs]).contiguous()
    fa, fq = st("feat_a"), st("feat_q")
    W = fa.shape[-1]
    roi_a, na = ops.roi_compact(st("mask_a"))
    roi_q, nq = ops.roi_compact(st("mask_q"))
    cap_a, cap_q = ops.round_up(int(na.max()), 256), ops.round_up(int(nq.max()), 256)
    assert cap_a > 2048, "the cascade's shape gate"
    a6, a_err, a_norm, _ = ops.gather_mx6(fa, roi_a, na, cap_a, C)
    q6, q_err, q_norm, _ = ops.gather_mx6(fq, roi_q, nq, cap_q, C)
    und = torch.full((len(pairs),), -7, dtype=torch.int32, device="cuda")
    key = torch.tensor(keys, dtype=torch.int64, device="cuda")
    out = ops.match_corrs_mx6_araw(fa, a_norm, a6, a_err, fq, roi_a, roi_q, q_norm, q6, q_err, na, nq, THR, W, MAX_CORRS, SEED, key, CORR_ROWS, und)
    torch.cuda.synchronize()
    r = dict(zip(("corrs", "n_valid", "n_sel", "status", "min_dist", "argmin", "valid"), (o.cpu().numpy() for o in out)))
    r.update(n_a=na.cpu().numpy(), n_q=nq.cpu().numpy(), roi_a=roi_a.cpu().numpy(), roi_q=roi_q.cpu().numpy(), W=W, cap_a=cap_a,
             a_err=a_err.cpu().numpy(), q_err=q_err.cpu().numpy())
    return r


def _against_oracle(r, pairs, keys):
    """valid, n_valid, n_sel, status, the sampled rows (restated draw on the oracle's valid set), their argmin and query pixels"""
    from oracle import c_oracle
    W = r["W"]
    for b, p in enumerate(pairs):
        n_a, n_q = int(r["n_a"][b]), int(r["n_q"][b])
        if n_a == 0 or n_q == 0:
            assert r["status"][b] == NO_MASK and r["n_valid"][b] == 0 and r["n_sel"][b] == 0
            continue
        roi_a, roi_q = r["roi_a"][b, :n_a], r["roi_q"][b, :n_q]
        _, am, va = c_oracle.match_lin(p["feat_a"].cpu().numpy(), p["feat_q"].cpu().numpy(), roi_a, roi_q, THR)
        va = va.astype(bool)
        assert np.array_equal(r["valid"][b, :n_a].astype(bool), va), f"pair {b}: valid set differs from the C oracle"
        rows = np.nonzero(va)[0]
        nv = len(rows)
        assert int(r["n_valid"][b]) == nv and nv > 1 and r["status"][b] == OK and r["n_sel"][b] == MAX_CORRS
        if nv < MAX_CORRS:
            pick = (keys_np(SEED, keys[b], 2, MAX_CORRS).astype(np.uint64) * np.uint64(nv)) >> np.uint64(32)
            sel = rows[pick.astype(np.int64)]
            assert len(np.unique(sel)) < len(sel), "this pair was to draw rows more than once"
        else:
            sel = rows[smallest_in_order(keys_np(SEED, keys[b], 1, nv), MAX_CORRS)]
        assert np.array_equal(r["argmin"][b, sel], am[sel]), f"pair {b}: argmin of a sampled row differs from the C oracle"
        pa, pq = roi_a[sel], roi_q[am[sel]]
        want = np.stack([pa // W, pa % W, pq // W, pq % W], 1)
        assert np.array_equal(r["corrs"][b, :MAX_CORRS], want), f"pair {b}: corrs differ from (oracle valid set, restated draw, oracle argmin)"


def _solver():
    from oracle import oryon_oracle as orc
    from oryon_amd.pointdsc import PointDSC
    m = PointDSC(in_dim=6, num_layers=2, num_channels=32, num_iterations=10, ratio=0.1, sigma_d=0.1, k=40, nms_radius=0.1)
    m.load_state_dict(orc.analytic_pointdsc_params(2, 32), strict=True)
    return m.cuda().eval()


def _engine(knob):
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    eng = MatchPoseEngine(_solver(), MatchPoseConfig(), overlap_registration=True, overlap_gather=True, native=True, result_views=True)
    eng.native_geometry["screen_cascade"] = knob
    eng.native_geometry["x3_prefetch"] = 0                        # every step stays on the default route
    return eng


def _engine_inputs(pairs):
    st = lambda k: torch.stack([p[k] for p in pairs]).contiguous()
    cam = st("camera").reshape(len(pairs), 9).float().cuda().contiguous()
    return [st("feat_a"), st("feat_q"), st("mask_a"), st("mask_q"), st("depth_a"), st("depth_q"), cam, cam]


def _step(eng, ins, keys):
    """one step -> the slot's outputs as numpy (bit patterns for the floats: a pose of a degenerate pair may hold NaNs)"""
    o = eng.run(*ins, torch.tensor(keys, dtype=torch.int64, device="cuda"))
    slot = o["_native_slot"]
    eng.finish(o)
    torch.cuda.synchronize()
    nat = eng._native
    r = {k: nat.view(slot, k).cpu().numpy().copy() for k in ("n_a", "n_q", "valid", "corrs", "n_valid", "n_sel", "status", "n_und", "min_dist",
                                                             "status_out", "n_lift")}
    r["pose_bits"] = o["pose"].cpu().numpy().view(np.uint32).copy()
    r["stats"] = nat.cascade_stats().numpy().copy()                # [B, 4]: probe, settled, open, band tiles
    return r


def _same_step(x, y, what):
    for b in range(len(x["n_a"])):
        n, ns = int(x["n_a"][b]), int(x["n_sel"][b])
        for k in ("n_a", "n_q", "n_valid", "n_sel", "status", "status_out", "n_lift"):
            assert x[k][b] == y[k][b], (what, b, k, x[k][b], y[k][b])
        assert np.array_equal(x["corrs"][b, :ns], y["corrs"][b, :ns]), (what, b, "corrs")
        assert np.array_equal(x["valid"][b, :n], y["valid"][b, :n]), (what, b, "valid")
        assert np.array_equal(x["pose_bits"][b], y["pose_bits"][b]), (what, b, "pose")


def _engine_equals_ops(e, r):
    for b in range(len(r["n_a"])):
        n, ns = int(r["n_a"][b]), int(r["n_sel"][b])
        assert e["n_valid"][b] == r["n_valid"][b] and e["n_sel"][b] == ns and e["status"][b] == r["status"][b], (b, "engine against ops")
        assert np.array_equal(e["valid"][b, :n], r["valid"][b, :n]) and np.array_equal(e["corrs"][b, :ns], r["corrs"][b, :ns]), (b, "engine against ops")


def _knob_0_and_1(pairs, keys, steps=2):
    ins = _engine_inputs(pairs)
    e0, e1 = _engine(0), _engine(1)
    last = None
    for i in range(steps):
        r0, r1 = _step(e0, ins, keys), _step(e1, ins, keys)
        _same_step(r0, r1, f"step {i}, plain screen against cascade")
        assert not r0["stats"].any(), "knob 0 took the cascade"
        last = r1
    del e0, e1
    return last


def test_mixed_batch_open_rows_in_several_panels_none_and_an_empty_mask():
    pairs, has, keys = _case("mixed")
    r = _ops_match(pairs, keys)
    assert r["cap_a"] == 3072 and r["n_a"].tolist() == [3000, 2100, 0] and r["n_q"].tolist() == [N_Q] * 3
    _against_oracle(r, pairs, keys)
    for b in (0, 1):
        assert np.array_equal(r["valid"][b, :len(has[b])].astype(bool), has[b]), "the generator's geometry is the valid set"
    e = _knob_0_and_1(pairs, keys)
    _engine_equals_ops(e, r)
    s = e["stats"]
    print("stats (probe, settled, open, band tiles):", s.tolist())
    # pair 0: three panels with learned bands - every row that is no probe row settles (counterpart) or stays open (none)
    probe0 = np.arange(3000) % STRIDE == 0
    assert s[0].tolist()[:3] == [300, int((has[0] & ~probe0).sum()), int((~has[0]).sum())]
    assert s[0, 2] > 1024 and s[0, 2] % 32 != 0, "more than two 512-row panels of open rows, the last one ragged"
    assert s[0, 3] <= 4 + 6 + 6
    # pair 1: no open row; its last panel (52 rows, 5 probe rows) scans all tiles, the first two settle their rows
    probe1 = np.arange(2100) % STRIDE == 0
    assert s[1].tolist()[:3] == [210, int((~probe1[:2048]).sum()), 0]
    assert not s[2].any(), "a pair without anchors"


def test_fewer_valid_rows_than_correspondences_draws_rows_twice():
    pairs, has, keys = _case("few_valid")
    r = _ops_match(pairs, keys)
    nv = r["n_valid"].tolist()
    assert 1 < nv[0] < MAX_CORRS and 1 < nv[1] < MAX_CORRS and nv[2] == 2100, nv
    _against_oracle(r, pairs, keys)
    e = _knob_0_and_1(pairs, keys)
    _engine_equals_ops(e, r)
    s = e["stats"]
    print("stats (probe, settled, open, band tiles):", s.tolist())
    for b in (0, 1):
        probe = np.arange(len(has[b])) % STRIDE == 0
        assert s[b].tolist()[:3] == [int(probe.sum()), int((has[b] & ~probe).sum()), int((~has[b]).sum())]


def test_smooth_fields_feed_the_second_level_from_the_folded_lists():
    pairs, _, keys = _smooth_case()
    r = _ops_match(pairs, keys)
    _against_oracle(r, pairs, keys)
    e = _knob_0_and_1(pairs, keys, steps=3)
    _engine_equals_ops(e, r)
    print("n_undecided", e["n_und"].tolist(), "stats", e["stats"].tolist())
    assert (e["n_und"][:2] > 0).all(), "the smooth pairs keep ambiguous sampled rows after the complete pass: the second level ran for them"
    assert (e["stats"][:, 0] > 0).all()


# ------------------------------------------------------------------------------------------------------------------ roi_compact
@pytest.mark.parametrize("H,W", [(71, 71), (52, 97), (224, 224), (300, 300)])
def test_roi_compact_counts_at_and_around_the_sampling_size(H, W):
    """0 pixels, exactly src_sampling = 5000, more, all; H x W with a last partial group of eight (71 x 71: no 16-byte loads at all;
    52 x 97: HW % 8 = 4), the benchmark's map (7 scan steps behind one barrier pair) and one beyond a group of eight steps (65536)"""
    from oracle import c_oracle
    from oryon_amd import ops
    g = np.random.default_rng(H * 1000 + W)
    n = H * W
    masks = np.zeros((6, n), np.int32)
    masks[1, g.choice(n, 5000, replace=False)] = 1
    masks[2, g.choice(n, 5001, replace=False)] = 1
    masks[3] = g.integers(0, 3, n)                       # values other than 0 / 1 are not ROI pixels
    masks[4] = 1
    masks[5, -3:] = 1                                    # only the ragged tail
    roi, cnt = ops.roi_compact(torch.from_numpy(masks.reshape(6, H, W)).cuda())
    roi, cnt = roi.cpu().numpy(), cnt.cpu().numpy()
    for m in range(6):
        want = c_oracle.roi_from_mask(masks[m].reshape(H, W))
        assert cnt[m] == len(want), (m, cnt[m], len(want))
        assert np.array_equal(roi[m, :cnt[m]], want), m
    assert cnt[:3].tolist() == [0, 5000, 5001]


# ------------------------------------------------------------------------------------------------------------------ K0's error norms
def _gather_set_words(nat, B, x3_prefetch=0):
    """byte offsets of (a_eps, q_eps) of every gather set in the engine's arena: the order of carve_engine (csrc/engine.hip), checked
    against the first named slot buffer, which follows the last set"""
    import ctypes
    from oryon_amd._lib import lib
    ca, cq, cp, nc = (ctypes.c_int() for _ in range(4))
    assert lib().oryon_engine_geometry(nat._h, ctypes.byref(ca), ctypes.byref(cq), ctypes.byref(cp), ctypes.byref(nc)) == 0
    cap_a, cap_q, c_pad = ca.value, cq.value, cp.value
    up = lambda v: (v + 255) // 256 * 256
    sizes = [B * cap_a * c_pad, B * cap_q * c_pad, B * (cap_a // 16) * 4, B * (cap_q // 16) * 4, B * 4, B * 4, B * cap_a * 4, B * cap_q * 4,
             B * cap_a * c_pad * 4]
    if x3_prefetch:
        sizes += [2 * B * cap_q * c_pad * 2, B * 4]
    offs, off = [], 0
    for _ in range(2):                                   # gather_sets
        o = [0] * len(sizes)
        for i, n in enumerate(sizes):
            o[i] = off
            off = up(off + n)
        offs.append((o[4], o[5]))
    first, nbytes = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib().oryon_engine_buffer(nat._h, 0, b"roi_a", ctypes.byref(first), ctypes.byref(nbytes)) == 0
    assert first.value == off, "the gather sets' layout is not what this test assumes"
    return offs


def test_engine_gathers_start_from_cleared_error_norms():
    """The engine's gathers raise their per-map error norms with atomic maxima from the zero its roi_compact launch stored: after two
    steps on heavy-tailed maps (larger norms, left in both gather sets) a step on Gaussian pairs must report the norms - and everything
    else - of the same step on a fresh engine, which are those of the public gather (it fills for itself)."""
    from oryon_amd import ops
    pairs, _, keys = _case("mixed")
    pairs = [pairs[0], pairs[1], _local_pair(3, 2500, 0.8)[0]]
    other = [dict(p) for p in pairs]
    for p in other:
        p["feat_a"], p["feat_q"] = p["feat_a"] ** 3, p["feat_q"] ** 3
    X, Y = _engine_inputs(pairs), _engine_inputs(other)
    fresh = _engine(1)
    r_fresh = _step(fresh, X, keys)
    words = _gather_set_words(fresh._native, 3)

    def norms(eng, s):
        a = eng._native.arena
        torch.cuda.synchronize()
        return [a[o:o + 12].view(torch.float32).cpu().numpy().copy() for o in words[s]]

    roi_a, na = ops.roi_compact(X[2])
    roi_q, nq = ops.roi_compact(X[3])
    want_a = ops.gather_mx6(X[0], roi_a, na, 3072, C)[1].cpu().numpy()
    want_q = ops.gather_mx6(X[1], roi_q, nq, 3072, C)[1].cpu().numpy()
    got_a, got_q = norms(fresh, 0)
    assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32)) and np.array_equal(got_q.view(np.uint32), want_q.view(np.uint32))
    del fresh
    used = _engine(1)
    _step(used, Y, keys)
    _step(used, Y, keys)
    for s in (0, 1):
        ya, yq = norms(used, s)
        assert (ya > want_a).all() and (yq > want_q).all(), "the other pairs were to leave LARGER norms behind"
    r_used = _step(used, X, keys)                        # third step: gather set 0 again
    got_a, got_q = norms(used, 0)
    assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32)), (got_a, want_a)
    assert np.array_equal(got_q.view(np.uint32), want_q.view(np.uint32)), (got_q, want_q)
    _same_step(r_fresh, r_used, "fresh engine against one that had matched other pairs")
    assert np.array_equal(r_fresh["n_und"], r_used["n_und"]) and np.array_equal(r_fresh["stats"], r_used["stats"])
    for b in range(3):
        n = int(r_fresh["n_a"][b])
        assert np.array_equal(r_fresh["min_dist"][b, :n].view(np.uint32), r_used["min_dist"][b, :n].view(np.uint32)), (b, "min_dist")
    del used
