"""The default route's validity cascade (oryon_engine_config_t.screen_cascade, csrc/match_corrs.hip match_dc_*): a probe of the anchors
screened completely, a learned band of query tiles per 1024-anchor panel, the other anchors settled inside the band, a complete scan only
for the anchors left open and for the sampled ones.  Every result must be BIT FOR BIT that of the plain full screen (knob 0) over
several steps - poses, statuses, counts, correspondences - and, where noted, what the C oracle's exact fp32 scan gives.  Every test
asserts through oryon_engine_cascade_stats that the path it is about really ran.

Shape: 96 x 96 maps (2304 anchors of the centred mask = 3 live panels, ~61 query tiles), C = 256, 3-4 pairs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 96
STRIDE = 10                 # the probe stride at cap_a = 5120 (dc_probe_stride)
KEYS = ("pose", "status", "n_valid", "n_lifted")


def _solver():
    from oracle import oryon_oracle as orc
    from oryon_amd.pointdsc import PointDSC
    m = PointDSC(in_dim=6, num_layers=2, num_channels=32, num_iterations=10, ratio=0.1, sigma_d=0.1, k=40, nms_radius=0.1)
    m.load_state_dict(orc.analytic_pointdsc_params(2, 32), strict=True)
    return m.cuda().eval()


def _stack(pairs, nhwc=False):
    st = lambda k: torch.stack([p[k] for p in pairs]).contiguous()
    B = len(pairs)
    cam = st("camera").reshape(B, 9).float().cuda().contiguous()
    fa, fq = st("feat_a"), st("feat_q")
    if nhwc:
        fa, fq = fa.contiguous(memory_format=torch.channels_last), fq.contiguous(memory_format=torch.channels_last)
    return [fa, fq, st("mask_a"), st("mask_q"), st("depth_a"), st("depth_q"), cam, cam]


def _run(ins, knob, steps=3, first_key=0, x3_prefetch=0):
    """`steps` steps of the native engine with the knob; per step the compared outputs, the live correspondence rows, the slot's
    valid flags / ROI lists and the cascade's counters."""
    from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine
    B = ins[0].shape[0]
    key = torch.arange(first_key, first_key + B, dtype=torch.int64, device="cuda")
    eng = MatchPoseEngine(_solver(), MatchPoseConfig(), overlap_registration=True, overlap_gather=True, native=True, result_views=True)
    eng.native_geometry["screen_cascade"] = knob
    eng.native_geometry["x3_prefetch"] = x3_prefetch
    res = []
    for _ in range(steps):
        o = eng.run(*ins, key)
        slot = o["_native_slot"]
        eng.finish(o)
        torch.cuda.synchronize()
        nat = eng._native
        r = {k: o[k].clone() for k in KEYS}
        n_sel = nat.view(slot, "n_sel").cpu()
        corrs = nat.view(slot, "corrs").cpu()
        r["corrs"] = [corrs[b, :int(n_sel[b])].clone() for b in range(B)]
        r["n_sel"] = n_sel.clone()
        for k in ("valid", "roi_a", "roi_q", "n_a", "n_q"):
            r[k] = nat.view(slot, k).cpu().numpy().copy()
        r["stats"] = nat.cascade_stats().numpy().copy()              # [B, 4]: probe, settled, open, band tiles
        r["x3_steps"] = nat.x3_steps()
        res.append(r)
    del eng
    return res


def _assert_equal(r0, r1):
    assert len(r0) == len(r1)
    for i, (a, b) in enumerate(zip(r0, r1)):
        for k in KEYS + ("n_sel",):
            assert torch.equal(a[k], b[k]), (i, k)
        for p, (ca, cb) in enumerate(zip(a["corrs"], b["corrs"])):
            assert torch.equal(ca, cb), (i, p, "corrs")
        assert not a["stats"].any(), "knob 0 took the cascade"


def _live_panels(n_a):
    return (int(n_a) + 1023) // 1024


def _vs_oracle(r, pairs_np):
    """valid of every anchor row, n_valid and the query pixel of every sampled correspondence against the C oracle's exact scan"""
    from oracle import c_oracle
    for b, (fa, fq) in enumerate(pairs_np):
        n_a, n_q = int(r["n_a"][b]), int(r["n_q"][b])
        roi_a, roi_q = r["roi_a"][b, :n_a], r["roi_q"][b, :n_q]
        md, am, va = c_oracle.match_lin(fa, fq, roi_a, roi_q, 0.25)
        assert np.array_equal(r["valid"][b, :n_a].astype(bool), va), f"pair {b}: valid set differs from the C oracle"
        assert int(r["n_valid"][b]) == int(va.sum())
        corrs = r["corrs"][b].numpy().astype(np.int64)
        row = np.searchsorted(roi_a, corrs[:, 0] * H + corrs[:, 1])
        assert va[row].all()
        assert np.array_equal(corrs[:, 2] * H + corrs[:, 3], roi_q[am[row]]), f"pair {b}: a sampled query pixel is not the oracle's argmin"
    return md, am, va, row


def _np_pairs(ins):
    return [(ins[0][b].cpu().numpy(), ins[1][b].cpu().numpy()) for b in range(ins[0].shape[0])]


def test_gaussian_pairs_settle_some_rows_and_leave_some_open():
    from oryon_amd.synth import make_pair
    ins = _stack([make_pair(900 + i, H, H, 256, device="cuda") for i in range(3)])
    r0, r1 = _run(ins, 0, first_key=900), _run(ins, 1, first_key=900)
    _assert_equal(r0, r1)
    for r in r1:
        s = r["stats"]
        print("stats (probe, settled, open, band tiles):", s.tolist(), "n_a", r["n_a"].tolist(), "n_q", r["n_q"].tolist())
        assert (s[:, 0] == (r["n_a"] + STRIDE - 1) // STRIDE).all()
        assert (s[:, 1] > 0).all() and (s[:, 2] > 0).all(), s
        assert (s[:, 0] + s[:, 1] + s[:, 2] <= r["n_a"]).all()
    assert r1[0]["status"].tolist() == [0, 0, 0]
    _vs_oracle(r1[-1], _np_pairs(ins))


@pytest.mark.parametrize("C,nhwc", [(32, False), (96, False), (96, True)])
def test_narrow_maps_and_channels_last(C, nhwc):
    """the KL = 1 / KL = 2 variants of both screen kernels (8-wave band pass, 4-wave probe / open / sampled passes)"""
    from oryon_amd.synth import make_pair
    ins = _stack([make_pair(910 + C + i, H, H, C, device="cuda") for i in range(3)], nhwc=nhwc)
    r0, r1 = _run(ins, 0, steps=2, first_key=910), _run(ins, 1, steps=2, first_key=910)
    _assert_equal(r0, r1)
    for r in r1:
        assert (r["stats"][:, 0] > 0).all() and (r["stats"][:, 3] > 0).all(), r["stats"]


def test_more_than_one_compact_panel_of_open_rows():
    """mask_q without its lower half: the anchors that match there have no counterpart left, stay open and fill more than one panel of
    the complete scan (more than 1024 rows).  This one case runs at 160 x 160 (5000 sampled anchors = 5 panels): at 96 x 96 a half-cleared
    query map has ~31 tiles, the matches of a 1024-anchor panel span more than half of them for every pair and cut (searched on the
    CPU), and such a band is "all tiles" by the very cap the rotated case below relies on.  Pair 963 is chosen on the CPU from the
    generator's geometry alone: the cut runs through the matches of three panels that keep enough valid probe rows to learn a band."""
    from oryon_amd.synth import _pair_geometry, make_pair
    HB = 160
    pairs = [make_pair(920, HB, HB, 256, device="cuda"), make_pair(963, HB, HB, 256, device="cuda"), make_pair(922, HB, HB, 256, device="cuda")]
    pairs[1]["mask_q"] = pairs[1]["mask_q"].clone()
    pairs[1]["mask_q"][HB // 2:] = 0
    ins = _stack(pairs)
    r0, r1 = _run(ins, 0, steps=2, first_key=920), _run(ins, 1, steps=2, first_key=920)
    _assert_equal(r0, r1)
    r = r1[-1]
    n_a = int(r["n_a"][1])
    assert n_a == 5000
    # the CPU's count, from the geometry: an anchor has a counterpart iff its re-projection owns a query pixel that survived the cut
    winner, hit = _pair_geometry(963, HB, HB)[5:7]
    tgt = torch.full((HB * HB,), -1, dtype=torch.long)
    tgt[winner[hit]] = torch.arange(HB * HB)[hit]
    ta = tgt[torch.from_numpy(r["roi_a"][1, :n_a]).long()]
    has = ((ta >= 0) & (pairs[1]["mask_q"].cpu().view(-1)[ta.clamp(min=0)] != 0)).numpy()
    stride = 10
    need_open = 0
    for a0 in range(0, n_a, 1024):
        rows = np.arange(a0, min(a0 + 1024, n_a))
        probe = rows[rows % stride == 0]
        if has[probe].sum() >= 8:                                    # enough valid probe rows to learn a band (DC_MIN_SURE)
            need_open += int((~has[rows]).sum() - (~has[probe]).sum())
    print("open rows expected from the geometry", need_open, "stats", r["stats"][1].tolist())
    assert need_open > 1024, need_open
    assert int(r["stats"][1, 2]) > 1024 and int(r["stats"][1, 1]) > 0, r["stats"][1]
    assert (r["valid"][1, :n_a].astype(bool) == has).mean() > 0.999


def test_empty_and_short_pairs_beside_full_ones():
    from oryon_amd.synth import make_pair
    pairs = [make_pair(930 + i, H, H, 256, device="cuda") for i in range(4)]
    for i in (0, 1, 2):
        pairs[i]["mask_q" if i == 0 else "mask_a"] = pairs[i]["mask_q" if i == 0 else "mask_a"].clone()
    pairs[0]["mask_q"][:] = 0                                            # no query pixel at all
    live = pairs[1]["mask_a"].view(-1).nonzero().flatten()
    pairs[1]["mask_a"].view(-1)[live[STRIDE - 3:]] = 0                   # fewer anchors than the probe stride
    live = pairs[2]["mask_a"].view(-1).nonzero().flatten()
    pairs[2]["mask_a"].view(-1)[live[700:]] = 0                          # fewer than one panel
    ins = _stack(pairs)
    r0, r1 = _run(ins, 0, steps=2, first_key=930), _run(ins, 1, steps=2, first_key=930)
    _assert_equal(r0, r1)
    r = r1[-1]
    assert r["n_a"].tolist()[1:3] == [STRIDE - 3, 700] and int(r["n_q"][0]) == 0
    assert r["stats"][:, 0].tolist() == [(int(n) + STRIDE - 1) // STRIDE for n in r["n_a"]]
    assert int(r["stats"][3, 1]) > 0                                     # the full pair settled rows in its bands
    assert int(r["status"][3]) == 0 and int(r["status"][0]) != 0


def test_rotated_query_maps_defeat_the_locality_and_scan_all_tiles():
    from oryon_amd.synth import make_pair
    pairs = [make_pair(940 + i, H, H, 256, device="cuda") for i in range(3)]
    for p in pairs:
        for k in ("feat_q", "mask_q", "depth_q"):
            p[k] = torch.rot90(p[k], 1, (-2, -1)).contiguous()
    ins = _stack(pairs)
    r0, r1 = _run(ins, 0, steps=2, first_key=940), _run(ins, 1, steps=2, first_key=940)
    _assert_equal(r0, r1)
    for r in r1:
        for b in range(3):
            nqt = (int(r["n_q"][b]) + 127) // 128
            assert int(r["stats"][b, 3]) == _live_panels(r["n_a"][b]) * nqt, (b, r["stats"][b], nqt)      # every band is "all tiles"
            assert int(r["stats"][b, 1]) == 0 and int(r["stats"][b, 2]) == 0
    assert (r1[-1]["n_valid"] > 0).all()


def test_an_equal_match_outside_the_band_wins_by_first_index():
    """The descriptors of the true matches of 120 anchors of the LAST panel (no probe rows among them) are copied onto query pixels of the
    first tile, far above that panel's band: the anchors settle on their witness inside the band, the oracle's argmin (first index) is
    the copy, and every sampled one of them must carry the copy's pixel."""
    from oracle import c_oracle
    from oryon_amd.synth import make_pair
    pairs = [make_pair(950 + i, H, H, 256, device="cuda") for i in range(3)]
    base = _run(_stack(pairs), 1, steps=1, first_key=950)[0]
    b = 1
    n_a, n_q = int(base["n_a"][b]), int(base["n_q"][b])
    roi_a, roi_q = base["roi_a"][b, :n_a], base["roi_q"][b, :n_q]
    fa, fq = _np_pairs(_stack(pairs))[b]
    _, am, va = c_oracle.match_lin(fa, fq, roi_a, roi_q, 0.25)
    rows = [a for a in range(n_a - 400, n_a) if a % STRIDE and va[a] and am[a] >= 16 * 128][:120]
    assert len(rows) == 120
    fq_t = pairs[b]["feat_q"].clone().view(256, -1)
    for i, a in enumerate(rows):
        fq_t[:, int(roi_q[i])] = fq_t[:, int(roi_q[am[a]])]              # query rows 0 .. 119: tile 0
    pairs[b]["feat_q"] = fq_t.view(256, H, H)
    ins = _stack(pairs)
    r0, r1 = _run(ins, 0, steps=2, first_key=950), _run(ins, 1, steps=2, first_key=950)
    _assert_equal(r0, r1)
    r = r1[-1]
    nqt = (n_q + 127) // 128
    assert int(r["stats"][b, 3]) < _live_panels(n_a) * nqt and int(r["stats"][b, 1]) > 0      # learned bands, settled rows
    _vs_oracle(r, _np_pairs(ins))
    fa, fq = _np_pairs(ins)[b]
    _, am2, _ = c_oracle.match_lin(fa, fq, roi_a, roi_q, 0.25)
    corrs = r["corrs"][b].numpy().astype(np.int64)
    srow = np.searchsorted(roi_a, corrs[:, 0] * H + corrs[:, 1])
    hit = 0
    for i, a in enumerate(rows):
        assert int(am2[a]) == i                                           # the oracle's argmin is the copy (first index)
        for s in np.nonzero(srow == a)[0]:
            assert corrs[s, 2] * H + corrs[s, 3] == int(roi_q[i])
            hit += 1
    assert hit > 0, "none of the 120 anchors was sampled"


def test_threshold_edge_on_either_side():
    """One query descriptor per side blended so that its cosine with its anchor is 0.5 -+ 0.004 (1 - 2 thr = 0.5; the screen's delta is
    ~0.04): the bound cannot settle those anchors, they stay open, are scanned completely and resolved exactly - n_valid is the oracle's."""
    from oracle import c_oracle
    from oryon_amd.synth import make_pair
    pairs = [make_pair(960 + i, H, H, 256, device="cuda") for i in range(3)]
    base = _run(_stack(pairs), 1, steps=1, first_key=960)[0]
    b = 2
    n_a, n_q = int(base["n_a"][b]), int(base["n_q"][b])
    roi_a, roi_q = base["roi_a"][b, :n_a], base["roi_q"][b, :n_q]
    fa, fq = _np_pairs(_stack(pairs))[b]
    _, am, va = c_oracle.match_lin(fa, fq, roi_a, roi_q, 0.25)
    rows = [a for a in range(1100, n_a) if a % STRIDE and va[a]][:2]
    fa_t, fq_t = pairs[b]["feat_a"].view(256, -1), pairs[b]["feat_q"].clone().view(256, -1)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    for a, c in zip(rows, (0.504, 0.496)):
        x = fa_t[:, int(roi_a[a])].double()
        x = x / x.norm()
        u = torch.randn(256, generator=g, device="cuda").double()
        u = u - (u @ x) * x
        u = u / u.norm()
        fq_t[:, int(roi_q[am[a]])] = (3.0 * (c * x + (1.0 - c * c) ** 0.5 * u)).float()
    pairs[b]["feat_q"] = fq_t.view(256, H, H)
    ins = _stack(pairs)
    r0, r1 = _run(ins, 0, steps=2, first_key=960), _run(ins, 1, steps=2, first_key=960)
    _assert_equal(r0, r1)
    r = r1[-1]
    assert int(r["stats"][b, 1]) > 0 and int(r["stats"][b, 2]) >= 2
    _vs_oracle(r, _np_pairs(ins))
    fa, fq = _np_pairs(ins)[b]
    _, _, va2 = c_oracle.match_lin(fa, fq, roi_a, roi_q, 0.25)
    assert bool(va2[rows[0]]) and not bool(va2[rows[1]])                  # one on each side of the threshold
    assert r["valid"][b, rows[0]] == 1 and r["valid"][b, rows[1]] == 0


def test_smooth_pairs_still_switch_to_the_hard_route():
    """Smooth fields: the first steps take the new route (every settled row counts as ambiguous, and the complete pass leaves the sampled
    ones ambiguous: the feedback says "hard"), later steps the hard route; every step's outputs equal the plain screen's."""
    from oryon_amd.synth import make_pair
    pairs = [make_pair(700, H, H, 256, device="cuda", smooth=0.02), make_pair(701, H, H, 256, device="cuda", smooth=0.02),
             make_pair(702, H, H, 256, device="cuda")]
    ins = _stack(pairs)
    r0, r1 = _run(ins, 0, steps=6, x3_prefetch=1), _run(ins, 1, steps=6, x3_prefetch=1)
    _assert_equal(r0, r1)
    assert (r1[0]["stats"][:, 0] > 0).all(), "the first step did not take the cascade"
    assert r1[-1]["x3_steps"] >= 4 and r0[-1]["x3_steps"] >= 4
    assert not r1[-1]["stats"].any()                                      # the hard route has its own cascade
    assert r1[0]["status"].tolist() == [0, 0, 0]


def test_gaussian_pairs_do_not_switch_to_the_hard_route():
    from oryon_amd.synth import make_pair
    ins = _stack([make_pair(970 + i, H, H, 256, device="cuda") for i in range(3)])
    r1 = _run(ins, 1, steps=5, first_key=970, x3_prefetch=1)
    assert r1[-1]["x3_steps"] == 0
    assert (r1[-1]["stats"][:, 1] > 0).all()
