"""Sub-bands of the default route's validity cascade (csrc/match_corrs.hip, match_dc_probe_band_kernel): every 512-row half of a
1024-anchor panel scans the tile range of its OWN sure probe rows, nested in the panel's band, in the 4-wave windowed screen
(match_mx6_screen_w4_win_kernel<256, 4, KL>); match_dc_settle_rows_kernel classifies with one row per lane and iteration and lists the
open rows through a block-wide ordered scan.  As in test_gpu_default_cascade.py every result must be BIT FOR BIT that of the plain full
screen (knob 0) - poses, statuses, counts, correspondences - and what the C oracle's exact fp32 scan gives.

Shape: 96 x 96 maps (2304 anchors = 3 live panels = 5 halves, the last one of 256 rows; ~61 query tiles), C = 256, 3-4 pairs."""
import numpy as np
import pytest
import torch

from tests.test_gpu_default_cascade import _assert_equal, _live_panels, _np_pairs, _run, _stack

pytestmark = pytest.mark.gpu

H = 96
STRIDE = 10                 # the probe stride at cap_a = 5120 (dc_probe_stride)
TILE = 128                  # query rows per tile


def _oracle(r, ins, b):
    from oracle import c_oracle
    n_a, n_q = int(r["n_a"][b]), int(r["n_q"][b])
    roi_a, roi_q = r["roi_a"][b, :n_a], r["roi_q"][b, :n_q]
    fa, fq = ins[0][b].cpu().numpy(), ins[1][b].cpu().numpy()
    _, am, va = c_oracle.match_lin(fa, fq, roi_a, roi_q, 0.25)
    return roi_a, roi_q, am, va


def _vs_oracle(r, ins, size=H, pairs=None):
    """valid of every anchor row, n_valid and the query pixel of every sampled correspondence against the C oracle's exact scan"""
    for b in (range(ins[0].shape[0]) if pairs is None else pairs):
        n_a = int(r["n_a"][b])
        roi_a, roi_q, am, va = _oracle(r, ins, b)
        assert np.array_equal(r["valid"][b, :n_a].astype(bool), va), f"pair {b}: valid set differs from the C oracle"
        assert int(r["n_valid"][b]) == int(va.sum())
        corrs = r["corrs"][b].numpy().astype(np.int64)
        if len(corrs) == 0:
            continue
        row = np.searchsorted(roi_a, corrs[:, 0] * size + corrs[:, 1])
        assert va[row].all()
        assert np.array_equal(corrs[:, 2] * size + corrs[:, 3], roi_q[am[row]]), f"pair {b}: a sampled query pixel is not the oracle's argmin"


def _sure_probe_tiles(am, va, a0, a1):
    """(lowest tile, highest tile, count) of the oracle-valid probe rows among the rows a0 .. a1 - 1"""
    t = [int(am[a]) // TILE for a in range(a0, a1) if a % STRIDE == 0 and va[a]]
    return (min(t), max(t), len(t)) if t else (0, -1, 0)


def test_partial_last_half():
    """2304 anchors: panels of 1024, 1024 and 256 rows, i.e. five halves of which the last holds 256 rows.  Pairs in which some anchors
    have no counterpart (the motion moves them out of the query view: 183 / 205 / 425 of 2304 by the generator's geometry), so every
    pair has rows to leave open."""
    from oryon_amd.synth import make_pair
    ins = _stack([make_pair(i, H, H, 256, device="cuda") for i in (983, 984, 986)])
    r0, r1 = _run(ins, 0, first_key=980), _run(ins, 1, first_key=980)
    _assert_equal(r0, r1)
    for r in r1:
        s = r["stats"]
        print("stats (probe, settled, open, band tiles):", s.tolist(), "n_a", r["n_a"].tolist(), "n_q", r["n_q"].tolist())
        assert r["n_a"].tolist() == [2304] * 3
        assert (s[:, 1] > 0).all() and (s[:, 2] > 0).all(), s
        for b in range(3):
            assert int(s[b, 3]) < _live_panels(r["n_a"][b]) * ((int(r["n_q"][b]) + TILE - 1) // TILE), s[b]
    _vs_oracle(r1[-1], ins)


def test_a_half_without_sure_probe_rows_takes_the_panels_band():
    """The anchor descriptors under rows 512 .. 1023 of one pair are fresh noise: that half has no sure probe row while its panel keeps the
    ~50 of the other half, so the panel still learns a band, the half scans it, finds no witness, and all its rows that are no probe
    rows end up open and - after the complete scan - invalid."""
    from oryon_amd.synth import make_pair
    pairs = [make_pair(983 + i, H, H, 256, device="cuda") for i in range(3)]
    b = 1
    live = pairs[b]["mask_a"].view(-1).nonzero().flatten()             # ROI order: no subsampling below 5000 anchors
    assert len(live) == 2304
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    fa = pairs[b]["feat_a"].clone().view(256, -1)
    fa[:, live[512:1024]] = torch.randn(256, 512, generator=g, device="cuda")
    pairs[b]["feat_a"] = fa.view(256, H, H)
    ins = _stack(pairs)
    r0, r1 = _run(ins, 0, steps=2, first_key=983), _run(ins, 1, steps=2, first_key=983)
    _assert_equal(r0, r1)
    r = r1[-1]
    roi_a, roi_q, am, va = _oracle(r, ins, b)
    assert np.array_equal(roi_a, live.cpu().numpy())
    assert _sure_probe_tiles(am, va, 0, 512)[2] >= 8 and _sure_probe_tiles(am, va, 512, 1024)[2] == 0       # the construction, on the CPU
    nqt = (int(r["n_q"][b]) + TILE - 1) // TILE
    print("stats", r["stats"][b].tolist(), "nqt", nqt)
    lo0, hi0, _ = _sure_probe_tiles(am, va, 0, 512)
    assert 2 * (hi0 - lo0 + 5) <= nqt                                     # ... whose range + slack is a band below the cap of 1/2
    assert int(r["stats"][b, 3]) < 3 * nqt
    n_probe_half = len([a for a in range(512, 1024) if a % STRIDE == 0])
    assert int(r["stats"][b, 2]) >= 512 - n_probe_half                                                      # the half's rows are open ..
    assert not r["valid"][b, 512:1024].any()                                                                # .. and invalid
    _vs_oracle(r, ins)


def test_a_better_match_in_the_panels_band_outside_the_halfs_sub_band():
    """The descriptors of the true matches of 60 anchors of the SECOND half of panel 0 (no probe rows among them) are copied onto earlier
    query pixels that no anchor matches, in tiles only the FIRST half's matches occupy: inside the panel's band, at least 3 tiles
    (slack 2 + 1: the device's sure line is not the oracle's threshold) below the second half's own range.  The anchors settle on
    their witness inside the sub-band, the oracle's argmin (first index) is the copy, and every sampled one must carry its pixel."""
    from oryon_amd.synth import make_pair
    pairs = [make_pair(980 + i, H, H, 256, device="cuda") for i in range(3)]
    ins = _stack(pairs)
    base = _run(ins, 1, steps=1, first_key=980)[0]
    b = 1
    n_q = int(base["n_q"][b])
    roi_a, roi_q, am, va = _oracle(base, ins, b)
    lo0, hi0, c0 = _sure_probe_tiles(am, va, 0, 512)
    lo1, hi1, c1 = _sure_probe_tiles(am, va, 512, 1024)
    assert c0 >= 8 and c1 >= 8
    t_hi = min(hi0, lo1 - 3)
    matched = set(am[va].tolist())
    targets = [j for j in range(lo0 * TILE, (t_hi + 1) * TILE) if j < n_q and j not in matched][:60]
    rows = [a for a in range(512, 1024) if a % STRIDE and va[a] and am[a] >= (lo1 - 2) * TILE][:60]
    assert len(targets) == 60 and len(rows) == 60, (lo0, hi0, lo1, hi1, len(targets), len(rows))
    fq_t = pairs[b]["feat_q"].clone().view(256, -1)
    for j, a in zip(targets, rows):
        fq_t[:, int(roi_q[j])] = fq_t[:, int(roi_q[am[a]])]
    pairs[b]["feat_q"] = fq_t.view(256, H, H)
    ins = _stack(pairs)
    r0, r1 = _run(ins, 0, steps=2, first_key=980), _run(ins, 1, steps=2, first_key=980)
    _assert_equal(r0, r1)
    r = r1[-1]
    nqt = (n_q + TILE - 1) // TILE
    assert int(r["stats"][b, 3]) < _live_panels(r["n_a"][b]) * nqt and int(r["stats"][b, 1]) > 0      # learned bands, settled rows
    _vs_oracle(r, ins)
    _, _, am2, _ = _oracle(r, ins, b)
    corrs = r["corrs"][b].numpy().astype(np.int64)
    srow = np.searchsorted(roi_a, corrs[:, 0] * H + corrs[:, 1])
    hit = 0
    for j, a in zip(targets, rows):
        assert int(am2[a]) == j                                           # the oracle's argmin is the copy (first index)
        for s in np.nonzero(srow == a)[0]:
            assert corrs[s, 2] * H + corrs[s, 3] == int(roi_q[j])
            hit += 1
    assert hit > 0, "none of the 60 anchors was sampled"


def test_ragged_counts_in_one_batch():
    """1030 anchors (the second panel holds 6 rows and no probe row: no band can be learned there), 1539 (the last half holds 3 rows),
    an empty query mask and a full pair in one batch"""
    from oryon_amd.synth import make_pair
    pairs = [make_pair(986 + i, H, H, 256, device="cuda") for i in range(4)]
    for i, n in ((0, 1030), (1, 1539)):
        pairs[i]["mask_a"] = pairs[i]["mask_a"].clone()
        live = pairs[i]["mask_a"].view(-1).nonzero().flatten()
        pairs[i]["mask_a"].view(-1)[live[n:]] = 0
    pairs[2]["mask_q"] = torch.zeros_like(pairs[2]["mask_q"])
    ins = _stack(pairs)
    r0, r1 = _run(ins, 0, steps=2, first_key=986), _run(ins, 1, steps=2, first_key=986)
    _assert_equal(r0, r1)
    r = r1[-1]
    s = r["stats"]
    print("stats", s.tolist(), "n_a", r["n_a"].tolist(), "n_q", r["n_q"].tolist())
    assert r["n_a"].tolist() == [1030, 1539, 2304, 2304] and int(r["n_q"][2]) == 0
    assert s[:, 0].tolist() == [(int(n) + STRIDE - 1) // STRIDE for n in r["n_a"]]
    nqt = [(int(n) + TILE - 1) // TILE for n in r["n_q"]]
    assert nqt[0] < int(s[0, 3]) < 2 * nqt[0]                            # panel 0 learned a band, the 6-row panel scans all tiles
    assert int(s[1, 3]) < 2 * nqt[1] and int(s[3, 3]) < 3 * nqt[3]
    assert int(s[2, 1]) == 0 and int(s[2, 2]) == 0 and int(s[2, 3]) == 0
    assert (s[[0, 1, 3], 1] > 0).all()
    assert (s[:, 0] + s[:, 1] + s[:, 2] <= r["n_a"]).all()
    assert int(r["status"][2]) != 0 and int(r["status"][3]) == 0 and int(r["n_valid"][2]) == 0
    _vs_oracle(r, ins, pairs=(0, 1, 3))


def test_ordered_open_list_over_scan_iterations_and_panels():
    """160 x 160, 5000 anchors = 10 halves, mask_q without its lower half (the construction of
    test_more_than_one_compact_panel_of_open_rows): more than 1024 open rows, spread over all five iterations of the settle pass's
    scan; an open list out of order or with a gap scatters a complete triple to the wrong row, which the oracle's valid set and
    argmins catch."""
    from oryon_amd.synth import make_pair
    HB = 160
    pairs = [make_pair(920, HB, HB, 256, device="cuda"), make_pair(963, HB, HB, 256, device="cuda"), make_pair(922, HB, HB, 256, device="cuda")]
    pairs[1]["mask_q"] = pairs[1]["mask_q"].clone()
    pairs[1]["mask_q"][HB // 2:] = 0
    ins = _stack(pairs)
    r0, r1 = _run(ins, 0, steps=2, first_key=920), _run(ins, 1, steps=2, first_key=920)
    _assert_equal(r0, r1)
    r = r1[-1]
    print("stats", r["stats"].tolist())
    assert int(r["n_a"][1]) == 5000
    assert int(r["stats"][1, 2]) > 1024 and int(r["stats"][1, 1]) > 0, r["stats"][1]
    _vs_oracle(r, ins, size=HB, pairs=(1,))


@pytest.mark.parametrize("C", [32, 96])
def test_narrow_maps(C):
    """the KL = 1 / KL = 2 instantiations of the 4-wave windowed kernel"""
    from oryon_amd.synth import make_pair
    ins = _stack([make_pair(990 + C + i, H, H, C, device="cuda") for i in range(3)])
    r0, r1 = _run(ins, 0, steps=2, first_key=990), _run(ins, 1, steps=2, first_key=990)
    _assert_equal(r0, r1)
    for r in r1:
        assert (r["stats"][:, 0] > 0).all() and (r["stats"][:, 3] > 0).all(), r["stats"]
    _vs_oracle(r1[-1], ins)
