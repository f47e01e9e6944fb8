"""CPU estimate of the default-route cascade's band rules (csrc/match_corrs.hip, match_dc_probe_band_kernel) on the benchmark's own
generator: the share of all (anchor row, query tile) products the band pass multiplies and the rows it leaves open, for one band per
1024-row panel and for one sub-band per 512-row half nested in the panel's band.  No GPU: the exact matcher of oracle/oryon_oracle.py
on oryon_amd/synth.py pairs, so a band rule can be re-priced before a kernel is written.

    python tools/dc_band_estimate.py [--pairs 12] [--first 0] [--size 224] [--channels 256]

Model (an estimate, not the device's arithmetic): a probe row is "sure" where the oracle calls it valid (the device's line sits a
screening error above the threshold); a row finds its witness in a band iff it is valid and its argmin's tile lies in the band (with
Gaussian descriptors the match is the only query within the threshold); the 5000 anchors are a random subset in ROI order, not the
device's keyed subsample.  Counts are means over the pairs."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oryon_oracle as orc  # noqa: E402
from oryon_amd.synth import make_pair  # noqa: E402

TILE = 128              # query rows per tile of the screen
PANEL = 1024            # anchor rows per parent panel
STRIDE, SLACK, MIN_SURE, CAP_NUM, CAP_DEN = 10, 2, 8, 1, 2      # dc_probe_stride, DC_SLACK, DC_MIN_SURE, DC_BAND_CAP_*
MAX_PROBE = 512         # MX6_SAMPLED_PANEL


def learned_bands(tile, valid, nqt, sub_rows, stride=STRIDE, slack=SLACK):
    """Per anchor row the band [first, end) its panel (sub_rows = 1024) or its half of the panel (sub_rows = 512) scans, and whether the
    row's 1024-row panel scans all tiles.  tile: the argmin's tile per row; valid: the oracle's flag per row."""
    n = len(tile)
    first, end, scans_all = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    rows = np.arange(n)
    probe = (rows % stride == 0) & (rows // stride < MAX_PROBE)

    def span(sel):
        t = tile[sel & probe & valid]
        return (int(t.min()), int(t.max()), len(t)) if len(t) else (0, -1, 0)
    for a0 in range(0, n, PANEL):
        in_panel = (rows >= a0) & (rows < a0 + PANEL)
        lo, hi, cnt = span(in_panel)
        f, e = max(lo - slack, 0), min(hi + slack + 1, nqt)
        full = cnt < MIN_SURE or (e - f) * CAP_DEN > nqt * CAP_NUM
        if full:
            f, e = 0, nqt
        first[in_panel], end[in_panel], scans_all[in_panel] = f, e, full
        if full or sub_rows >= PANEL:
            continue
        for h0 in range(a0, min(a0 + PANEL, n), sub_rows):
            in_half = (rows >= h0) & (rows < h0 + sub_rows)
            lo, hi, cnt = span(in_half)
            if cnt >= MIN_SURE:
                first[in_half], end[in_half] = max(lo - slack, f), min(hi + slack + 1, e)
    return first, end, scans_all, probe


def estimate(index, size, channels, n_anchors, rules):
    """[(band share, open rows) for sub_rows in rules] of pair `index`: one exact match, every rule on it"""
    p = make_pair(index, size, size, channels)
    roi = orc.roi_from_mask(p["mask_a"])
    g = torch.Generator().manual_seed(4242 + index)
    if roi.shape[0] > n_anchors:
        roi = roi[torch.randperm(roi.shape[0], generator=g)[:n_anchors].sort().values]      # a random subset, kept in ROI order
    m = orc.match_presample(p["feat_a"], p["feat_q"], p["mask_a"], p["mask_q"], 0.25, roi1_override=roi)
    valid, tile = m["valid"].numpy(), m["argmin"].numpy() // TILE
    nqt = (m["roi2"].shape[0] + TILE - 1) // TILE
    out = []
    for sub_rows in rules:
        first, end, scans_all, probe = learned_bands(tile, valid, nqt, sub_rows)
        witness = valid & (tile >= first) & (tile < end)
        out.append((float((end - first).sum()) / (len(tile) * nqt), int((~probe & ~scans_all & ~witness).sum())))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--anchors", type=int, default=5000)
    a = ap.parse_args()
    print("| | band share of all (row, tile) products | open rows per pair |")
    print("|---|---:|---:|")
    names = ("one band per 1024 rows", "sub-band per 512 rows, nested in the panel's band")
    r = [estimate(a.first + i, a.size, a.channels, a.anchors, (PANEL, PANEL // 2)) for i in range(a.pairs)]
    for k, name in enumerate(names):
        print(f"| {name} | {np.mean([x[k][0] for x in r]):.3f} | {np.mean([x[k][1] for x in r]):.0f} |")


if __name__ == "__main__":
    main()
