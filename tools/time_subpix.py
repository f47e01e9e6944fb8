"""Time of the sub-pixel refinement's two entry points (csrc/match_subpix.hip) on the GPU box.

    python tools/time_subpix.py [--json OUT] [--pairs 64] [--rows 500] [--size 224] [--channels 256]

In ONE process on one GPU, for 64 pairs x 500 rows on 224 x 224 maps of 256 channels (bench.py's shape):
  fit_nchw / fit_nhwc   ops.subpix_refine (the fit and the count launch) on channel-planar and on channels_last maps;
  lift_subpix           ops.lift_pairs_subpix with the fit's offsets onto 480 x 640 depth maps;
  lift                  ops.lift_pairs (K2, unchanged) on the same rows: the yardstick.
Each figure is the median of 7 windows of CALLS back-to-back calls between two HIP events, the contestants alternating window by
window after a warm-up of all; min and max of the windows are printed next to it.  Before anything is timed the two layouts' outputs
are compared byte for byte.  The maps are seeded normals: the fit's work does not depend on the values.  The bytes the fit needs are
computed from the shape (19 descriptor reads per row: one anchor pixel, nine query pixels - the line count on NCHW is an estimate of
one 128-byte line per channel and map row touched, not a counter reading)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oryon_amd  # noqa: E402

oryon_amd.configure()
from oryon_amd import ops  # noqa: E402

WINDOWS = 7
CALLS = 5


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(B, rows, S, C, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    fa = torch.empty((B, C, S, S), dtype=torch.float32, device=dev)
    fq = torch.empty((B, C, S, S), dtype=torch.float32, device=dev)
    for p in range(B):                                                    # pair by pair: no second copy of the large operand
        fa[p].normal_(generator=g)
        fq[p].normal_(generator=g)
    fa_l, fq_l = fa.contiguous(memory_format=torch.channels_last), fq.contiguous(memory_format=torch.channels_last)
    n_cap = ops.round_up(rows, 128)
    corrs = torch.randint(1, S - 1, (B, n_cap, 4), generator=g, device=dev, dtype=torch.int32)      # interior rows: every one is fitted
    n = torch.full((B,), rows, dtype=torch.int32, device=dev)
    HD, WD = 480, 640
    depth = (600.0 + 0.2 * torch.arange(WD, device=dev, dtype=torch.float32)[None, None, :] +
             0.1 * torch.arange(HD, device=dev, dtype=torch.float32)[None, :, None]).expand(B, HD, WD).contiguous()
    cam = torch.tensor([[600.0, 0, WD / 2, 0, 600.0, HD / 2, 0, 0, 1]], dtype=torch.float32, device=dev).repeat(B, 1)
    fit = {"fit_nchw": lambda: ops.subpix_refine(fa, fq, corrs, n, None, 1e-4), "fit_nhwc": lambda: ops.subpix_refine(fa_l, fq_l, corrs, n, None, 1e-4)}
    a, b = fit["fit_nchw"](), fit["fit_nhwc"]()
    torch.cuda.synchronize()
    if not (torch.equal(a["offsets"].view(torch.int32), b["offsets"].view(torch.int32)) and torch.equal(a["flags"], b["flags"])
            and torch.equal(a["counts"], b["counts"])):
        raise SystemExit("the two layouts disagree - nothing timed")
    off = a["offsets"]
    contestants = dict(fit, lift_subpix=lambda: ops.lift_pairs_subpix(corrs, n, (S, S), depth, depth, cam, cam, None, offsets=off, depth_jump=0.02),
                       lift=lambda: ops.lift_pairs(corrs, n, (S, S), depth, depth, cam, cam, None))
    for f in contestants.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in contestants}
    for _ in range(WINDOWS):
        for k, f in contestants.items():
            t[k].append(window_ms(f, CALLS))
    med = {k: sorted(v)[WINDOWS // 2] for k, v in t.items()}
    need = B * rows * 10 * C * 4                                          # descriptor bytes the fit reads
    lines_nchw = B * rows * C * 4 * 128                                   # one line per channel for the anchor, three for the stencil's rows
    out = dict(B=B, rows=rows, n_cap=n_cap, size=S, C=C, windows=WINDOWS, calls_per_window=CALLS, ms=med,
               spread_ms={k: [min(v), max(v)] for k, v in t.items()}, fit_bytes_needed=need, fit_nchw_line_bytes_estimated=lines_nchw,
               fit_nhwc_gbps_of_needed=need / med["fit_nhwc"] / 1e6, fit_nchw_gbps_of_estimated_lines=lines_nchw / med["fit_nchw"] / 1e6,
               flag_counts=a["counts"].sum(0).tolist(), layouts_equal=True)
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_subpix.py measures on the GPU: none here, nothing measured")
    res = measure(a.pairs, a.rows, a.size, a.channels, "cuda")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
