"""Time of the ratio matcher's second scan against one call of the exact matcher (GPU box).

    python tools/time_match_second.py [--json OUT] [--shapes bench,ref,c512,...] [--radius 5] [--ratio 0.8]

For every shape, in ONE process on one GPU: ops.match_second (csrc/match_second.hip: K1's tile walk with a per-anchor spatial mask in
the fold) against ONE call of ops.match at the same shape - the existing kernel, unchanged by the ratio matcher, so its time is the
parent's.  The expectation to check is one scan plus a small term.  Each figure is the median of 7 windows of CALLS back-to-back calls
between two HIP events, the two contestants alternating window by window after a warm-up of both; min and max of the windows are
printed next to it.  Before a shape is timed, second_dist / second_argmin of a few rows are compared byte for byte with the existing
kernel run on those rows' candidates alone (compacted in order), and keep with its definition on every row, so a time is never read
for a kernel that computes something else.
Shapes (unit rows of seeded normals, n_a / n_q rows of every pair in use; the query rows are the pixels of a full square map):
  bench  bench.py's matcher shape: B = 64, C = 256, n_a = 5000, n_q = 224 x 224
  ref    the reference's own width: B = 64, C = 32, n_a = 5000, n_q = 192 x 192
  c64 / c128  the two widths between (same pair shape as ref)
  c512   the LDS-staged kernel: B = 8, C = 512, n_a = 5000, n_q = 192 x 192"""
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
SHAPES = {          # name: (B, C, n_a, W (n_q = W x W), calls per window)
    "bench": (64, 256, 5000, 224, 3),
    "ref": (64, 32, 5000, 192, 10),
    "c64": (64, 64, 5000, 192, 10),
    "c128": (64, 128, 5000, 192, 6),
    "c512": (8, 512, 5000, 192, 6),
}
PROBES = ((0, 0), (0, 127), (0, 128), (1, 4999), (3, 2500), (7, 31))       # (pair, anchor row) compared with the existing kernel


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def rows(B, n, C, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    cap = ops.round_up(n, ops.ROW_PAD)
    x = torch.empty((B, cap, C), dtype=torch.float32, device=dev)
    for p in range(B):                                                   # pair by pair: no second copy of the large operand
        x[p] = torch.nn.functional.normalize(torch.randn(cap, C, generator=g, device=dev), dim=1)
    return x, torch.full((B,), n, dtype=torch.int32, device=dev)


def outputs_agree(a_hat, q_hat, n_q, W, radius, ratio, md, am, va, sd, sa, kp, na):
    """second_* of PROBES against ops.match on the candidates alone; keep against its definition on every row."""
    dev = a_hat.device
    nq, Cp = int(n_q[0]), a_hat.shape[2]
    pix = torch.arange(nq, device=dev)
    y, x = pix // W, pix % W
    a = torch.zeros((len(PROBES), 128, Cp), device=dev)
    q = torch.zeros((len(PROBES), q_hat.shape[1], Cp), device=dev)
    tables, counts = [], []
    for b, (p, i) in enumerate(PROBES):
        j0 = int(am[p, i])
        js = torch.nonzero((y - y[j0]) ** 2 + (x - x[j0]) ** 2 >= radius * radius).squeeze(1)
        a[b, 0] = a_hat[p, i]
        q[b, :len(js)] = q_hat[p, js]
        tables.append(js)
        counts.append(len(js))
    one = torch.ones(len(PROBES), dtype=torch.int32, device=dev)
    ymd, yam, _ = ops.match(a, q, one, torch.tensor(counts, dtype=torch.int32, device=dev), 0.25)
    ok = all(torch.equal(sd[p, i].view(torch.int32), ymd[b, 0].view(torch.int32)) and int(sa[p, i]) == int(tables[b][int(yam[b, 0])])
             for b, (p, i) in enumerate(PROBES))
    want = va[:, :na].bool() & (md[:, :na] <= torch.tensor(ratio, dtype=torch.float32, device=dev) * sd[:, :na])
    return ok and torch.equal(kp[:, :na].bool(), want) and bool((sd[:, :na] >= md[:, :na]).all())


def measure(name, dev, radius, ratio):
    B, C, na, W, calls = SHAPES[name]
    nq = W * W
    a_hat, n_a = rows(B, na, C, 1, dev)
    q_hat, n_q = rows(B, nq, C, 2, dev)
    roi_q = torch.arange(q_hat.shape[1], dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
    thr = 0.25
    md, am, va = ops.match(a_hat, q_hat, n_a, n_q, thr)
    second = lambda: ops.match_second(a_hat, q_hat, n_a, n_q, roi_q, W, radius, md, am, va, ratio)
    first = lambda: ops.match(a_hat, q_hat, n_a, n_q, thr)
    sd, sa, kp = second()
    torch.cuda.synchronize()
    if not outputs_agree(a_hat, q_hat, n_q, W, radius, ratio, md, am, va, sd, sa, kp, na):
        raise SystemExit(f"{name}: the second scan disagrees with the existing kernel on its candidates - nothing timed")
    for f in (second, first):
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {"second": [], "match": []}
    for _ in range(WINDOWS):
        t["second"].append(window_ms(second, calls))
        t["match"].append(window_ms(first, calls))
    med = {k: sorted(v)[WINDOWS // 2] for k, v in t.items()}
    tflop = 2.0 * B * na * nq * C / 1e12
    out = dict(shape=name, B=B, C=C, n_a=na, n_q=nq, W_q=W, radius=radius, ratio=ratio, windows=WINDOWS, calls_per_window=calls,
               valid_rows=int(va[:, :na].sum()), kept_rows=int(kp[:, :na].sum()), second_ms=med["second"], match_ms=med["match"],
               second_over_match=med["second"] / med["match"], spread_ms={k: [min(v), max(v)] for k, v in t.items()},
               matrix_tflop_one_scan=tflop, second_tflops=tflop / (med["second"] * 1e-3), outputs_equal=True)
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="bench,ref,c64,c128,c512")
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_match_second.py measures on the GPU: none here, nothing measured")
    res = [measure(s, "cuda", a.radius, a.ratio) for s in a.shapes.split(",")]
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
