"""Time of the fused mutual matcher against the two calls it replaces (GPU box).

    python tools/time_match_mutual.py [--json OUT] [--shapes bench,ref,c512,...]

For every shape, in ONE process on one GPU: ops.match_mutual (csrc/match_mutual.hip: one scan, both directions) against TWO calls of
ops.match (forward, then the roles swapped) - the existing kernel, which is what a caller without the fused entry would run.  Each
figure is the median of 7 windows of CALLS back-to-back calls between two HIP events, the two contestants alternating window by window
after a warm-up of both; min and max of the windows are printed next to it.  Before a shape is timed the two sets of outputs are
compared byte for byte on the rows of every pair, so a time is never read for a kernel that computes something else.
Shapes (unit rows of seeded normals, n_a / n_q rows of every pair in use):
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
SHAPES = {          # name: (B, C, n_a, n_q, calls per window)
    "bench": (64, 256, 5000, 224 * 224, 3),
    "ref": (64, 32, 5000, 192 * 192, 10),
    "c64": (64, 64, 5000, 192 * 192, 10),
    "c128": (64, 128, 5000, 192 * 192, 6),
    "c512": (8, 512, 5000, 192 * 192, 6),
}


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


def measure(name, dev):
    B, C, na, nq, calls = SHAPES[name]
    a_hat, n_a = rows(B, na, C, 1, dev)
    q_hat, n_q = rows(B, nq, C, 2, dev)
    thr = 0.25
    fused = lambda: ops.match_mutual(a_hat, q_hat, n_a, n_q, thr)
    two = lambda: (ops.match(a_hat, q_hat, n_a, n_q, thr), ops.match(q_hat, a_hat, n_q, n_a, thr))
    one = lambda: ops.match(a_hat, q_hat, n_a, n_q, thr)
    md, am, va, rmd, ram, mu = fused()
    (md2, am2, va2), (rmd2, ram2, _) = two()
    torch.cuda.synchronize()
    same = all(torch.equal(x[:, :n].view(torch.int32) if x.dtype == torch.float32 else x[:, :n], y[:, :n].view(torch.int32) if y.dtype == torch.float32 else y[:, :n])
               for x, y, n in ((md, md2, na), (am, am2, na), (va, va2, na), (rmd, rmd2, nq), (ram, ram2, nq)))
    if not same:
        raise SystemExit(f"{name}: the fused call and the two calls disagree - nothing timed")
    for f in (fused, two, one):
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {"fused": [], "two_calls": [], "forward_only": []}
    for _ in range(WINDOWS):
        t["fused"].append(window_ms(fused, calls))
        t["two_calls"].append(window_ms(two, calls))
        t["forward_only"].append(window_ms(one, calls))
    med = {k: sorted(v)[WINDOWS // 2] for k, v in t.items()}
    tflop = 2.0 * B * na * nq * C / 1e12
    out = dict(shape=name, B=B, C=C, n_a=na, n_q=nq, windows=WINDOWS, calls_per_window=calls, mutual_rows=int(mu.sum()),
               fused_ms=med["fused"], two_calls_ms=med["two_calls"], forward_only_ms=med["forward_only"],
               fused_over_two_calls=med["fused"] / med["two_calls"], fused_over_forward_only=med["fused"] / med["forward_only"],
               spread_ms={k: [min(v), max(v)] for k, v in t.items()}, matrix_tflop_one_scan=tflop,
               fused_tflops=tflop / (med["fused"] * 1e-3), atomic_bytes=B * nq * ((na + 127) // 128) * 8, outputs_equal=True)
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="bench,ref,c64,c128,c512")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_match_mutual.py measures on the GPU: none here, nothing measured")
    res = [measure(s, "cuda") for s in a.shapes.split(",")]
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
