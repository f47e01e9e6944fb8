"""Time of the one-to-many matcher's rank scan and of the complete oryon_topk_corrs against the ratio matcher's second scan (GPU box).

    python tools/time_match_next.py [--json OUT] [--shapes bench,ref] [--radius 5]

For every shape, in ONE process on one GPU:
  next     one rank scan (ops.match_next, csrc/match_next.hip) on the DRAWN rows only: 64 pairs x 512 rows, one earlier rank;
  second   ops.match_second (K1r, unchanged by this feature) on ALL cap_a anchor rows of the same pairs: the yardstick;
  topk2/4  the complete ops.topk_corrs (sampler, gather, K - 1 rank scans, expansion) at K = 2 and K = 4, max_corrs = 512;
  select   ops.select_corrs alone (what topk = 1 runs).
The expectation to check, not to assume: a rank scan on cap_s rows costs roughly cap_s / cap_a of K1r (the query stream is the same,
the anchor panels are a tenth).  Each figure is the median of 7 windows of CALLS back-to-back calls between two HIP events, the
contestants alternating window by window after a warm-up of all; min and max of the windows are printed next to it.  Before a shape is
timed, the rank scan of the drawn rows is compared byte for byte with K1r's second minimum of the same rows, so a time is never read
for a kernel that computes something else.
Shapes (unit rows of seeded normals; the query rows are the pixels of bench.py's 224 x 224 map):
  bench  bench.py's matcher shape: B = 64, C = 256, n_a = 5000
  ref    the reference's own width: B = 64, C = 32, n_a = 5000"""
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
DRAWN = 512
SHAPES = {          # name: (B, C, n_a, W (n_q = W x W), calls per window)
    "bench": (64, 256, 5000, 224, 3),
    "ref": (64, 32, 5000, 224, 6),
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


def measure(name, dev, radius):
    B, C, na, W, calls = SHAPES[name]
    nq = W * W
    a_hat, n_a = rows(B, na, C, 1, dev)
    q_hat, n_q = rows(B, nq, C, 2, dev)
    cap_a = a_hat.shape[1]
    roi_a = torch.arange(cap_a, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
    roi_q = torch.arange(q_hat.shape[1], dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
    thr = 0.5                                                            # every row valid: the sampler draws 512 of 5000 without replacement
    md, am, va = ops.match(a_hat, q_hat, n_a, n_q, thr)
    key = torch.arange(B, dtype=torch.int64, device=dev)
    # the drawn rows, as oryon_topk_corrs gathers them
    t2 = ops.topk_corrs(a_hat, q_hat, roi_a, roi_q, n_a, n_q, md, am, va, thr, W, DRAWN, 1, 2, radius, 0.1, key, tables=True)
    sel = t2["sel_rows"].long()
    a_s = torch.gather(a_hat, 1, sel[:, :, None].expand(-1, -1, a_hat.shape[2])).contiguous()
    am_s = torch.gather(am, 1, sel).contiguous()
    n_s = torch.full((B,), DRAWN, dtype=torch.int32, device=dev)
    nxt = lambda: ops.match_next(a_s, q_hat, n_s, n_q, roi_q, W, radius, am_s[None])
    second = lambda: ops.match_second(a_hat, q_hat, n_a, n_q, roi_q, W, radius, md, am, va, 1.0)
    topk = {K: (lambda K=K: ops.topk_corrs(a_hat, q_hat, roi_a, roi_q, n_a, n_q, md, am, va, thr, W, DRAWN, 1, K, radius, 0.1, key)) for K in (2, 4)}
    select = lambda: ops.select_corrs(roi_a, roi_q, n_a, n_q, am, va, W, DRAWN, 1, key)
    nd, nj = nxt()
    sd, sa, _ = second()
    torch.cuda.synchronize()
    want_d, want_j = torch.gather(sd, 1, sel), torch.gather(sa, 1, sel)
    same = torch.equal(nd.view(torch.int32), want_d.view(torch.int32)) and torch.equal(nj, torch.where(torch.isinf(want_d), -1, want_j)) \
        and torch.equal(t2["cand_dist"][1].view(torch.int32), nd.view(torch.int32)) and torch.equal(t2["cand_argmin"][1], nj)
    if not same:
        raise SystemExit(f"{name}: the rank scan of the drawn rows disagrees with K1r's second minimum of those rows - nothing timed")
    contestants = {"next": nxt, "second": second, "topk2": topk[2], "topk4": topk[4], "select": select}
    for f in contestants.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in contestants}
    for _ in range(WINDOWS):
        for k, f in contestants.items():
            t[k].append(window_ms(f, calls))
    med = {k: sorted(v)[WINDOWS // 2] for k, v in t.items()}
    out = dict(shape=name, B=B, C=C, n_a=na, cap_a=cap_a, drawn=DRAWN, n_q=nq, W_q=W, radius=radius, windows=WINDOWS, calls_per_window=calls,
               ms=med, spread_ms={k: [min(v), max(v)] for k, v in t.items()}, next_over_second=med["next"] / med["second"],
               rows_ratio=DRAWN / cap_a, topk2_minus_select_ms=med["topk2"] - med["select"],
               topk4_minus_select_ms=med["topk4"] - med["select"], rows_k2=int(t2["n_rows"].sum()), outputs_equal=True)
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="bench,ref")
    ap.add_argument("--radius", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_match_next.py measures on the GPU: none here, nothing measured")
    res = [measure(s, "cuda", a.radius) for s in a.shapes.split(",")]
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
