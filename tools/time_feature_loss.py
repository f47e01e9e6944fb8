"""Time of the validation step's loss at the workload's sizes (GPU box): 64 pairs x 500 correspondences x a pool of 2000, at C = 32 on
192 x 192 maps and at C = 256 on 224 x 224 maps.

    python tools/time_feature_loss.py [--pairs 64] [--corrs 500] [--json OUT]

Prints, measured in ONE process on one GPU, after warm-up, with HIP events, as the median of several windows of back-to-back calls:
  * oryon_feature_loss alone (ops.feature_loss with the pool tables and workspace made beforehand);
  * losses.FeatureLoss.forward as a whole (coordinate rescale, the pool draws of torch.multinomial, both mask losses);
  * the comparison: the per-sample torch loop of the same definition on the same device (the structure of the reference's loop: per
    valid pair and side a [N, P, C] cosine, the fp32 penalty, argmin, a gather) with the same pool tables.  The parent commit has no
    counterpart to compare with;
  * the arithmetic next to it: 2 N P C flop per pair and side, and the pool gather's bytes (P C 4 per pair and side)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oryon_amd  # noqa: E402

oryon_amd.configure()
from oryon_amd import ops  # noqa: E402
from oryon_amd.losses import FeatureLoss  # noqa: E402
from oryon_amd.pipeline import default_args  # noqa: E402

POOL = 2000


def windows_ms(fn, reps, windows=5, warm=3):
    """Median over `windows` of the HIP-event time of `reps` back-to-back calls, per call."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return float(np.median(out)), [round(x, 4) for x in out]


def torch_loop(fa, fq, corrs, pool, neg_kernel=5.0):
    """The per-sample loop of the definition in torch on the device: (d_pos, d_neg) as the kernel returns them."""
    B, C, FH, FW = fa.shape
    d_neg = torch.zeros((B, 2, corrs.shape[1]), device=fa.device)
    d_pos = torch.zeros((B, corrs.shape[1]), device=fa.device)
    unit = lambda r: r / torch.linalg.vector_norm(r, dim=1, keepdim=True).clamp_min(1e-8)
    for b in range(B):
        pos = []
        for side, fm in ((0, fa), (1, fq)):
            rows = fm[b].reshape(C, FH * FW).T
            yx = corrs[b, :, 2 * side:2 * side + 2].long()
            p = unit(rows[yx[:, 0] * FW + yx[:, 1]])
            pl = pool[b, side].long()
            cand = unit(rows[pl])
            d = 0.5 * (1.0 - p @ cand.T)
            cy, cx = (pl // FW).float(), (pl % FW).float()
            pd = torch.sqrt((yx[:, :1].float() - cy[None]) ** 2 + (yx[:, 1:].float() - cx[None]) ** 2 + 1e-7)
            j = torch.argmin(d + 1e6 * torch.relu(neg_kernel - pd), dim=1)
            d_neg[b, side] = d.gather(1, j[:, None])[:, 0]
            pos.append(p)
        d_pos[b] = 0.5 * (1.0 - (pos[0] * pos[1]).sum(1))
    return d_pos, d_neg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--corrs", type=int, default=500)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = "cuda"
    rows = []
    for C, S in ((32, 192), (256, 224)):
        g = torch.Generator(device=dev).manual_seed(C)
        B, N = a.pairs, a.corrs
        fa = torch.randn((B, C, S, S), generator=g, device=dev)
        fq = torch.randn((B, C, S, S), generator=g, device=dev)
        corrs = torch.randint(0, S, (B, N, 4), generator=g, device=dev, dtype=torch.int32)
        pool = torch.stack([torch.randperm(S * S, generator=g, device=dev)[:POOL] for _ in range(2 * B)]).reshape(B, 2, POOL).to(torch.int32)
        valid = torch.ones((B,), dtype=torch.int32, device=dev)
        ws = torch.empty((4096,), dtype=torch.uint8, device=dev)
        k_ms, k_all = windows_ms(lambda: ops.feature_loss(fa, fq, corrs, valid, pool, workspace=ws), reps=10)
        out = ops.feature_loss(fa, fq, corrs, valid, pool, workspace=ws)
        t_ms, t_all = windows_ms(lambda: torch_loop(fa, fq, corrs, pool), reps=2, windows=3, warm=1)
        d_pos, d_neg = torch_loop(fa, fq, corrs, pool)
        agree = float((d_neg - out["d_neg"]).abs().max()), float((d_pos - out["d_pos"]).abs().max())
        floss = FeatureLoss(default_args(), dev)
        batch = {"corrs": corrs.long().cpu(), "valid": torch.ones(B), "anchor": {"rgb": torch.zeros(B, 3, S, S), "mask": torch.ones(B, S, S, dtype=torch.uint8)},
                 "query": {"rgb": torch.zeros(B, 3, S, S), "mask": torch.ones(B, S, S, dtype=torch.uint8)}}
        outputs = {"featmap_a": fa, "featmap_q": fq, "mask_a": torch.randn((B, 1, S, S), generator=g, device=dev),
                   "mask_q": torch.randn((B, 1, S, S), generator=g, device=dev)}
        f_ms, f_all = windows_ms(lambda: floss.forward(batch, outputs), reps=3, windows=3, warm=1)
        flop = 2.0 * N * POOL * C * 2 * B
        row = {"C": C, "map": S, "pairs": B, "corrs": N, "pool": POOL, "oryon_feature_loss_ms": round(k_ms, 4), "windows_ms": k_all,
               "FeatureLoss_forward_ms": round(f_ms, 3), "forward_windows_ms": f_all, "torch_loop_ms": round(t_ms, 3), "torch_windows_ms": t_all,
               "max_abs_diff_vs_torch_loop": {"d_neg": agree[0], "d_pos": agree[1]}, "gflop": flop / 1e9,
               "tflops_of_the_call": flop / (k_ms * 1e-3) / 1e12, "pool_gather_bytes_per_pair_and_side": POOL * C * 4}
        print(json.dumps(row))
        rows.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
