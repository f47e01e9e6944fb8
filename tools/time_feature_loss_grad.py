"""Time of the training step's loss backward at the reference's training shape (GPU box): 32 pairs, C = 32 on 192 x 192 maps, 500
correspondences, a pool of 2000.

    python tools/time_feature_loss_grad.py [--pairs 32] [--corrs 500] [--json OUT]

Prints, measured in ONE process on one GPU, after warm-up, with HIP events, as the median of several windows of back-to-back calls:
  * oryon_feature_loss_grad (ops.feature_loss_grad with workspace and outputs made beforehand): the two memsets of the maps, the rows
    kernel and the scatter kernel - i.e. the memset is inside the number;
  * oryon_mask_dice_grad for the two logit tensors;
  * the comparison: torch autograd's backward of the per-sample torch statement of the same loss on the same device (gathers, cosine,
    relu, means; the negatives given, the graph built beforehand and retained), which also ends in zero-filled maps;
  * the bytes next to it: the two zero-filled maps (B C H W 4 each) and the workspace of contribution vectors."""
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
from oryon_amd import _lib, ops  # noqa: E402

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


def torch_losses(fa, fq, corrs, neg_idx, pos_margin=0.2, neg_margin=0.9):
    """The per-sample torch statement of the contrastive terms with the negatives given: (pos, neg_a, neg_q), differentiable."""
    F = torch.nn.functional
    B, C, FH, FW = fa.shape
    terms = []
    for b in range(B):
        rows = (fa[b].reshape(C, -1).T, fq[b].reshape(C, -1).T)
        c = corrs[b].long()
        pos = (rows[0][c[:, 0] * FW + c[:, 1]], rows[1][c[:, 2] * FW + c[:, 3]])
        d_pos = 0.5 * (1 - F.cosine_similarity(pos[0], pos[1], dim=1))
        d_neg = [0.5 * (1 - F.cosine_similarity(pos[s], rows[s][neg_idx[b, s].long()], dim=1)) for s in (0, 1)]
        terms.append(torch.stack([F.relu(d_pos - pos_margin).mean(), F.relu(neg_margin - d_neg[0]).mean(), F.relu(neg_margin - d_neg[1]).mean()]))
    return torch.stack(terms).mean(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--corrs", type=int, default=500)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = "cuda"
    B, N, C, S = a.pairs, a.corrs, 32, 192
    g = torch.Generator(device=dev).manual_seed(C)
    fa = torch.randn((B, C, S, S), generator=g, device=dev)
    fq = torch.randn((B, C, S, S), generator=g, device=dev)
    corrs = torch.randint(0, S, (B, N, 4), generator=g, device=dev, dtype=torch.int32)
    pool = torch.stack([torch.randperm(S * S, generator=g, device=dev)[:POOL] for _ in range(2 * B)]).reshape(B, 2, POOL).to(torch.int32)
    valid = torch.ones((B,), dtype=torch.int32, device=dev)
    fwd = ops.feature_loss(fa, fq, corrs, valid, pool)
    gvec = torch.tensor([0.5, 0.25, 0.25], device=dev)
    need = _lib.lib().oryon_feature_loss_grad_workspace_bytes(B, C, N)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    outs = (torch.empty_like(fa), torch.empty_like(fq))
    call = lambda: ops.feature_loss_grad(fa, fq, corrs, valid, fwd["neg_idx"], fwd["d_pos"], fwd["d_neg"], gvec, workspace=ws, out=outs)
    k_ms, k_all = windows_ms(call, reps=10)
    z_ms, z_all = windows_ms(lambda: (outs[0].zero_(), outs[1].zero_()), reps=10)

    logits = torch.randn((B, S, S), generator=g, device=dev)
    gt = (torch.rand((B, S, S), generator=g, device=dev) > 0.5).to(torch.int32)
    sums, _, _ = ops.mask_dice_sums(logits, gt, 0.5)
    gm = torch.tensor([0.5], device=dev)
    gl = torch.empty_like(logits)
    d_ms, d_all = windows_ms(lambda: (ops.mask_dice_grad(logits, gt, sums, gm, out=gl), ops.mask_dice_grad(logits, gt, sums, gm, out=gl)), reps=10)

    ta, tq = fa.clone().requires_grad_(), fq.clone().requires_grad_()
    total = (gvec * torch_losses(ta, tq, corrs, fwd["neg_idx"])).sum()

    def torch_backward():
        ta.grad = tq.grad = None
        total.backward(retain_graph=True)
    t_ms, t_all = windows_ms(torch_backward, reps=2, windows=3, warm=1)
    torch_backward()
    call()
    torch.cuda.synchronize()
    diff = max(float((ta.grad - outs[0]).abs().max()), float((tq.grad - outs[1]).abs().max()))
    row = {"C": C, "map": S, "pairs": B, "corrs": N, "pool": POOL, "oryon_feature_loss_grad_ms": round(k_ms, 4), "windows_ms": k_all,
           "of_which_zero_fill_ms": round(z_ms, 4), "zero_fill_windows_ms": z_all, "oryon_mask_dice_grad_x2_ms": round(d_ms, 4),
           "dice_windows_ms": d_all, "torch_autograd_backward_ms": round(t_ms, 3), "torch_windows_ms": t_all,
           "max_abs_diff_vs_torch_autograd": diff, "largest_gradient": float(outs[0].abs().max()),
           "map_bytes_zeroed": 2 * B * C * S * S * 4, "workspace_bytes": int(need)}
    print(json.dumps(row))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump([row], fh, indent=1)


if __name__ == "__main__":
    main()
