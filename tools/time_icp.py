"""ICP refinement time (ops.icp_refine, csrc/icp.hip): B pairs of N x N points, ITERS forced iterations (tolerance = 0: no pair
finishes early), device events after a warm-up.  GPU box.

    python tools/time_icp.py [B=64] [N=2048] [ITERS=20]

Prints one JSON line: ms per call (median and spread over the repeats), the candidate evaluations per second, and - for scale - the
estimate DESIGN.md "ICP refinement" started from (B ITERS N^2 candidates at ~8 float64 VALU instructions each at the unpacked vector
rate: about 1 ms at 64 x 2048 x 20)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oryon_amd import ops  # noqa: E402


def clouds(B, N, dev, seed=0):
    """Object-sized clouds (~10 x 6 x 4 cm, 0.9 m away), the target a moved, independently sampled image of the same surface."""
    rng = np.random.default_rng(seed)

    def cloud():
        u = rng.normal(size=(B, N, 3)) * np.array([0.05, 0.03, 0.02])
        u[..., 2] += 0.01 * np.sin(u[..., 0] * 60.0) + 0.008 * np.cos(u[..., 1] * 45.0)
        return u
    src, dst = cloud() + np.array([0.05, -0.03, 0.9]), cloud()
    a = 0.2
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    dst = dst @ Rz.T + np.array([0.06, -0.025, 0.905])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t(src), t(dst)


def main(argv):
    B, N, iters = (int(a) for a in (argv + ["64", "2048", "20"][len(argv):])[:3])
    dev = torch.device("cuda", 0)
    src, dst = clouds(B, N, dev)
    n = torch.full((B,), N, dtype=torch.int32, device=dev)
    T0 = torch.eye(4, dtype=torch.float32, device=dev).repeat(B, 1, 1).contiguous()
    need = ops.lib().oryon_icp_workspace_bytes(B, N, N)
    ws = torch.empty((max(need, 256),), dtype=torch.uint8, device=dev)
    call = lambda: ops.icp_refine(src, dst, n, n, T0, max_iter=iters, tolerance=0.0, workspace=ws)
    for _ in range(3):
        out = call()
    torch.cuda.synchronize()
    assert int(out["iters"].min()) == iters, "tolerance = 0 forces every iteration"
    reps, per = 7, 10
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / per)
    ms.sort()
    med = ms[len(ms) // 2]
    print(json.dumps({"B": B, "N": N, "iters": iters, "ms_per_call": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                      "us_per_pair": round(1e3 * med / B, 2), "candidates_per_s": round(B * iters * N * N / (med * 1e-3), -6),
                      "estimate_ms_at_64x2048x20": 1.0, "mean_err_first_pair": float(out["mean_err"][0])}))


if __name__ == "__main__":
    main(sys.argv[1:])
