"""ICP refinement time (ops.icp_refine, csrc/icp.hip): B pairs of N x N points, ITERS forced iterations (tolerance = 0: no pair
finishes early), device events after a warm-up.  GPU box.

    python tools/time_icp.py [B=64] [N=2048] [ITERS=20] [--mode icp|plane|verify]

`--mode plane`: point-to-plane ICP on the depth map instead (ops.icp_plane_refine, csrc/icp_plane.hip): B pairs of N source rows onto
480 x 640 depth maps, ITERS forced iterations - 2 ITERS + 1 small launches, no candidate search.

`--mode verify`: depth-consistency verification (ops.pose_verify, csrc/pose_verify.hip) of K = 2 candidate poses per pair - the start
pose of `--mode plane` and the identity, which is the truth here - on the same inputs: two launches per call, ITERS is not used.

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


def plane_inputs(B, N, dev, H=480, W=640, seed=0):
    """A smooth bumpy surface ~0.9 m away filling the map, an elliptic object mask, and N sub-pixel samples of the object as the source;
    the start pose is 2 degrees and 5 mm off and every row is kept at every forced iteration: the full cost of a row, every time."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    surf = lambda x, y: 900.0 + 30.0 * np.sin(0.02 * x + 0.3) * np.cos(0.017 * y) + 0.05 * x + 15.0 * np.cos(0.03 * (x + y))
    depth = surf(xx, yy).astype(np.float32)
    mask = (((xx - W / 2) / (0.3 * W)) ** 2 + ((yy - H / 2) / (0.3 * H)) ** 2 <= 1.0).astype(np.int32)
    f, cx, cy = 600.0, W / 2 - 0.5, H / 2 - 0.5
    r, a = np.sqrt(rng.uniform(0, 1, (B, N))) * 0.29, rng.uniform(0, 2 * np.pi, (B, N))
    x, y = W / 2 + r * W * np.cos(a), H / 2 + r * H * np.sin(a)
    z = surf(x, y)
    src = np.stack([(x - cx) * z / f / 1000.0, (y - cy) * z / f / 1000.0, z / 1000.0], axis=-1)
    c = src.reshape(-1, 3).mean(axis=0)
    ang = np.deg2rad(2.0)
    T0 = np.eye(4)
    T0[:3, :3] = np.array([[np.cos(ang), 0.0, np.sin(ang)], [0.0, 1.0, 0.0], [-np.sin(ang), 0.0, np.cos(ang)]])
    T0[:3, 3] = c - T0[:3, :3] @ c + np.array([0.003, -0.003, 0.003])
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v)).to(dt).to(dev)
    cam9 = np.tile(np.array([f, 0.0, cx, 0.0, f, cy, 0.0, 0.0, 1.0]), (B, 1))
    return (t(src, torch.float64), t(np.tile(depth, (B, 1, 1)), torch.float32), t(np.tile(mask, (B, 1, 1)), torch.int32), t(cam9, torch.float64),
            t(np.tile(T0, (B, 1, 1)), torch.float32))


def main_plane(B, N, iters):
    dev = torch.device("cuda", 0)
    src, depth, mask, cam9, T0 = plane_inputs(B, N, dev)
    n = torch.full((B,), N, dtype=torch.int32, device=dev)
    ws = torch.empty((max(ops.lib().oryon_icp_plane_workspace_bytes(B, N), 256),), dtype=torch.uint8, device=dev)
    call = lambda: ops.icp_plane_refine(src, n, depth, mask, cam9, T0, max_iter=iters, tolerance=0.0, workspace=ws)
    for _ in range(3):
        out = call()
    torch.cuda.synchronize()
    assert int(out["iters"].min()) == iters, "tolerance = 0 forces every iteration"
    ms = timed(call)
    med = ms[len(ms) // 2]
    print(json.dumps({"mode": "plane", "B": B, "N": N, "map": [480, 640], "iters": iters, "launches": 2 * iters + 1, "ms_per_call": round(med, 4),
                      "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "us_per_pair": round(1e3 * med / B, 2),
                      "us_per_launch": round(1e3 * med / (2 * iters + 1), 2), "n_kept_first_pair": int(out["n_kept"][0]),
                      "mean_err_first_pair": float(out["mean_err"][0])}))


def main_verify(B, N, K=2):
    dev = torch.device("cuda", 0)
    src, depth, mask, cam9, T0 = plane_inputs(B, N, dev)
    n = torch.full((B,), N, dtype=torch.int32, device=dev)
    poses = torch.stack([T0, torch.eye(4, dtype=torch.float32, device=dev).expand(B, 4, 4)], dim=1).contiguous()
    ws = torch.empty((max(ops.lib().oryon_pose_verify_workspace_bytes(B, N, K), 256),), dtype=torch.uint8, device=dev)
    call = lambda: ops.pose_verify(src, n, depth, mask, cam9, poses, tol=0.01, workspace=ws)
    for _ in range(3):
        out = call()
    torch.cuda.synchronize()
    assert (out["counts"].sum(dim=2) == N).all(), "every row has one class"
    ms = timed(call)
    med = ms[len(ms) // 2]
    print(json.dumps({"mode": "verify", "B": B, "N": N, "K": K, "map": [480, 640], "launches": 2, "ms_per_call": round(med, 4),
                      "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "us_per_pair": round(1e3 * med / B, 2),
                      "counts_first_pair": out["counts"][0].cpu().tolist(), "best_first_pair": int(out["best"][0])}))


def timed(call, reps=7, per=10):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / per)
    return sorted(ms)


def main(argv):
    mode = "icp"
    if "--mode" in argv:
        at = argv.index("--mode")
        mode, argv = argv[at + 1], argv[:at] + argv[at + 2:]
    if mode not in ("icp", "plane", "verify"):
        raise SystemExit("--mode icp|plane|verify")
    B, N, iters = (int(a) for a in (argv + ["64", "2048", "20"][len(argv):])[:3])
    if mode == "plane":
        return main_plane(B, N, iters)
    if mode == "verify":
        return main_verify(B, N)
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
    ms = timed(call)
    med = ms[len(ms) // 2]
    print(json.dumps({"B": B, "N": N, "iters": iters, "ms_per_call": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                      "us_per_pair": round(1e3 * med / B, 2), "candidates_per_s": round(B * iters * N * N / (med * 1e-3), -6),
                      "estimate_ms_at_64x2048x20": 1.0, "mean_err_first_pair": float(out["mean_err"][0])}))


if __name__ == "__main__":
    main(sys.argv[1:])
