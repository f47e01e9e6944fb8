"""Time of the spectral pose solver at the workload's size: 64 pairs x 500 correspondences in buffers of 512 rows (GPU box).

    python tools/time_spectral.py [--pairs 64] [--rows 500] [--json OUT]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUTDIR -o spectral -- python tools/time_spectral.py --trace-only 20

Prints, measured in ONE process on one GPU, each as the median of 7 windows of 20 back-to-back calls between two HIP events, after a
warm-up of every shape:
  * oryon_spectral_register (defaults: 10 iterations, k = 40, 1 cm thresholds);
  * oryon_ransac_register on the same points (10 000 iterations, the reference's arguments);
  * PointDSC.register (12 x 128, the bench's solver) on the same points;
and the pose errors of the three against the planted motions, so that a time is never read without what it bought.
--trace-only N: N calls of oryon_spectral_register after a warm-up and nothing else - the run to put under rocprofv3 (second line
above) for per-kernel times; tracing slows the host, so end-to-end figures come from the first form only.
Point sets: tests/spectral_restatement.planted - uniform points in a 0.3 m cube, a planted rigid motion, 1 mm noise, 80 % of the rows
replaced by random points - seeded per pair."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oryon_amd  # noqa: E402

oryon_amd.configure()
from oryon_amd import ops  # noqa: E402
from oryon_amd._lib import lib  # noqa: E402

WINDOWS, CALLS = 7, 20


def window_ms(fn, calls=CALLS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def median_ms(fn, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ws = sorted(window_ms(fn) for _ in range(WINDOWS))
    return ws[len(ws) // 2], ws[0], ws[-1]


def errors(T, truth):
    import spectral_restatement as sr
    e = [sr.pose_error(T[b].double().cpu().numpy(), G) for b, G in enumerate(truth)]
    return dict(rot_deg_median=float(np.median([x[0] for x in e])), rot_deg_max=float(max(x[0] for x in e)),
                trans_mm_max=float(max(x[1] for x in e) * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--outliers", type=float, default=0.8)
    ap.add_argument("--trace-only", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_spectral.py measures on the GPU: no device found")
    import spectral_restatement as sr
    dev = torch.device("cuda", 0)
    B, n = a.pairs, a.rows
    n_cap = ops.round_up(n, 128)
    src_h, tgt_h, truth = np.zeros((B, n_cap, 3), np.float32), np.zeros((B, n_cap, 3), np.float32), []
    for b in range(B):
        s, t, G, _ = sr.planted(n, a.outliers, 1000 + b)
        src_h[b, :n], tgt_h[b, :n] = s, t
        truth.append(G)
    src, tgt = torch.from_numpy(src_h).to(dev), torch.from_numpy(tgt_h).to(dev)
    nn = torch.full((B,), n, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    cfg = ops.spectral_config()
    import ctypes
    ws = torch.empty((lib().oryon_spectral_workspace_bytes(ctypes.byref(cfg), B, n_cap),), dtype=torch.uint8, device=dev)
    spectral = lambda: ops.spectral_register(src, tgt, nn, status, workspace=ws)
    if a.trace_only:
        for _ in range(3):
            spectral()
        torch.cuda.synchronize()
        for _ in range(a.trace_only):
            spectral()
        torch.cuda.synchronize()
        print(f"trace-only: {a.trace_only} calls of oryon_spectral_register, {B} pairs x {n} rows")
        return
    rec = dict(pairs=B, rows=n, n_cap=n_cap, outliers=a.outliers, device=torch.cuda.get_device_name(0), windows=WINDOWS, calls_per_window=CALLS,
               workspace_MiB=ws.numel() / 2 ** 20)
    rec["spectral_call_ms"], rec["spectral_call_ms_min"], rec["spectral_call_ms_max"] = median_ms(spectral)
    rec["spectral_errors"] = errors(spectral()["T"], truth)
    rws = torch.empty((lib().oryon_ransac_workspace_bytes(B, n_cap, 10000),), dtype=torch.uint8, device=dev)
    ransac = lambda: ops.ransac_register(src, tgt, nn, 10000, 0.001, 0.9999, None, 1, None, status, workspace=rws)
    rec["ransac_call_ms"], rec["ransac_call_ms_min"], rec["ransac_call_ms_max"] = median_ms(ransac)
    rec["ransac_errors"] = errors(ransac()["T"], truth)
    from bench import build_solver
    solver = build_solver(dev)
    pointdsc = lambda: solver.register(src, tgt, nn, status)
    rec["pointdsc_call_ms"], rec["pointdsc_call_ms_min"], rec["pointdsc_call_ms_max"] = median_ms(pointdsc)
    rec["pointdsc_errors"] = errors(pointdsc()[0], truth)
    for k, v in rec.items():
        print(f"{k}: {v}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
