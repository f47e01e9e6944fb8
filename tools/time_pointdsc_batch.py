"""PointDSC registration time against the number of pairs per call (the launches are latency-bound at 64 pairs), timed with device
events.  GPU box.

    python tools/time_pointdsc_batch.py [--rows N] [--repeat R] [pairs ...]

--rows: rows per pair (default 500; n_cap is the next multiple of 128, so 500 -> 512 takes pdsc_hyp_fused_kernel<2>, 1152 the
pdsc_seed_dist_kernel<128> + pdsc_knn_matrix_kernel(dist_pre) route and 1280 pdsc_knn_matrix_kernel with its own distances);
--repeat: timed windows of 20 calls per batch size, one line each."""
import argparse, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_solver
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=500)
ap.add_argument("--repeat", type=int, default=1)
ap.add_argument("pairs", type=int, nargs="*", default=[32, 64, 128, 256])
args = ap.parse_args()
n_cap = (args.rows + 127) // 128 * 128
dev = torch.device("cuda", 0)
solver = build_solver(dev)
g = torch.Generator(device=dev).manual_seed(0)
for B in args.pairs:
    src = torch.rand(B, n_cap, 3, generator=g, device=dev)
    tgt = src + 0.01 * torch.randn(B, n_cap, 3, generator=g, device=dev)
    n = torch.full((B,), args.rows, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    for _ in range(3):
        solver.register(src, tgt, n, status)
    for _ in range(args.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            solver.register(src, tgt, n, status)
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 20
        print(f"B={B} rows={args.rows}: {ms:.3f} ms per call, {1e3 * ms / B:.1f} us per pair")
