"""Time of the RANSAC pose solver at the workload's size: 64 pairs x 500 correspondences x 10 000 iterations (GPU box).

    python tools/time_ransac.py [--pairs 64] [--rows 500] [--iters 10000] [--json OUT]

Prints, measured in ONE process on one GPU:
  * stand-alone: oryon_ransac_register per call (HIP events around 20 back-to-back calls, after warm-up) and its scoring kernel alone
    (the HIP events of oryon_profile_events around ransac_score_kernel, median of 10);
  * 64 PointDSC registrations (12 x 128, the bench's solver) on the same points, the same way;
  * inside the engine step: the registration section of oryon_engine_timing for solver = ransac and solver = pointdsc, and the step time;
  * the float64 numpy restatement of one pair on this host's CPU (tests/ransac_restatement.py).  The reference's own function can only be
    timed where the reference exists: tools/gen_goldens.py gen_ransac prints its time on fixture 7 (same n, same K) next to the
    restatement's on that host, which ties the two CPU figures together;
  * the yardstick: n*K*B point tests x VALU_PER_TEST fp32 VALU instructions (counted in the scoring loop's disassembly) at the chip's
    fp32 VALU issue rate (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz).
Point sets: 60 % inliers with 2e-5 m noise, outliers uniform in the box - fixture 7's recipe, seeded per pair."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oryon_amd  # noqa: E402

oryon_amd.configure()
from oryon_amd import ops  # noqa: E402
from oryon_amd._lib import lib  # noqa: E402
from oryon_amd.engine import MatchPoseConfig, MatchPoseEngine  # noqa: E402

# fp32 VALU instructions per (hypothesis, point) in ransac_score_kernel's row loop.  Recount after any change of that loop:
#   hipcc (the Makefile's CXXFLAGS) --save-temps -c oryon_amd/csrc/ransac.hip, open ransac-hip-amdgcn-amd-amdhsa-gfx950.s, find the
#   "Inner Loop Header" inside ransac_score_kernel that holds ds_read2_b64, and count the v_* lines of ONE of its four unrolled copies up
#   to the s_cbranch_execz that skips the fp64 fallback (9 fma/fmac + 3 sub for the residual, 3 for the square sum, 3 compares, the
#   count's add-with-carry and one address move = 20).
VALU_PER_TEST = 20
CHIP_LANE_RATE = 256 * 4 * 16 * 2.4e9


def points(B, n, n_cap, seed=0):
    g = np.random.default_rng(seed)
    src = np.zeros((B, n_cap, 3), np.float32)
    tgt = np.zeros((B, n_cap, 3), np.float32)
    for b in range(B):
        A = g.uniform(-0.15, 0.15, (n, 3))
        q = g.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        t = np.array([g.uniform(-0.2, 0.2), g.uniform(-0.2, 0.2), g.uniform(0.4, 0.7)])
        Bm = A @ R.T + t + g.normal(0.0, 2e-5, (n, 3))
        out = g.permutation(n)[: int(0.4 * n)]
        Bm[out] = t + g.uniform(-0.15, 0.15, (len(out), 3))
        src[b, :n], tgt[b, :n] = A, Bm
    return src, tgt


def events_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rows", type=int, default=500)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_ransac.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    B, n, K = a.pairs, a.rows, a.iters
    n_cap = ops.round_up(n, 128)
    src_h, tgt_h = points(B, n, n_cap)
    src, tgt = torch.from_numpy(src_h).to(dev), torch.from_numpy(tgt_h).to(dev)
    nn = torch.full((B,), n, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    ws = torch.empty((lib().oryon_ransac_workspace_bytes(B, n_cap, K),), dtype=torch.uint8, device=dev)
    rec = dict(pairs=B, rows=n, iters=K, device=torch.cuda.get_device_name(0))

    run = lambda: ops.ransac_register(src, tgt, nn, K, 0.001, 0.9999, None, 1, None, status, workspace=ws)
    out = run()
    rec["winner_counts_ok"] = bool((out["winner"] >= 0).all())
    rec["ransac_call_ms"] = events_ms(run, 20)
    ks = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); e1.record()
        lib().oryon_profile_events(e0.cuda_event, e1.cuda_event)
        run()
        torch.cuda.synchronize()
        ks.append(e0.elapsed_time(e1))
    rec["ransac_score_kernel_ms"] = sorted(ks)[len(ks) // 2]
    rec["ransac_score_kernel_ms_min_max"] = [min(ks), max(ks)]
    rec["valu_floor_ms"] = 1e3 * n * K * B * VALU_PER_TEST / CHIP_LANE_RATE

    from bench import build_solver
    solver = build_solver(dev)
    rec["pointdsc_call_ms"] = events_ms(lambda: solver.register(src, tgt, nn, status), 20)

    # inside the engine step (cfg2-like synthetic maps at the reference's 192^2, C = 32)
    from oryon_amd.synth import make_batch
    H, C = 192, 32
    mb = make_batch(0, B, H, H, C, device=dev)
    cam = mb["camera"].to(dev)
    for name, slv in (("ransac", None), ("pointdsc", solver)):
        eng = MatchPoseEngine(slv, MatchPoseConfig(solver=name, ransac_max_iter=K), overlap_registration=True, overlap_gather=True,
                              result_views=True)
        eng.native_timing = True
        step = lambda: eng.finish(eng.run(mb["feat_a"], mb["feat_q"], mb["mask_a"], mb["mask_q"], mb["depth_a"], mb["depth_q"], cam, cam,
                                          inputs_resident=True))
        for _ in range(4):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 16
        for _ in range(reps):
            step()
        torch.cuda.synchronize()
        rec[f"engine_{name}_step_ms"] = (time.perf_counter() - t0) / reps * 1e3
        nat = eng._native
        regs = sorted(nat.timing(s)["registration_ms"] for s in range(nat.steps - 8, nat.steps))
        rec[f"engine_{name}_registration_ms"] = regs[len(regs) // 2]
        del eng

    import ransac_restatement as rr
    A64, B64 = src_h[0, :n].astype(np.float64), tgt_h[0, :n].astype(np.float64)
    np.random.seed(0)
    idx = np.random.randint(0, n, (K, 4))
    t0 = time.perf_counter()
    r = rr.restate(A64, B64, idx, K, 0.001, 0.9999)
    rec["cpu_restatement_one_pair_s"] = time.perf_counter() - t0
    rec["cpu_restatement_winner_count"] = int(r["counts"][r["winner"]]) if r["winner"] >= 0 else 0
    for k, v in rec.items():
        print(f"{k}: {v}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
