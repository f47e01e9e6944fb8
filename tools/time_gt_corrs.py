"""Time of the ground-truth correspondence search (csrc/gt_corrs.hip) next to the reference's form of it (GPU box).

    python tools/time_gt_corrs.py [--batches 1 8 64] [--sizes 20000 6000] [--ppl N] [--no-cpu] [--json OUT]

For every (B, n) - B pairs of n x n points, n = 20 000 (the reference's cap) and 6 000 (a typical object mask) - measured in ONE process
on one GPU, medians of HIP-event times after warm-up:
  * nearest_ms     oryon_pcd_nearest_f64 alone (the hot path);
  * cdist_ms       torch.cdist in float64 + amin + argmin on the same device, pair after pair (one 3.2 GB matrix at a time): the
                   reference's own form (scripts/data/make_toyl_test.py:68-72) run on the GPU;
  * agree          whether the two pick the same index in every row.
Once: the reference's form on this host's CPU at 20 000 x 20 000 (torch, float64), and the evaluation count B n^2.
--ppl N loads the DEVELOPMENT build (liboryon_hip_dev.so) with N anchor points per lane (1 or 2) in the nearest kernel: the A/B behind
the shipped choice.  Clouds: tests/gt_corrs_restatement.py's bumpy sheet, seeded per pair."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clouds(B, n, seed=0):
    rng = np.random.default_rng(seed)

    def sheet(shift):
        u, v = rng.uniform(-0.05, 0.05, (B, n)), rng.uniform(-0.05, 0.05, (B, n))
        z = 0.8 + 0.01 * np.sin(u * 40.0) + 0.008 * np.cos(v * 55.0)
        return np.stack([u + shift[0], v + shift[1], z + shift[2]], axis=2)
    return sheet((0.0, 0.0, 0.0)), sheet((0.0002, -0.0001, 0.0001))


def median_ms(fn, reps, warm=1):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 6000])
    ap.add_argument("--ppl", type=int, default=0, help="1 | 2: development build with that many anchor points per lane (0 = the shipped library)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the reference's form on the CPU")
    ap.add_argument("--no-cdist", action="store_true", help="skip torch.cdist on the device")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.ppl:
        os.environ["ORYON_GTC_PPL"] = str(a.ppl)
    import torch
    import oryon_amd
    from oryon_amd import _lib
    if a.ppl:
        _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "liboryon_hip_dev.so")
    oryon_amd.configure()
    from oryon_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_gt_corrs.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    rec = dict(device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH), ppl=a.ppl or 1, cases=[])
    for n in a.sizes:
        for B in a.batches:
            s_h, q_h = clouds(B, n, seed=n + B)
            src, dst = torch.from_numpy(s_h).to(dev), torch.from_numpy(q_h).to(dev)
            cnt = torch.full((B,), n, dtype=torch.int32, device=dev)
            idx, _ = ops.pcd_nearest(src, dst, cnt, cnt)
            med, lo, hi = median_ms(lambda: ops.pcd_nearest(src, dst, cnt, cnt), 5 if B * n * n > 4e9 else 11)
            case = dict(B=B, n=n, evaluations=B * n * n, nearest_ms=med, nearest_ms_min_max=[lo, hi])
            if not a.no_cdist:
                def ref_form():
                    out = []
                    for b in range(B):
                        d = torch.cdist(src[b], dst[b], p=2)
                        out.append((torch.amin(d, dim=1), torch.argmin(d, dim=1)))
                    return out
                got = ref_form()
                case["agree"] = bool(all(torch.equal(got[b][1].to(torch.int32), idx[b]) for b in range(B)))
                del got
                med, lo, hi = median_ms(ref_form, 3)
                case["cdist_ms"], case["cdist_ms_min_max"] = med, [lo, hi]
                torch.cuda.empty_cache()
            print(json.dumps(case), flush=True)
            rec["cases"].append(case)
    if not a.no_cpu:
        s_h, q_h = clouds(1, 20000, seed=1)
        s, q = torch.from_numpy(s_h[0]), torch.from_numpy(q_h[0])
        t0 = time.perf_counter()
        d = torch.cdist(s, q, p=2)
        torch.amin(d, dim=1), torch.argmin(d, dim=1)
        rec["cpu_reference_form_20000_s"] = time.perf_counter() - t0
        rec["cpu_threads"] = torch.get_num_threads()
        print(json.dumps({k: rec[k] for k in ("cpu_reference_form_20000_s", "cpu_threads")}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
