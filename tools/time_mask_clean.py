"""Mask clean-up time (ops.mask_clean, csrc/mask_clean.hip): N maps of SIZE x SIZE - the synthetic pairs' anchor and query masks, each
with three small islands away from the object - mode `largest` with hole filling, on the LDS route and on the global route, device
events after a warm-up, the two routes alternating inside one run.  GPU box.

    python tools/time_mask_clean.py [N=128] [SIZE=224] [REPS=12] [PER=10]

Prints one JSON line: per route the median, minimum and maximum over REPS windows of PER calls (REPS x PER >= 100 calls), the launches
per call, and whether the two routes returned identical bytes.  A call includes what ops.mask_clean does around the kernels: three
tensors from torch's caching allocator and the workspace."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oryon_amd import ops  # noqa: E402
from oryon_amd.synth import make_pair  # noqa: E402


def masks(n, size):
    """n maps: mask_a and mask_q of the synthetic pairs 0, 1, .., each with up to three 3 x 3 islands where nothing is near."""
    out = []
    for i in range((n + 1) // 2):
        p = make_pair(i, size, size, 4)
        for k in ("mask_a", "mask_q"):
            m = p[k].numpy().astype(np.int32).copy()
            rng = np.random.default_rng(1000 + 2 * i + (k == "mask_q"))
            placed = 0
            for _ in range(200):
                y, x = (int(v) for v in rng.integers(2, size - 5, 2))
                if placed < 3 and not m[y - 2:y + 5, x - 2:x + 5].any():
                    m[y:y + 3, x:x + 3] = 1
                    placed += 1
            out.append(m)
    return np.stack(out[:n])


def timed(call, per):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(per):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / per


def main(argv):
    n, size, reps, per = (int(a) for a in (argv + ["128", "224", "12", "10"][len(argv):])[:4])
    assert reps * per >= 100, "time at least 100 calls"
    dev = torch.device("cuda", 0)
    m = torch.from_numpy(masks(n, size)).to(dev)
    routes = ["lds", "global"] if size * size <= ops.MASK_CLEAN_LDS_PIXELS else ["global"]
    calls = {r: (lambda r=r: ops.mask_clean(m, mode="largest", fill_holes=True, route=r, want_stats=True)) for r in routes}
    got = {}
    for r, call in calls.items():
        for _ in range(5):
            got[r] = call()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(got[routes[0]], got[routes[-1]]))
    ms = {r: [] for r in routes}
    for _ in range(reps):                                      # alternating: both routes see the same minutes of the box
        for r in routes:
            ms[r].append(timed(calls[r], per))
    stats = got[routes[0]][1].cpu().numpy().astype(np.int64)
    res = {"maps": n, "size": size, "mode": "largest", "fill_holes": True, "calls_per_route": reps * per, "routes_identical": bool(same),
           "removed_pixels_mean": float(stats[:, 4].mean()), "filled_pixels_mean": float(stats[:, 5].mean()), "components_mean": float(stats[:, 0].mean())}
    for r in routes:
        v = sorted(ms[r])
        res[r] = {"launches": 1 if r == "lds" else 8, "ms_per_call": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                  "us_per_map": round(1e3 * v[len(v) // 2] / n, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
