#!/usr/bin/env python3
"""Time of the augmenting rgb resize (oryon_rgb_augment_resize, K-1a: both launches, all four augmentations live on every image)
against the plain one (oryon_rgb_resize_bilinear) for 32 images 480x640 -> 224x224 on one MI355X (DESIGN.md §7b quotes the result).

Both are called through the C ABI on preallocated buffers (no allocation inside the window).  One window = `--calls` back-to-back
calls between two HIP events on the launch stream; the two kernels alternate, `--windows` windows each, the median is reported with
the spread.  `host_us` is the host time of one enqueue in the same window: where it is close to the event time the window measures
the enqueue rate, not the kernel.  Prints one JSON line.

    python tools/bench_augment.py [--images 32] [--calls 2000] [--windows 7]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args(argv)
    import oryon_amd
    oryon_amd.configure()
    import torch
    from oryon_amd import _lib, augment
    from oryon_amd._lib import check, lib, ptr, stream_ptr
    dev = _lib.require_gpu("cuda")
    n, HI, WI, HO, WO = a.images, 480, 640, 224, 224
    g = torch.Generator().manual_seed(0)
    rgb = torch.randint(0, 256, (n, HI, WI, 3), dtype=torch.uint8, generator=g).to(dev)
    # every image: jitter (a different permutation per image, all four factors) then bright, both flips
    perms = [(0, 1, 2, 3), (1, 0, 2, 3), (3, 2, 1, 0), (2, 3, 0, 1)]
    params = [augment.AugParams(jitter=augment.ColorApplication(perms[i % 4], (1.1, 0.7 + 0.01 * i, 1.4, 0.03 if i % 2 else -0.03)),
                                bright=augment.ColorApplication((0, 1, 2, 3), (0.8 + 0.01 * i, None, None, None)), hflip=True, vflip=True)
              for i in range(n)]
    table = augment.build_table(params).to(dev)
    out = torch.empty((n, 3, HO, WO), dtype=torch.float32, device=dev)
    ws_bytes = int(lib().oryon_rgb_augment_workspace_bytes(n))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=dev)
    L, st = lib(), stream_ptr(dev)

    def plain():
        check(L.oryon_rgb_resize_bilinear(ptr(rgb), n, HI, WI, HO, WO, ptr(out), st), "oryon_rgb_resize_bilinear")

    def augmented():
        check(L.oryon_rgb_augment_resize(ptr(rgb), ptr(table), n, HI, WI, HO, WO, ptr(ws), ws_bytes, ptr(out), st), "oryon_rgb_augment_resize")

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        host = time.perf_counter() - t0
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls, host * 1e6 / a.calls

    for fn in (plain, augmented):
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {"plain": [], "augmented": []}
    for _ in range(a.windows):
        times["plain"].append(window(plain))
        times["augmented"].append(window(augmented))
    res = {"images": n, "shape": [HI, WI, HO, WO], "calls_per_window": a.calls, "windows": a.windows}
    for k, v in times.items():
        us = sorted(t[0] for t in v)
        res[k] = {"us_per_call": round(statistics.median(us), 2), "min": round(us[0], 2), "max": round(us[-1], 2),
                  "host_us": round(statistics.median(t[1] for t in v), 2)}
    res["ratio"] = round(res["augmented"]["us_per_call"] / res["plain"]["us_per_call"], 3)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
