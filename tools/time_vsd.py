#!/usr/bin/env python3
"""Time VSD on 64 pairs at 640 x 480: evaluate_batch with compute_vsd on the device, the numpy path on a few pairs of the same batch,
and the rasteriser's share (ops.render_depth of the same 128 images) - with the golden's meshes and with one dense mesh (icosphere
level 6, 81920 faces, the size of a BOP model).  Prints one JSON line.

    python tools/time_vsd.py [--pairs 64] [--numpy-pairs 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oryon_amd import evaluation as ev, ops, synth  # noqa: E402


def _timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def measure(tag, objs, cls, n, numpy_pairs):
    gt8, pred8 = synth.vsd_poses()
    keep = [i for i in range(8) if i != 5]                  # the pair behind the camera renders nothing: leave it out of a timing
    gt, pred = np.stack([gt8[keep[i % 7]] for i in range(n)]), np.stack([pred8[keep[i % 7]] for i in range(n)])
    K = np.tile(np.array(synth.VSD_K), (n, 1, 1))
    for o in objs.values():
        o["syms"] = ev.format_sym_set(ev.get_symmetry_transformations({}))
    names = list(objs)
    verts = torch.from_numpy(np.concatenate([objs[k]["pts"] for k in names])).cuda()
    faces = torch.from_numpy(np.concatenate([objs[k]["faces"] for k in names])).cuda()
    vo = torch.tensor(np.concatenate(([0], np.cumsum([objs[k]["pts"].shape[0] for k in names]))), dtype=torch.int32)
    fo = torch.tensor(np.concatenate(([0], np.cumsum([objs[k]["faces"].shape[0] for k in names]))), dtype=torch.int32)
    which = torch.tensor([names.index(c) for c in cls], dtype=torch.int32)
    P = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    for i in range(n):
        R, t = ev._pose_f16_mm(gt[i])
        P[i, :3, :3], P[i, :3, 3] = R, t[:, 0]
    Pd, Kd = torch.from_numpy(P).cuda(), torch.from_numpy(K).cuda()
    depth_gt = ops.render_depth(Pd, Kd, verts, faces, synth.VSD_H, synth.VSD_W, vo, fo, which)
    _, routes = ops.render_depth(Pd, Kd, verts, faces, synth.VSD_H, synth.VSD_W, vo, fo, which, return_route_counts=True)
    depth = [synth.vsd_test_depth(d) for d in depth_gt.cpu().numpy()]
    depth_d = torch.from_numpy(np.stack(depth)).cuda()
    diam = torch.tensor([objs[c]["diameter"] for c in cls], dtype=torch.float64).cuda()
    args = dict(pred_pose_rel=pred, anchor_pose=np.tile(np.eye(4), (n, 1, 1)), gt_pose=gt, K=K, status=[0] * n, cls_ids=cls,
                instance_ids=[str(i) for i in range(n)], objects=objs, iou_a=np.ones(n), iou_q=np.ones(n))
    t_eval_vsd = _timed(lambda: ev.evaluate_batch(ev.Evaluator("t", compute_vsd=True), device="cuda", depth=depth, **args), 3)
    t_eval = _timed(lambda: ev.evaluate_batch(ev.Evaluator("t"), device="cuda", **args), 3)
    pd_, gd_ = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    t_counts = _timed(lambda: ops.vsd_counts(pd_, gd_, Kd, depth_d, verts, faces, diam, vo, fo, which))
    P2, K2, w2 = torch.cat([Pd, Pd]), torch.cat([Kd, Kd]), torch.cat([which, which])
    t_render = _timed(lambda: ops.render_depth(P2, K2, verts, faces, synth.VSD_H, synth.VSD_W, vo, fo, w2))
    m = min(numpy_pairs, n)
    t0 = time.perf_counter()
    sub = {k: (v[:m] if not isinstance(v, dict) else v) for k, v in args.items()}
    ev.evaluate_batch(ev.Evaluator("t", compute_vsd=True), depth=depth[:m], **sub)
    t_numpy = (time.perf_counter() - t0) / m
    return {"case": tag, "pairs": n, "faces": {k: int(objs[k]["faces"].shape[0]) for k in names},
            "triangles_wave_route": routes[0], "triangles_thread_route": routes[1],
            "evaluate_batch_vsd_ms_per_pair": 1e3 * t_eval_vsd / n, "evaluate_batch_no_vsd_ms_per_pair": 1e3 * t_eval / n,
            "vsd_counts_us_per_pair": 1e6 * t_counts / n, "render_2n_images_us_per_pair": 1e6 * t_render / n,
            "numpy_evaluate_batch_vsd_ms_per_pair": 1e3 * t_numpy, "numpy_pairs_timed": m}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--numpy-pairs", type=int, default=2)
    a = ap.parse_args()
    objs = synth.vsd_objects()
    keep = [c for i, c in enumerate(synth.VSD_CLS) if i != 5]
    out = [measure("golden meshes", objs, [keep[i % 7] for i in range(a.pairs)], a.pairs, a.numpy_pairs)]
    v, f = synth.icosphere(6)
    dense = {"ico6": {"pts": v, "faces": f, "diameter": 120.0}}
    out.append(measure("icosphere level 6", dense, ["ico6"] * a.pairs, a.pairs, min(a.numpy_pairs, 1)))
    print(json.dumps(out))
