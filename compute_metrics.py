#!/usr/bin/env python3
"""Metrics of a prediction CSV, VSD and AR included: the counterpart of the reference's scripts/evaluation/compute_metrics.py, which
scores the file that its test run wrote with `Evaluator(compute_vsd=True)`.

    python run_test.py --data-root data --dataset nocs --split cross_scene_test --mask predicted ... --out preds/nocs.csv
    python compute_metrics.py preds/nocs.csv --data-root data --dataset nocs --split cross_scene_test --mask predicted

Every pair of the fixed split is read again (oryon_amd.datasets.FixedSplit), its relative pose is taken from the CSV
(`<scene_a> <img_a> <obj>,<scene_q> <img_q> <obj>,<12 floats>[,iou_a,iou_q]`, compute_metrics.py:14-47) and registered as the reference
registers it (:86-115): pred_q = pose_rel @ anchor pose, the query's sensor depth as the VSD test image, an invalid pair as an automatic
failure.  The errors come from the device kernels (oryon_pose_metrics, oryon_pose_bop_errors, oryon_vsd_counts: the model meshes are
rendered by csrc/vsd.hip in place of the BOP toolkit's OpenGL renderer); `--device cpu` uses the numpy statements instead.  Prints the
reference's per-class and overall table rows (AR and VSD filled in), one JSON summary line, and writes the metrics JSON next to the CSV."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def read_predictions(path):
    """instance id -> (pose_rel [4,4], iou_a, iou_q or None) (compute_metrics.py:14-47)."""
    preds = {}
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            tok = line.strip().split(",")
            if len(tok) not in (3, 5):
                raise RuntimeError("Anomaly in line: " + line)
            sa, ia, obj = tok[0].split(" ")
            sq, iq, _ = tok[1].split(" ")
            P = np.eye(4)
            P[:3, :] = np.asarray([float(v) for v in tok[2].split(" ")]).reshape(3, 4)
            iou = (float(tok[3]), float(tok[4])) if len(tok) == 5 else (None, None)
            preds[f"{sa}_{ia}_{sq}_{iq}_{obj}"] = (P, *iou)
    return preds


def compute_metrics(a) -> dict:
    from oryon_amd.datasets import FixedSplit
    from oryon_amd.evaluation import Evaluator, evaluate_batch
    preds = read_predictions(a.csv)
    compute_iou = bool(preds) and all(v[1] is not None for v in preds.values())
    split = FixedSplit(a.dataset, a.data_root, a.dataset_name or a.dataset, a.split, a.obj, mask_type=a.mask)
    evaluator = Evaluator(exp_tag=f"{a.dataset}_{a.split}_{a.mask}", compute_iou=compute_iou, compute_vsd=True)
    device = None if a.device == "cpu" else a.device
    n = len(split) if a.pairs <= 0 else min(a.pairs, len(split))
    for first in range(0, n, a.batch):
        rows = [split[i] for i in range(first, min(first + a.batch, n))]
        ids = [r[7] for r in rows]
        cls = [r[6] for r in rows]
        rel = np.stack([preds[i][0] for i in ids])
        evaluate_batch(evaluator, pred_pose_rel=rel, anchor_pose=np.stack([r[0]["metadata"]["poses"][0].numpy() for r in rows]),
                       gt_pose=np.stack([r[1]["metadata"]["poses"][0].numpy() for r in rows]),
                       K=np.stack([np.asarray(r[1]["camera"], dtype=np.float64).reshape(3, 3) for r in rows]),
                       status=[0 if r[8] else 2 for r in rows], cls_ids=cls, instance_ids=ids,
                       objects={k: split.object_info(k, faces=True) for k in dict.fromkeys(cls)},
                       iou_a=[preds[i][1] for i in ids] if compute_iou else None, iou_q=[preds[i][2] for i in ids] if compute_iou else None,
                       device=device, depth=[np.asarray(r[1]["orig_depth"], dtype=np.float32).squeeze() for r in rows])
    if n == 0:
        print(json.dumps({"pairs": 0, "csv": a.csv, "note": "the split / filter selected no pair: nothing to evaluate"}))
        return {"pairs": 0}
    metric_file = os.path.splitext(a.csv)[0] + ".json"
    with open(metric_file, "w") as f:
        evaluator.save(f)
    for line in evaluator.test_summary():
        print(line)
    latex = evaluator.get_latex_str()
    print(latex, end="")
    means = evaluator.get_means()
    summary = {"dataset": a.dataset, "split": a.split, "obj": a.obj, "mask": a.mask, "pairs": n, "csv": a.csv, "metrics_json": metric_file,
               "AR": means["AR"], "VSD": means["VSD"], "MSSD": means["MSSD"], "MSPD": means["MSPD"], "ADD(S)-0.1d": means["ADD(S)-0.1d"],
               "Mean IoU": means.get("Mean IoU"), "latex_row": latex.strip(), "device": a.device}
    print(json.dumps(summary))
    return summary


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("csv", help="prediction file written by run_test.py --out (or by the reference)")
    ap.add_argument("--data-root", required=True, help="dataset.root")
    ap.add_argument("--dataset", choices=["nocs", "toyl"], default="nocs")
    ap.add_argument("--dataset-name", default=None, help="dataset.test.name (sub-folder of --data-root; default = --dataset)")
    ap.add_argument("--split", default="cross_scene_test")
    ap.add_argument("--obj", default="all")
    ap.add_argument("--mask", default="predicted")
    ap.add_argument("--pairs", type=int, default=0, help="first N pairs of the split only (0 = all)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--device", default="cuda", help="'cuda' (HIP kernels) or 'cpu' (numpy statements)")
    return compute_metrics(ap.parse_args(argv))


if __name__ == "__main__":
    main()
