#!/usr/bin/env python3
"""Validation driver: the counterpart of the reference's validation loop (Lightning calls `FPM_Pipeline.validation_step` per batch,
pipeline.py:196-247): forward, `FeatureLoss.forward` on the HIP kernels of csrc/feature_loss.hip (positive / hardest-negative / dice mask
loss), the matcher and the solver per pair, the evaluator in validation mode.

    python run_valid.py --pairs 8 --batch 4                      # synthetic pairs (descriptor maps given; ground-truth correspondences
                                                                 # from oryon_amd.synth.pair_gt_corrs)
    python run_valid.py --pairs 8 --batch 4 --debug-valid        # poses from the GROUND-TRUTH correspondences (debug_valid, config.yaml:11)
    python run_valid.py --data-root data --dataset nocs --split cross_scene_test --ckpt ... --pointdsc ... --bpe ...      # a fixed split

It takes the arguments of run_test.py that apply to a validation pass plus `--debug-valid`, builds models and batches with run_test's
own functions, and prints one JSON line last: the three losses and their weighted sum (means over the batches), FMR at
(test.dist_th, 0.05) over the pairs with ground-truth correspondences, and the evaluator's means.

Needs an MI355X (no CPU fallback by design)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--debug-valid", action="store_true", help="debug_valid: solve the pose from the ground-truth correspondences")
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=192, help="feature-map / depth size of the synthetic pairs (reference: 192)")
    ap.add_argument("--channels", type=int, default=32, help="descriptor channels of the synthetic pairs (reference: 32)")
    ap.add_argument("--seed", type=int, default=1)
    g = ap.add_argument_group("real assets (as run_test.py)")
    g.add_argument("--data-root", default=None)
    g.add_argument("--dataset", choices=["nocs", "toyl"], default="nocs")
    g.add_argument("--dataset-name", default=None)
    g.add_argument("--split", default="cross_scene_test")
    g.add_argument("--obj", default="all")
    g.add_argument("--mask", default="predicted")
    g.add_argument("--ckpt", default=None)
    g.add_argument("--catseg", default=None)
    g.add_argument("--pointdsc", default=None)
    g.add_argument("--bpe", default=None)
    g.add_argument("--fp16x3", action="store_true")
    g.add_argument("--hash-prompts", action="store_true")
    return ap.parse_args(argv)


def synthetic_valid_batch(run_test, first, B, H, C, dev, max_corrs):
    """run_test.synthetic_batch plus what the validation step reads on top: ground-truth correspondences in the frame of `rgb` (made
    H x H here, so the rescale of losses.py:77 is the identity), the `valid` flags, and mask logits (+-4 on the generator's masks with
    N(0, 2) noise, so that the predicted masks are good but not perfect)."""
    import torch
    from oryon_amd.synth import pair_gt_corrs
    batch, pairs = run_test.synthetic_batch(first, B, H, C, dev)
    corrs, valid = [], []
    for i in range(B):
        c = pair_gt_corrs(first + i, H, H, max_corrs)
        valid.append(1.0 if c.shape[0] > 0 else 0.0)
        corrs.append(c[torch.arange(max_corrs) % c.shape[0]] if c.shape[0] > 0 else torch.zeros((max_corrs, 4), dtype=torch.long))
    batch["corrs"], batch["valid"] = torch.stack(corrs), torch.tensor(valid)
    g = torch.Generator().manual_seed(3000 + first)
    for side, key in (("anchor", "mask_a"), ("query", "mask_q")):
        batch[side]["rgb"] = torch.zeros(B, 3, H, H)
        m = batch[side]["mask"].float()
        batch[key] = (4.0 * (2.0 * m - 1.0) + 2.0 * torch.randn(m.shape, generator=g))[:, None].to(dev)
    return batch, pairs


def build_solver(args, pointdsc_dir, dev):
    """The PointDSC solver when test.solver asks for one (released weights from `pointdsc_dir`, else bench.py's closed-form ones)."""
    if args.test.solver != "pointdsc":
        return None
    import torch
    if pointdsc_dir:
        from oryon_amd.pointdsc import get_pointdsc_solver
        return get_pointdsc_solver(pointdsc_dir, dev)
    from bench import build_solver as bench_solver
    return bench_solver(torch.device(dev))


def main(argv=None):
    a = parse(argv)
    import oryon_amd
    oryon_amd.configure()
    import torch
    import run_test
    from oryon_amd.pipeline import Pipeline, default_args
    dev = "cuda"
    if a.fp16x3:
        from oryon_amd.backbone import enable_fp16x3
        enable_fp16x3(True)
    if a.data_root:
        from oryon_amd.data import DeviceCollate
        from oryon_amd.datasets import FixedSplit
        from oryon_amd.net import Oryon, default_model_args
        split = FixedSplit(a.dataset, a.data_root, a.dataset_name or a.dataset, a.split, a.obj, mask_type=a.mask)
        margs = default_model_args()
        margs.model.use_catseg_ckpt = False
        torch.manual_seed(0)
        model = Oryon(margs, dev, bpe_path=a.bpe).eval()
        if a.catseg:
            model.load_catseg_checkpoint(a.catseg)
        if a.ckpt:
            run_test.load_oryon_checkpoint(model, a.ckpt)
        args = default_args(**{"test.mask": a.mask, "seed": a.seed, "debug_valid": a.debug_valid})
        pipe = Pipeline(args, model=model, pointdsc_solver=build_solver(args, a.pointdsc, dev))
        collate = DeviceCollate(args.dataset.max_corrs, args.dataset.img_size, dev)
        n = len(split) if a.pairs <= 0 else min(a.pairs, len(split))

        def batches():
            for first in range(0, n, a.batch):
                batch = collate([split[i] for i in range(first, min(first + a.batch, n))])
                if a.hash_prompts:
                    batch["prompt_tokens"] = run_test.hashed_prompt_tokens(batch["prompt"])
                yield batch, {k: split.object_info(k) for k in dict.fromkeys(batch["cls_id"])}
    else:
        H, C = a.size, a.channels
        args = default_args(**{"test.mask": "oracle", "model.image_encoder.img_size": [H, H], "dataset.img_size": [H, H], "seed": a.seed,
                               "debug_valid": a.debug_valid})
        pipe = Pipeline(args, pointdsc_solver=build_solver(args, None, dev))
        n = a.pairs

        def batches():
            for first in range(0, n, a.batch):
                yield synthetic_valid_batch(run_test, first, min(a.batch, n - first), H, C, dev, args.dataset.max_corrs)[0], None
    torch.manual_seed(a.seed)                                # the pool draws of FeatureLoss and the matcher's draws (set_deterministic_seed)
    torch.cuda.manual_seed(a.seed)
    pipe.on_validation_start()
    n_rows = 0
    for i, (batch, objects) in enumerate(batches()):
        if objects is not None:
            pipe.add_validation_objects(objects)
        pipe.validation_step(batch, i)
        n_rows += len(batch["cls_id"])
    torch.cuda.synchronize()
    summary = {"pairs": n_rows, "debug_valid": bool(a.debug_valid), "solver": args.test.solver, "loss_weights": dict(args.loss.w),
               "fmr_thresholds": [args.test.dist_th, 0.05]}
    summary.update(pipe.on_validation_end())
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
