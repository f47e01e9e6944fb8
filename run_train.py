#!/usr/bin/env python3
"""Training driver: the counterpart of the reference's run_train.py (a Lightning Trainer around FPM_Pipeline.training_step,
pipeline.py:100-152, 170-181) without Lightning.  Per epoch: for every batch `Pipeline.training_step` -> `loss.backward()` ->
`optimizer.step()` -> `optimizer.zero_grad()`; the scheduler steps once per epoch; `Pipeline.validation_step` runs over the validation
batches every `training.freq_valid` epochs; a checkpoint is written every `training.freq_save` epochs and after the last one.  The loss
and its backward run on the HIP kernels of csrc/feature_loss.hip and csrc/feature_loss_grad.hip; fusion and decoder - the only trainable
modules - are torch modules under torch autograd.

    python run_train.py --pairs 8 --batch 2 --epochs 2                       # synthetic pairs: images from oryon_amd.synth.pair_rgb, a small
                                                                             # Oryon (small frozen random CLIP towers) trained from scratch
    python run_train.py --data-root data --dataset nocs --split cross_scene_test --ckpt ... --catseg ... --bpe ... --epochs 20 --augs all

A checkpoint is `{"state_dict": {"model.<key>": tensor}, "epoch": e}`: what run_test.load_oryon_checkpoint reads, so a trained model goes
straight into `run_test.py --ckpt` / `run_valid.py --ckpt`.  Files: `<out>/epoch=NNNN.ckpt` and `<out>/last.ckpt`.  The last stdout line
is one JSON line with the per-epoch means of the weighted losses.

`--augs` turns the reference's training augmentations on for the training loader of the real-asset mode (config.yaml's default recipe is
`--augs all`: colour jitter, brightness, horizontal and vertical flip, each with probability 0.5 per image): drawn in the
collate with the reference's calls to `random` and torch's generator, applied inside the resize kernels.  The validation loader never
augments; the synthetic mode builds its batches without the collate and takes `--augs none` only.

Not here: DDP / gradient all-reduce, the text augmentation (augs.text.synset), the lovasz and focal mask losses.

Needs an MI355X (no CPU fallback by design)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SYNTH_SIZE = 192          # the network's output size (net.py: featmap [B,32,192,192]); the synthetic images, masks and depths have it too


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=8, help="training pairs per epoch (real assets: 0 = the whole split)")
    ap.add_argument("--valid-pairs", type=int, default=2, help="validation pairs (synthetic: the pairs after the training ones)")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=None, help="training.n_epochs (config.yaml: 20)")
    ap.add_argument("--freq-valid", type=int, default=None, help="training.freq_valid (config.yaml: 5)")
    ap.add_argument("--freq-save", type=int, default=None, help="training.freq_save (config.yaml: 5)")
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--optim", choices=["Adam", "SGD"], default=None)
    ap.add_argument("--scheduler", choices=["step", "cosine", "exp", "None"], default=None)
    ap.add_argument("--out", default=os.path.join("exp_data", "train", "models"), help="checkpoint directory")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--augs", default="none", help="training augmentations of the real-asset mode: none (default), all, or a comma list of "
                    "jitter,bright,hflip,vflip (augs.rgb.* of config.yaml; with any of them on, Python's `random` is seeded with --seed)")
    g = ap.add_argument_group("real assets (as run_valid.py)")
    g.add_argument("--data-root", default=None)
    g.add_argument("--dataset", choices=["nocs", "toyl"], default="nocs")
    g.add_argument("--dataset-name", default=None)
    g.add_argument("--split", default="cross_scene_test")
    g.add_argument("--valid-split", default=None, help="validation split (default: none, no validation pass)")
    g.add_argument("--obj", default="all")
    g.add_argument("--mask", default="predicted")
    g.add_argument("--ckpt", default=None, help="start from this checkpoint")
    g.add_argument("--catseg", default=None)
    g.add_argument("--pointdsc", default=None)
    g.add_argument("--bpe", default=None)
    g.add_argument("--hash-prompts", action="store_true")
    return ap.parse_args(argv)


AUG_NAMES = ("jitter", "bright", "hflip", "vflip")


def parse_augs(text):
    """--augs -> {name: bool} for the four augs.rgb switches."""
    text = text.strip().lower()
    names = () if text in ("", "none") else AUG_NAMES if text == "all" else tuple(t.strip() for t in text.split(","))
    unknown = [n for n in names if n not in AUG_NAMES]
    if unknown:
        raise SystemExit(f"--augs: unknown augmentation(s) {unknown}; choose none, all or a comma list of {', '.join(AUG_NAMES)}")
    return {n: n in names for n in AUG_NAMES}


def training_args(a, **extra):
    from oryon_amd.pipeline import default_args
    over = {"seed": a.seed}
    for flag, key in ((a.epochs, "training.n_epochs"), (a.freq_valid, "training.freq_valid"), (a.freq_save, "training.freq_save"),
                      (a.lr, "optimization.lr"), (a.optim, "optimization.optim_type"), (a.scheduler, "optimization.scheduler_type")):
        if flag is not None:
            over[key] = flag
    over.update(extra)
    return default_args(**over)


def small_clip_config():
    """Small towers for the synthetic mode: 24 x 24 patch tokens (what fusion and the Swin guidance are built for), one block each."""
    from oryon_amd.backbone.clip import CLIPConfig
    return CLIPConfig(image_size=96, patch=4, v_width=64, v_layers=1, v_heads=2, embed_dim=32, t_width=32, t_layers=1, t_heads=2)


def synthetic_prompt_tokens(B):
    """[B,80,77] token ids of 80 fixed pseudo-templates (the synthetic pairs show no nameable object)."""
    import torch
    toks = torch.randint(1, 49000, (1, 80, 77), generator=torch.Generator().manual_seed(0))
    toks[..., 10] = 49407
    toks[..., 11:] = 0
    return toks.expand(B, 80, 77).contiguous()


def synthetic_train_batch(run_test, first, B, dev, max_corrs):
    """run_valid.synthetic_valid_batch's fields with images a network can learn from (synth.pair_rgb) in place of given descriptor maps:
    what Oryon.forward, FeatureLoss.forward and - for the validation pass - the matcher and the evaluator read."""
    import torch
    import run_valid
    from oryon_amd.synth import pair_rgb
    batch, _ = run_valid.synthetic_valid_batch(run_test, first, B, SYNTH_SIZE, 1, dev, max_corrs)
    for k in ("featmap_a", "featmap_q", "mask_a", "mask_q"):
        del batch[k]
    rgb = [pair_rgb(first + i, SYNTH_SIZE, SYNTH_SIZE) for i in range(B)]
    batch["anchor"]["rgb"] = torch.stack([r[0] for r in rgb]).to(dev)
    batch["query"]["rgb"] = torch.stack([r[1] for r in rgb]).to(dev)
    batch["prompt_tokens"] = synthetic_prompt_tokens(B)
    return batch


def save_checkpoint(model, path, epoch):
    import torch
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    torch.save({"state_dict": {"model." + k: v.detach().cpu() for k, v in model.state_dict().items()}, "epoch": epoch}, path)


def main(argv=None):
    a = parse(argv)
    augs_on = parse_augs(a.augs)
    if any(augs_on.values()) and not a.data_root:
        raise SystemExit("--augs: the synthetic mode builds its batches without the collate and cannot augment them; "
                         "use --augs none, or --data-root ... for the real-asset mode")
    import oryon_amd
    oryon_amd.configure()
    import torch
    import run_test
    import run_valid
    from oryon_amd.net import Oryon, default_model_args
    from oryon_amd.pipeline import Pipeline
    dev = "cuda"
    margs = default_model_args()
    margs.model.use_catseg_ckpt = False
    torch.manual_seed(0)
    valid_batches = None
    if a.data_root:
        from oryon_amd.data import DeviceCollate
        from oryon_amd.datasets import FixedSplit
        args = training_args(a, **{"test.mask": a.mask})
        model = Oryon(margs, dev, bpe_path=a.bpe)
        if a.catseg:
            model.load_catseg_checkpoint(a.catseg)
        if a.ckpt:
            run_test.load_oryon_checkpoint(model, a.ckpt)
        collate = DeviceCollate(args.dataset.max_corrs, args.dataset.img_size, dev)
        train_collate = collate
        if any(augs_on.values()):
            import random
            random.seed(a.seed)                              # the gates of the augmentations (their factors come from torch's generator)
            for name, on in augs_on.items():
                setattr(args.augs.rgb, name, on)
            train_collate = DeviceCollate(args.dataset.max_corrs, args.dataset.img_size, dev, augs=args.augs)

        def loader(split, n_pairs, collate=collate):
            n = len(split) if n_pairs <= 0 else min(n_pairs, len(split))

            def batches():
                for first in range(0, n, a.batch):
                    batch = collate([split[i] for i in range(first, min(first + a.batch, n))])
                    if a.hash_prompts:
                        batch["prompt_tokens"] = run_test.hashed_prompt_tokens(batch["prompt"])
                    yield batch, {k: split.object_info(k) for k in dict.fromkeys(batch["cls_id"])}
            return batches
        train_batches = loader(FixedSplit(a.dataset, a.data_root, a.dataset_name or a.dataset, a.split, a.obj, mask_type=a.mask), a.pairs,
                               train_collate)
        if a.valid_split:
            valid_batches = loader(FixedSplit(a.dataset, a.data_root, a.dataset_name or a.dataset, a.valid_split, a.obj, mask_type=a.mask),
                                   a.valid_pairs)
    else:
        args = training_args(a, **{"test.mask": "predicted", "model.image_encoder.img_size": [SYNTH_SIZE] * 2,
                                   "dataset.img_size": [SYNTH_SIZE] * 2})
        model = Oryon(margs, dev, clip_cfg=small_clip_config())

        def loader(first0, n):
            def batches():
                for first in range(first0, first0 + n, a.batch):
                    yield synthetic_train_batch(run_test, first, min(a.batch, first0 + n - first), dev, args.dataset.max_corrs), None
            return batches
        train_batches = loader(0, a.pairs)
        if a.valid_pairs > 0:
            valid_batches = loader(a.pairs, a.valid_pairs)
    pipe = Pipeline(args, model=model)                      # the pose solver is built when the first validation pass needs it
    (optimizer,), (scheduler,) = pipe.configure_optimizers()
    torch.manual_seed(a.seed)                                # the pool draws of FeatureLoss (set_deterministic_seed)
    torch.cuda.manual_seed(a.seed)
    keys = ("train/mask", "train/pos", "train/neg", "train/loss")
    epochs, written = [], []
    n_epochs = args.training.n_epochs
    for epoch in range(n_epochs):
        sums, n_batches = torch.zeros(len(keys), device=dev), 0
        for i, (batch, _) in enumerate(train_batches()):
            loss, log = pipe.training_step(batch, i)
            loss.backward()
            optimizer.step()
            optimizer.zero_grad(set_to_none=True)
            sums += torch.stack([log[k].float() for k in keys])         # on the device: no host read inside the epoch
            n_batches += 1
        row = {"epoch": epoch, "lr": float(scheduler.get_last_lr()[0]), "batches": n_batches}
        row.update({k: v / max(n_batches, 1) for k, v in zip(keys, sums.tolist())})
        row["Mean IoU"] = pipe.train_evaluator.get_means().get("Mean IoU") if pipe.train_evaluator is not None else None
        scheduler.step()
        if valid_batches is not None and (epoch + 1) % args.training.freq_valid == 0:
            model.eval()
            if pipe.pointdsc_solver is None:
                pipe.pointdsc_solver = run_valid.build_solver(args, a.pointdsc, dev)
            with torch.no_grad():
                pipe.on_validation_start()
                for i, (batch, objects) in enumerate(valid_batches()):
                    if objects is not None:
                        pipe.add_validation_objects(objects)
                    pipe.validation_step(batch, i)
                row["valid"] = pipe.on_validation_end()
        if (epoch + 1) % args.training.freq_save == 0:
            written.append(os.path.join(a.out, f"epoch={epoch:04d}.ckpt"))
            save_checkpoint(model, written[-1], epoch)
        epochs.append(row)
        print(json.dumps(row), flush=True)
    written.append(os.path.join(a.out, "last.ckpt"))
    save_checkpoint(model, written[-1], n_epochs - 1)
    torch.cuda.synchronize()
    summary = {"epochs": epochs, "checkpoints": written, "loss_weights": dict(args.loss.w), "optimizer": args.optimization.optim_type,
               "scheduler": args.optimization.scheduler_type, "trainable_parameters": sum(p.numel() for p in model.get_trainable_parameters())}
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
