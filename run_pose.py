#!/usr/bin/env python3
"""The test driver with the pose solver on the command line (test.solver of the reference's configs/config.yaml:57).

    python run_pose.py --solver ransac [every argument of run_test.py]
    python run_pose.py --solver ransac --pairs 8 --batch 4
    python run_pose.py --solver ransac --data-root /data --dataset nocs --ckpt ... --bpe ...       # no --pointdsc snapshot needed

`--solver {pointdsc,ransac,spectral}` (default pointdsc) becomes the process-wide default solver (oryon_amd.engine.set_default_solver): every
`default_args()` and `MatchPoseConfig()` that run_test.py builds - the per-sample loop, the batched engine, its --half-descriptors
engine - then selects it.  Everything else goes to run_test.py unchanged.  With `ransac` (best_fit_transform_with_RANSAC,
utils/geo6d.py:75-120, max_iter=10000, fix_percent=0.9999, match_err=0.001 as pipeline.py:463) no PointDSC weights take part in a pose.

With `spectral` (csrc/spectral.hip: spectral matching and second-order spatial compatibility in front of PointDSC's hypothesis and
refinement kernels) no weights and no random numbers take part either; its thresholds (test.spectral_*) are object-scale defaults
chosen on synthetic data only.

    python run_pose.py --solver spectral --pairs 8 --batch 4
    python run_pose.py --solver ransac --refine icp --pairs 8

`--refine {none,icp,icp_plane}` (default none; test.refine) becomes the process-wide default refinement (oryon_amd.pipeline.set_default_refine),
which every Pipeline that run_test.py builds then applies: every solved pose is refined by ICP of the anchor's object cloud onto the
query's (utils/geo6d.py:157-208 `icp`, csrc/icp.hip), in the per-sample loop and behind the batched engine alike; `icp_plane` refines it
by point-to-plane ICP of that cloud onto the query's depth map instead (projective association, csrc/icp_plane.hip).

    python run_pose.py --solver ransac --mutual --pairs 8 --batch 4

`--mutual` (test.mutual; off by default) becomes the process-wide default (oryon_amd.engine.set_default_mutual), so every
`default_args()` and `MatchPoseConfig()` that run_test.py builds selects it: the matcher runs in both directions in one fused scan
(csrc/match_mutual.hip) and only the mutual nearest neighbours reach the solver.  run_test.py never sees the flag; the summary this
driver returns - and prints as its last JSON line - carries `"mutual": true`.

    python run_pose.py --solver ransac --ratio 0.8 --ratio-radius 5 --pairs 8 --batch 4

`--ratio R [--ratio-radius N]` (test.ratio / test.ratio_radius; off by default, N = 5) becomes the process-wide default
(oryon_amd.engine.set_default_ratio) in the same way: behind the exact scan a second one (csrc/match_second.hip) finds every anchor's
best match at least N pixels away from its nearest one, and only rows with min_dist <= R * that distance reach the solver (N = 1 is
Lowe's ratio test; with `--mutual` the mutual rows are filtered).  The summary carries `"ratio": R, "ratio_radius": N`.

    python run_pose.py --solver ransac --topk 2 --topk-radius 5 --topk-margin 0.1 --pairs 8 --batch 4

`--topk K [--topk-radius N] [--topk-margin M]` (test.topk / test.topk_radius / test.topk_margin; off by default: K = 1, N = 5, M = 0.1)
becomes the process-wide default (oryon_amd.engine.set_default_topk) in the same way: every drawn anchor hands the solver up to K rows -
its nearest query pixel and the K - 1 next best ones, each at least N pixels from all earlier ones (csrc/match_next.hip), kept while
under test.dist_th and within M (cosine distance) of the nearest.  K <= 4 and K * n_corrs <= 2048; `--mutual`, `--ratio` and K > 1 do
not combine.  The summary carries `"topk": K, "topk_radius": N, "topk_margin": M`.  N and M are design choices, not tuned on data.

    python run_pose.py --solver ransac --refine icp --verify guard --pairs 8 --batch 4

`--verify {none,score,guard} [--verify-tol M]` (test.verify / test.verify_tol; default none, M = 0.01 m) becomes the process-wide default
(oryon_amd.pipeline.set_default_verify) in the same way.  `score` rates the final pose of every solved pair against the query's depth
map (csrc/pose_verify.hip): the share of the anchor's object cloud that lands on the object within M of the measured depth - no ground
truth, no mesh.  `guard` (needs `--refine`) rates the solver's pose and the refined one and keeps the refinement only when more of the
cloud agrees with it.  The summary carries `"verify"`, `"verify_tol"`, `"verify_score_mean"` over the solved pairs and, for `guard`,
`"verify_refinements_kept"`.  M is a design choice at the scale of the refiners' gates, not tuned on data.

    python run_pose.py --solver ransac --mask-clean largest --fill-holes --pairs 8 --batch 4

`--mask-clean {none,largest,area} [--mask-clean-frac F] [--fill-holes]` (test.mask_clean / test.mask_clean_frac / test.mask_fill_holes;
default none, F = 0.25, no filling) becomes the process-wide default (oryon_amd.pipeline.set_default_mask_clean) in the same way: every
binary mask - predicted or external - is cleaned before the matcher, a refiner or the verifier uses it (csrc/mask_clean.hip): enclosed
holes filled, then the largest 8-connected component kept, or every one of at least F x the largest area.  The summary carries
`"mask_clean"`, `"mask_clean_frac"`, `"mask_fill_holes"` and the means of the clean-up's statistics over the masks it saw.  F is a
design choice, not tuned on data.

    python run_pose.py --solver ransac --subpixel --subpixel-curv-min 1e-4 --subpixel-depth-jump 0.02 --pairs 8 --batch 4

`--subpixel [--subpixel-curv-min X] [--subpixel-depth-jump M]` (test.subpixel / test.subpixel_curv_min / test.subpixel_depth_jump; off by
default, X = 1e-4, M = 0.02 m) becomes the process-wide default (oryon_amd.engine.set_default_subpixel) in the same way: every selected
correspondence gets a sub-pixel offset on the query side from a quadratic fit of the descriptor distance over the 3 x 3 pixels around the
match (csrc/match_subpix.hip), and the lift reads the depth bilinearly there where the four depths around it lie within M of each other.
Composes with every other flag.  The summary carries `"subpixel"`, the two numbers, the rows per flag (refined, border, flat, outside)
and the mean |offset| of the refined rows.  X and M are design choices, not tuned on data.

    python run_pose.py --vsd --data-root /data --dataset nocs --ckpt ... --out preds/nocs.csv

`--vsd` (real-asset mode only) also reports VSD and AR = (VSD + MSSD + MSPD) / 3, the reference's headline column
(utils/evaluator.py:281-288): once run_test.py has written its prediction CSV, compute_metrics.py scores that file over the same pairs
with `Evaluator(compute_vsd=True)` on the device (model meshes rendered by csrc/vsd.hip) and the summary printed last carries `VSD`, `AR`
and the full table row in place of run_test.py's `not_computed` note.  The split's images are decoded a second time for it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


REFINE_CHOICES = ["none", "icp", "icp_plane"]          # oryon_amd.pipeline.REFINEMENTS
VERIFY_CHOICES = ["none", "score", "guard"]            # oryon_amd.pipeline.VERIFY_MODES
MASK_CLEAN_CHOICES = ["none", "largest", "area"]       # oryon_amd.pipeline.MASK_CLEAN_MODES


def take_refine(argv=None):
    """-> (test.refine: 'none', 'icp' or 'icp_plane', argv without `--refine ...`); an unknown refinement exits like an unknown solver."""
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--refine", choices=REFINE_CHOICES, default="none")
    a, rest = ap.parse_known_args(argv)
    return a.refine, rest


def take_mask_clean(argv=None):
    """-> (the `--mask-clean` / `--mask-clean-frac` / `--fill-holes` values, argv without them).  A parser of its own that takes no
    abbreviations: run_test.py's `--mask` is a prefix of `--mask-clean` and must go through untouched."""
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    ap.add_argument("--mask-clean", choices=MASK_CLEAN_CHOICES, default="none")
    ap.add_argument("--mask-clean-frac", type=float, default=0.25)
    ap.add_argument("--fill-holes", action="store_true")
    return ap.parse_known_args(argv)


def take_topk(argv=None):
    """-> (the `--topk` / `--topk-radius` / `--topk-margin` values, argv without them); a parser of its own that takes no abbreviations."""
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    ap.add_argument("--topk", type=int, default=1)
    ap.add_argument("--topk-radius", type=int, default=5)
    ap.add_argument("--topk-margin", type=float, default=0.1)
    return ap.parse_known_args(argv)


def take_subpixel(argv=None):
    """-> (the `--subpixel` / `--subpixel-curv-min` / `--subpixel-depth-jump` values, argv without them); a parser of its own that takes
    no abbreviations."""
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    ap.add_argument("--subpixel", action="store_true")
    ap.add_argument("--subpixel-curv-min", type=float, default=1e-4)
    ap.add_argument("--subpixel-depth-jump", type=float, default=0.02)
    return ap.parse_known_args(argv)


class Parsed(tuple):
    """(solver, the arguments left for run_test.py), with `.mutual`: whether `--mutual` was given (taken out, like `--refine`),
    `.ratio` / `.ratio_radius`: what `--ratio` / `--ratio-radius` gave (0.0 / 5 when absent), and `.verify` / `.verify_tol`: what
    `--verify` / `--verify-tol` gave ('none' / 0.01 when absent), and `.mask_clean` / `.mask_clean_frac` / `.mask_fill_holes`: what
    `--mask-clean` / `--mask-clean-frac` / `--fill-holes` gave ('none' / 0.25 / False when absent), and `.topk` / `.topk_radius` /
    `.topk_margin`: what `--topk` / `--topk-radius` / `--topk-margin` gave (1 / 5 / 0.1 when absent), and `.subpixel` /
    `.subpixel_curv_min` / `.subpixel_depth_jump`: what `--subpixel` / `--subpixel-curv-min` / `--subpixel-depth-jump` gave (False / 1e-4 /
    0.02 when absent)."""
    def __new__(cls, solver, rest, mutual, ratio=0.0, ratio_radius=5, verify="none", verify_tol=0.01, mask_clean="none", mask_clean_frac=0.25,
                mask_fill_holes=False, topk=1, topk_radius=5, topk_margin=0.1, subpixel=False, subpixel_curv_min=1e-4,
                subpixel_depth_jump=0.02):
        self = super().__new__(cls, (solver, rest))
        self.mutual = mutual
        self.ratio = ratio
        self.ratio_radius = ratio_radius
        self.verify = verify
        self.verify_tol = verify_tol
        self.mask_clean = mask_clean
        self.mask_clean_frac = mask_clean_frac
        self.mask_fill_holes = mask_fill_holes
        self.topk = topk
        self.topk_radius = topk_radius
        self.topk_margin = topk_margin
        self.subpixel = subpixel
        self.subpixel_curv_min = subpixel_curv_min
        self.subpixel_depth_jump = subpixel_depth_jump
        return self


def parse(argv=None):
    """-> Parsed: (solver, the arguments left for run_test.py) + .mutual.  `--refine` is checked and taken out as well (take_refine
    returns it), and so are `--mutual` (test.mutual: keep only the mutual nearest neighbours, csrc/match_mutual.hip) and `--ratio` /
    `--ratio-radius` (test.ratio, test.ratio_radius: the ratio test with an exclusion disc, csrc/match_second.hip) and `--verify` /
    `--verify-tol` (test.verify, test.verify_tol: depth-consistency verification of the poses, csrc/pose_verify.hip) and `--mask-clean` /
    `--mask-clean-frac` / `--fill-holes` (test.mask_clean, test.mask_clean_frac, test.mask_fill_holes: connected-component clean-up of
    the masks, csrc/mask_clean.hip) and `--topk` / `--topk-radius` / `--topk-margin` (test.topk, test.topk_radius, test.topk_margin:
    up to K rows per drawn anchor, csrc/match_next.hip) and `--subpixel` / `--subpixel-curv-min` / `--subpixel-depth-jump` (test.subpixel,
    test.subpixel_curv_min, test.subpixel_depth_jump: sub-pixel refinement of the selected rows, csrc/match_subpix.hip)."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, add_help=False)
    ap.add_argument("--solver", choices=["pointdsc", "ransac", "spectral"], default="pointdsc",
                    help="test.solver: PointDSC registration, best_fit_transform_with_RANSAC, or the spectral solver (the last two need no "
                         "PointDSC weights)")
    ap.add_argument("--refine", choices=REFINE_CHOICES, default="none", help="test.refine: ICP refinement of every solved pose (see above)")
    ap.add_argument("--mutual", action="store_true", help="test.mutual: match in both directions, keep the mutual nearest neighbours")
    ap.add_argument("--ratio", type=float, default=0.0, help="test.ratio: keep a match only when min_dist <= RATIO * the best distance "
                                                             "outside the exclusion disc (0 = off)")
    ap.add_argument("--ratio-radius", type=int, default=5, help="test.ratio_radius: radius of that disc in pixels (1 = Lowe's ratio test)")
    ap.add_argument("--verify", choices=VERIFY_CHOICES, default="none", help="test.verify: score the final pose against the query's depth "
                                                                             "map, or guard a refinement with that score (see above)")
    ap.add_argument("--verify-tol", type=float, default=0.01, help="test.verify_tol: metres a moved point may lie from the measured surface")
    ap.add_argument("-h", "--help", action="store_true")
    mc, argv = take_mask_clean(argv)
    tk, argv = take_topk(argv)
    sp, argv = take_subpixel(argv)
    a, rest = ap.parse_known_args(argv)
    if a.help:
        ap.print_help()
        rest = ["--help"] + rest               # then run_test.py's own help
    return Parsed(a.solver, rest, a.mutual, a.ratio, a.ratio_radius, a.verify, a.verify_tol, mc.mask_clean, mc.mask_clean_frac, mc.fill_holes,
                  tk.topk, tk.topk_radius, tk.topk_margin, sp.subpixel, sp.subpixel_curv_min, sp.subpixel_depth_jump)


def take_vsd(argv):
    """-> (whether `--vsd` was given, argv without it)."""
    argv = list(sys.argv[1:] if argv is None else argv)
    return "--vsd" in argv, [x for x in argv if x != "--vsd"]


def add_vsd(summary: dict, rest) -> dict:
    """Score the CSV that run_test.py just wrote with VSD and AR and fold the result into its summary."""
    import compute_metrics
    ap = argparse.ArgumentParser(add_help=False)
    for name, default in (("--data-root", None), ("--dataset", "nocs"), ("--dataset-name", None), ("--split", "cross_scene_test"),
                          ("--obj", "all"), ("--mask", "predicted")):
        ap.add_argument(name, default=default)
    a, _ = ap.parse_known_args(rest)
    m = compute_metrics.main([summary["csv"], "--data-root", a.data_root, "--dataset", a.dataset, "--split", a.split, "--obj", a.obj,
                              "--mask", a.mask, "--pairs", str(summary["pairs"])] +
                             (["--dataset-name", a.dataset_name] if a.dataset_name else []))
    out = {k: v for k, v in summary.items() if k != "not_computed"}
    out.update({"VSD": m["VSD"], "AR": m["AR"], "latex_row": m["latex_row"], "metrics_json": m["metrics_json"]})
    print(json.dumps(out))
    return out


def main(argv=None):
    vsd, argv = take_vsd(argv)
    refine, _ = take_refine(argv)
    parsed = parse(argv)
    solver, rest = parsed
    if vsd and "--data-root" not in rest and not any(r.startswith("--data-root=") for r in rest):
        raise SystemExit("run_pose.py --vsd needs real-asset mode (--data-root ...): the synthetic pairs have no object mesh")
    if parsed.verify == "guard" and refine == "none":
        raise SystemExit("run_pose.py --verify guard needs --refine icp or --refine icp_plane: nothing to choose from")
    if not parsed.verify_tol >= 0.0:
        raise SystemExit("run_pose.py --verify-tol is a distance in metres, >= 0")
    if not 0.0 <= parsed.mask_clean_frac <= 1.0:
        raise SystemExit("run_pose.py --mask-clean-frac is a share of the largest component's area, in [0, 1]")
    if parsed.topk > 1 and (parsed.mutual or parsed.ratio > 0):
        raise SystemExit("run_pose.py --topk K > 1 does not combine with --mutual (no reverse ranks) or --ratio (it deletes what --topk keeps)")
    from oryon_amd.engine import set_default_topk
    try:
        set_default_topk(parsed.topk, parsed.topk_radius, parsed.topk_margin)
    except ValueError as e:
        raise SystemExit(f"run_pose.py: {e}")
    from oryon_amd.engine import set_default_subpixel
    try:
        set_default_subpixel(parsed.subpixel, parsed.subpixel_curv_min, parsed.subpixel_depth_jump)
    except ValueError as e:
        raise SystemExit(f"run_pose.py: {e}")
    from oryon_amd.engine import set_default_solver
    set_default_solver(solver)
    from oryon_amd.pipeline import set_default_refine
    set_default_refine(refine)
    from oryon_amd.engine import set_default_mutual
    set_default_mutual(parsed.mutual)
    from oryon_amd.engine import set_default_ratio
    set_default_ratio(parsed.ratio, parsed.ratio_radius)
    from oryon_amd.pipeline import set_default_verify
    set_default_verify(parsed.verify, parsed.verify_tol)
    from oryon_amd.pipeline import set_default_mask_clean
    set_default_mask_clean(parsed.mask_clean, parsed.mask_clean_frac, parsed.mask_fill_holes)
    import run_test
    summary = run_test.main(rest)
    verified = parsed.verify != "none"
    cleaned = parsed.mask_clean != "none" or parsed.mask_fill_holes
    if parsed.mutual or parsed.ratio > 0 or verified or cleaned or parsed.topk > 1 or parsed.subpixel:
        if parsed.mutual:
            summary = dict(summary, mutual=True)
        if parsed.ratio > 0:
            summary = dict(summary, ratio=parsed.ratio, ratio_radius=parsed.ratio_radius)
        if parsed.topk > 1:
            summary = dict(summary, topk=parsed.topk, topk_radius=parsed.topk_radius, topk_margin=parsed.topk_margin)
        if parsed.subpixel:
            from oryon_amd.pipeline import subpixel_summary       # what the pipelines run_test.py built have refined
            summary = {**summary, "subpixel": True, "subpixel_curv_min": parsed.subpixel_curv_min,
                       "subpixel_depth_jump": parsed.subpixel_depth_jump, **subpixel_summary()}
        if verified:
            from oryon_amd.pipeline import verify_summary         # what the pipelines run_test.py built have rated
            summary = {**summary, "verify": parsed.verify, "verify_tol": parsed.verify_tol, **verify_summary()}
        if cleaned:
            from oryon_amd.pipeline import mask_clean_summary     # what the pipelines run_test.py built have cleaned
            summary = {**summary, "mask_clean": parsed.mask_clean, "mask_clean_frac": parsed.mask_clean_frac,
                       "mask_fill_holes": parsed.mask_fill_holes, **mask_clean_summary()}
        if not (vsd and summary.get("pairs")):
            print(json.dumps(summary))               # run_test.py's line again, with the flag recorded
    return add_vsd(summary, rest) if vsd and summary.get("pairs") else summary


if __name__ == "__main__":
    main()
