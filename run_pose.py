#!/usr/bin/env python3
"""The test driver with the pose solver on the command line (test.solver of the reference's configs/config.yaml:57).

    python run_pose.py --solver ransac [every argument of run_test.py]
    python run_pose.py --solver ransac --pairs 8 --batch 4
    python run_pose.py --solver ransac --data-root /data --dataset nocs --ckpt ... --bpe ...       # no --pointdsc snapshot needed

`--solver {pointdsc,ransac}` (default pointdsc) becomes the process-wide default solver (oryon_amd.engine.set_default_solver): every
`default_args()` and `MatchPoseConfig()` that run_test.py builds - the per-sample loop, the batched engine, its --half-descriptors
engine - then selects it.  Everything else goes to run_test.py unchanged.  With `ransac` (best_fit_transform_with_RANSAC,
utils/geo6d.py:75-120, max_iter=10000, fix_percent=0.9999, match_err=0.001 as pipeline.py:463) no PointDSC weights take part in a pose."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse(argv=None):
    """-> (solver, the arguments left for run_test.py)."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, add_help=False)
    ap.add_argument("--solver", choices=["pointdsc", "ransac"], default="pointdsc",
                    help="test.solver: PointDSC registration, or best_fit_transform_with_RANSAC (needs no PointDSC weights)")
    ap.add_argument("-h", "--help", action="store_true")
    a, rest = ap.parse_known_args(argv)
    if a.help:
        ap.print_help()
        rest = ["--help"] + rest               # then run_test.py's own help
    return a.solver, rest


def main(argv=None):
    solver, rest = parse(argv)
    from oryon_amd.engine import set_default_solver
    set_default_solver(solver)
    import run_test
    return run_test.main(rest)


if __name__ == "__main__":
    main()
