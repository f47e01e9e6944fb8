#!/usr/bin/env python3
"""Fixed-split builder: the counterpart of the reference's scripts/data/make_toyl_test.py and make_nocs_test.py.  Draws view pairs of one
object in one scene from a source split, computes each pair's ground-truth pixel correspondences on the device (lift both masks, move
the anchor cloud by pose_q @ inv(pose_a), all-pairs nearest neighbour in float64, keep rows within the threshold: csrc/gt_corrs.hip)
and writes what datasets.FixedSplit reads:

    <data-root>/fixed_split/<dest-split>/instance_list.txt
    <data-root>/fixed_split/<dest-split>/annots.pkl        {"<sa>_<ia>_<sq>_<iq>_<cat>[_<obj_name>]": {"gt": 4x4 (translation mm), "corrs": [n,4] float64}}

    python make_split.py --kind toyl --data-root data/toyl --src-split test --dest-split my_pairs --pairs 2000 --seed 1

`--data-root` is the dataset's own directory (the `<dataset.root>/<name>` of run_test.py / run_valid.py), laid out as the header of
oryon_amd/datasets.py documents.  One seed writes the same split every time; the pair draws are this driver's own (a seeded numpy
generator), so a split is not row-for-row the one the reference's unseeded script would draw - see oryon_amd/pairs.py.  Prints one JSON
line last.

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
    ap.add_argument("--kind", choices=["nocs", "toyl"], default="toyl")
    ap.add_argument("--data-root", default=None, help="the dataset's directory (holds split/ and fixed_split/)")
    ap.add_argument("--src-split", default=None, help="split the images come from (default: real_test for nocs, test for toyl)")
    ap.add_argument("--dest-split", default="overfit_self", help="name of the fixed split to write")
    ap.add_argument("--pairs", type=int, default=5, help="number of pairs to draw")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=0.002, help="largest distance of a correspondence, metres")
    ap.add_argument("--max-corrs", type=int, default=10000, help="correspondences kept per pair at most")
    ap.add_argument("--min-corrs", type=int, default=100, help="pairs with fewer correspondences are drawn again")
    a = ap.parse_args(argv)
    if a.src_split is None:
        a.src_split = "real_test" if a.kind == "nocs" else "test"
    return a


def main(argv=None):
    a = parse(argv)
    if not a.data_root:
        raise SystemExit("make_split.py: --data-root is required")
    import oryon_amd
    oryon_amd.configure()
    from oryon_amd.pairs import make_fixed_split
    n = make_fixed_split(a.kind, a.data_root, a.src_split, a.dest_split, a.pairs, a.seed, threshold=a.threshold, max_corrs=a.max_corrs,
                         min_corrs=a.min_corrs, log=lambda *m: print(*m, file=sys.stderr))
    summary = {"kind": a.kind, "dest": os.path.join(a.data_root, "fixed_split", a.dest_split), "pairs_requested": a.pairs, "pairs_written": n,
               "seed": a.seed, "threshold": a.threshold, "max_corrs": a.max_corrs, "min_corrs": a.min_corrs}
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
