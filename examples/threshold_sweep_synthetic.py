"""Per-class decision thresholds over a labelled gallery -- the tail of the reference's retrieval drivers
(code/search_image.py `find_thresholds`: score every gallery image against a class vector, split the scores by label,
sweep 200 thresholds between the smallest and the largest score, keep the one with the best F1), in one pass over the
gallery per batch of class vectors and without the [classes, N] score matrix.  Synthetic features: each class is a unit
centre, each gallery row a noisy copy of its class centre.

    python examples/threshold_sweep_synthetic.py [--rows 200000] [--classes 7] [--dim 512]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd as clip  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--points", type=int, default=200)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")

    centres = clip.synth.synth_unit_rows(args.classes, args.dim, seed=1).to(dev)             # the class vectors
    labels = torch.randint(0, args.classes, (args.rows,), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(dev)
    feats = 0.12 * centres[labels.long()] + clip.synth.synth_unit_rows(args.rows, args.dim, seed=3).to(dev)
    feats = (feats / feats.norm(dim=-1, keepdim=True)).bfloat16()                            # the gallery's image features
    index = clip.GalleryIndex(feats)
    queries = centres.bfloat16()
    targets = torch.arange(args.classes, dtype=torch.int32, device=dev)

    lo, hi = index.score_extent(queries)                                                     # min_val / max_val, exact
    grid = np.linspace(float(lo.min()), float(hi.max()), args.points)
    sweep = index.threshold_sweep(queries, labels, targets, grid)                            # TP / FP at every grid point
    best = sweep.best()
    print(f"gallery: {args.rows} x {args.dim} bf16, {args.classes} classes, {args.points}-point grid over "
          f"[{grid[0]:.4f}, {grid[-1]:.4f}]; {sweep.counts[1]} of {args.classes * args.rows} pairs needed the fp64 recheck")
    report = []
    for c in range(args.classes):
        report.append((c, float(best["threshold"][c]), float(best["f1"][c]), float(best["precision"][c]), float(best["recall"][c])))
        print(f"class {c}: best threshold {report[-1][1]:7.4f}  F1 {report[-1][2]:.4f}  precision {report[-1][3]:.4f}  "
              f"recall {report[-1][4]:.4f}  ({int(sweep.pos[c])} positives)")
    return report


if __name__ == "__main__":
    main()
