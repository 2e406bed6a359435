"""The reference's few-shot retrieval protocol (code/search_image.py:340-390) as ONE call: every class builds its query
from its own sample images ("shots"), `construct_dataset` takes exactly those images out of the gallery it is then
scored against, and `find_thresholds` sweeps a threshold grid for the best F1 -- for reference_nums = [1, 5, 10, 20] x
classes, i.e. 24 queries over 24 different galleries.  A class's shots stay in the other classes' galleries as negatives.

With one mask per call that is 24 threshold sweeps, each streaming the whole gallery; ``row_masks=`` gives every query
its own mask and streams it once.  The script runs both and checks that they agree exactly.  Synthetic features: each
class is a unit centre, each gallery row a noisy copy of its class centre, a query the normalised mean of its shots.

    python examples/few_shot_sweep_synthetic.py [--rows 200000] [--dim 512]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd as clip  # noqa: E402

CLASSES, SHOTS = 6, (1, 5, 10, 20)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--points", type=int, default=200)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")

    centres = clip.synth.synth_unit_rows(CLASSES, args.dim, seed=1).to(dev)
    labels = torch.randint(0, CLASSES, (args.rows,), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(dev)
    feats = 0.12 * centres[labels.long()] + clip.synth.synth_unit_rows(args.rows, args.dim, seed=3).to(dev)
    feats = (feats / feats.norm(dim=-1, keepdim=True)).bfloat16()
    index = clip.GalleryIndex(feats)

    # query (n shots, class c): the mean of n sample images of class c; those images leave ITS gallery only
    rng = np.random.default_rng(4)
    lab = labels.cpu().numpy()
    queries, targets, qids, rows = [], [], [], []
    for n in SHOTS:
        for c in range(CLASSES):
            shots = rng.choice(np.flatnonzero(lab == c), n, replace=False)
            v = feats[torch.from_numpy(shots).to(dev)].float().mean(0)
            queries.append(v / v.norm())
            targets.append(c)
            qids += [len(queries) - 1] * n
            rows += shots.tolist()
    queries = torch.stack(queries).bfloat16()
    targets = torch.tensor(targets, dtype=torch.int32, device=dev)
    Q = queries.shape[0]
    masks = clip.leave_out_masks(Q, args.rows, qids, rows, dev)

    lo, hi = index.score_extent(queries)
    grid = np.linspace(float(lo.min()), float(hi.max()), args.points)
    sweep = index.threshold_sweep(queries, labels, targets, grid, row_masks=masks)           # one pass, 24 galleries
    best = sweep.best()

    # the same through the single-mask call: one gallery pass per query
    for i in range(Q):
        one = index.threshold_sweep(queries[i:i + 1], labels, targets[i:i + 1], grid, row_mask=masks.row_mask(i))
        assert torch.equal(one.tp[0], sweep.tp[i]) and torch.equal(one.fp[0], sweep.fp[i]), i
        assert int(one.pos[0]) == int(sweep.pos[i]) and int(one.neg[0]) == int(sweep.neg[i]), i
    print(f"gallery: {args.rows} x {args.dim} bf16; {Q} queries ({len(SHOTS)} shot counts x {CLASSES} classes), each without its own "
          f"shots; one call equals the loop of {Q} single-mask calls exactly")
    report = []
    for i in range(Q):
        n, c = SHOTS[i // CLASSES], i % CLASSES
        report.append((n, c, float(best["threshold"][i]), float(best["f1"][i])))
        print(f"shots {n:2d} class {c}: best threshold {report[-1][2]:7.4f}  F1 {report[-1][3]:.4f}  "
              f"({int(sweep.pos[i])} positives left in its gallery)")
    return report


if __name__ == "__main__":
    main()
