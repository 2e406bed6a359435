"""Per-class decisions of two backends and their union -- the flow of the reference's code/merge_dataset.py `__main__`
and CLIP/union_dataset.py: an English and a Chinese CLIP each score every image against every class vector, each class
has a threshold of its own per backend (found by a sweep on labelled data), an image is predicted for a class when
EITHER backend clears its threshold, and the union's TP / FP / FN are counted per class.

Here each backend's decision is one pass over its gallery that leaves one packed row mask per class
(`GalleryIndex.decide`), the union is a word-wise OR (`en | cn`), the confusion counts come from the masks
(`.confusion`), and a mask row restricts a later search (`row_mask=`).  No [classes, N] score matrix is written.
Synthetic features: each class is a unit centre per backend, each gallery row a noisy copy of its class centre.

    python examples/union_predict_synthetic.py [--rows 200000] [--classes 7]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd as clip  # noqa: E402


def _backend(rows, labels, classes, dim, dtype, seed, dev):
    """(index over the backend's image features, its class vectors)"""
    centres = clip.synth.synth_unit_rows(classes, dim, seed=seed).to(dev)
    feats = 0.12 * centres[labels.long()] + clip.synth.synth_unit_rows(rows, dim, seed=seed + 1).to(dev)
    feats = (feats / feats.norm(dim=-1, keepdim=True)).to(dtype)
    return clip.GalleryIndex(feats), centres.to(dtype)


def _best_thresholds(index, queries, labels, targets, points):
    """find_thresholds per class: the first grid point with the largest F1"""
    lo, hi = index.score_extent(queries)
    grid = np.linspace(float(lo.min()), float(hi.max()), points)
    return index.threshold_sweep(queries, labels, targets, grid).best()["threshold"]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--points", type=int, default=200)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    C, N = args.classes, args.rows

    labels = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(dev)
    targets = torch.arange(C, dtype=torch.int32, device=dev)
    en_index, en_q = _backend(N, labels, C, 512, torch.bfloat16, 10, dev)        # the "EN" backend: 512-d bf16
    cn_index, cn_q = _backend(N, labels, C, 768, torch.float16, 20, dev)         # the "CN" backend: 768-d fp16

    en_thr = _best_thresholds(en_index, en_q, labels, targets, args.points)      # one threshold per class and backend
    cn_thr = _best_thresholds(cn_index, cn_q, labels, targets, args.points)
    en = en_index.decide(en_q, en_thr)                                           # C row masks each, one gallery pass each
    cn = cn_index.decide(cn_q, cn_thr)
    union = en | cn                                                              # predicted if either backend says so
    conf = union.confusion(labels, targets)
    _, _, f1 = conf.metrics()
    _, _, f1_en = en.confusion(labels, targets).metrics()
    _, _, f1_cn = cn.confusion(labels, targets).metrics()
    print(f"gallery: {N} rows, {C} classes; EN 512-d bf16 ({en.counts[0]} pairs rechecked in fp64), CN 768-d fp16 "
          f"({cn.counts[0]}); masks: {union.words.numel() * 4} bytes")
    tp, fp, fn, tn = (x.cpu().tolist() for x in (conf.tp, conf.fp, conf.fn, conf.tn))
    report, top5 = [], []
    for c in range(C):
        report.append((c, tp[c], fp[c], fn[c], tn[c], float(f1[c])))
        print(f"class {c}: union TP {tp[c]} FP {fp[c]} FN {fn[c]} TN {tn[c]}  F1 {f1[c]:.4f}  (EN alone {f1_en[c]:.4f} at "
              f"{en_thr[c]:.4f}, CN alone {f1_cn[c]:.4f} at {cn_thr[c]:.4f})")
        # the five best EN matches among the images the union predicts for this class
        _, idx = en_index.search(en_q[c], 5, row_mask=union.row_mask(c))
        top5.append(idx.cpu().numpy())
    return {"report": report, "top5": top5, "labels": labels.cpu().numpy(), "en_bits": en.to_bool().cpu().numpy(),
            "cn_bits": cn.to_bool().cpu().numpy(), "en": (en_q, en_index.gallery, en_thr), "cn": (cn_q, cn_index.gallery, cn_thr)}


if __name__ == "__main__":
    main()
