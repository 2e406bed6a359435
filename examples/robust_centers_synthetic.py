"""Outlier-trimmed class centres of a labelled gallery -- the reference's `outlier_filter` (code/search_image.py:295-318),
the rule its live main() loop builds every class's query vector with -- for all classes of a gallery in one pass on the GPU.

Each class is a cloud of unit rows around a prototype; a few rows per class are PLANTED: they carry the class's label but
come from another class's prototype (a mislabelled image).  `trimmed_centers` takes every row's exact distance to its
class mean, drops the rows beyond the class's 95th percentile and averages the rest.  Three products:

  * the trimmed centre of every class, nearer the prototype than the plain mean;
  * the per-class outlier list -- the rows a class should not contain: a data-governance product in its own right;
  * retrieval with the trimmed centre as the query (`cosine_topk`).

    python examples/robust_centers_synthetic.py [--classes 10] [--per-class 2000] [--planted 40] [--dim 512]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd as clip  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--per-class", type=int, default=2000)
    ap.add_argument("--planted", type=int, default=40, help="off-class rows per class; keep it below 5 %% of --per-class")
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--percentile", type=float, default=95.0)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    C, P, E = args.classes, args.per_class, args.dim
    N = C * P

    protos = clip.synth.synth_unit_rows(C, E, seed=50)
    labels = torch.arange(N) // P
    source = labels.clone()
    gen = torch.Generator().manual_seed(51)
    planted = {}
    for c in range(C):
        rows = c * P + torch.randperm(P, generator=gen)[:args.planted]
        source[rows] = (c + 1 + torch.randint(0, C - 1, (args.planted,), generator=gen)) % C      # any class but c
        planted[c] = sorted(rows.tolist())
    feats = protos[source] + 0.6 * clip.synth.synth_unit_rows(N, E, seed=52)
    feats = (feats / feats.norm(dim=-1, keepdim=True)).to(torch.float16).to(dev)
    labels = labels.to(dev)

    res = clip.trimmed_centers(feats, labels, C, percentile=args.percentile)
    plain_sums, sizes = clip.cluster_sums(feats, labels, C)
    plain = plain_sums / sizes.to(torch.float64)[:, None]
    outlier = ~res.keep & (labels >= 0)
    protos64 = protos.to(dev, torch.float64)

    def cos(a, b):
        return float((a * b).sum() / (a.norm() * b.norm()))

    # retrieval: the trimmed centres as queries, the class's own clean rows as what should come back
    k = 64
    queries = torch.nn.functional.normalize(res.centers.to(torch.float32), dim=-1).to(feats.dtype)
    _, idx = clip.cosine_topk(queries, feats, k)
    clean = (source.to(dev) == labels)

    report = []
    for c in range(C):
        flagged = torch.nonzero(outlier & (labels == c)).reshape(-1).tolist()
        hits = int((clean[idx[c].long()] & (labels[idx[c].long()] == c)).sum())
        entry = {"class": c, "size": int(res.sizes[c]), "kept": int(res.kept[c]), "threshold": float(res.thresholds[c]),
                 "planted": planted[c], "outliers": flagged, "plain_cos": cos(plain[c], protos64[c]),
                 "trimmed_cos": cos(res.centers[c], protos64[c]), "hits": hits}
        report.append(entry)
        found = len(set(flagged) & set(planted[c]))
        print(f"class {c}: {entry['size']} rows, kept {entry['kept']} (1 - x.c <= {entry['threshold']:.4f}); flagged {len(flagged)}, "
              f"{found} of the {len(planted[c])} planted among them; cos(centre, prototype) plain {entry['plain_cos']:.5f} -> trimmed "
              f"{entry['trimmed_cos']:.5f}; top-{k} of the trimmed centre: {hits} clean rows of the class")
    return report


if __name__ == "__main__":
    main()
