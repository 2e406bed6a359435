"""Picking K for a gallery -- the reference's loop over `n_clusters in [2, 3, 4]` with `silhouette_score(image_features,
kmeans.labels_)` (code/search_image.py:256-259), for N rows on the GPU instead of a handful of shots on the CPU.

Planted clusters: each gallery row is a noisy copy of one of C unit centres.  `select_k` runs `kmeans` for every K of a
list and scores each labelling with the silhouette: one N x N pairwise scan on the matrix cores per K, nothing of size
N x N stored.  `silhouette_samples` then shows the rows that sit worst in the chosen clustering.

    python examples/select_k_synthetic.py [--rows 50000] [--clusters 3] [--dim 512]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd as clip  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--clusters", type=int, default=3)
    ap.add_argument("--dim", type=int, default=512)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    C, N, E = args.clusters, args.rows, args.dim

    truth = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(3))
    centres = clip.synth.synth_unit_rows(C, E, seed=30)
    feats = centres[truth] + 0.5 * clip.synth.synth_unit_rows(N, E, seed=31)
    feats = (feats / feats.norm(dim=-1, keepdim=True)).to(torch.float16).to(dev)

    ks = tuple(range(2, C + 3))
    res = clip.select_k(feats, ks, generator=torch.Generator().manual_seed(4), max_iter=30)
    for k in ks:
        r = res.results[k]
        print(f"K={k}: silhouette {res.scores[k]:+.4f}, {r.n_iter} assignments, converged={r.converged}, sizes {r.sizes.tolist()}")
    print(f"chosen K = {res.best_k}")

    best = res.results[res.best_k]
    samples = clip.silhouette_samples(feats, best.labels, res.best_k)
    worst = torch.argsort(samples)[:5]
    print("rows that fit their cluster worst: " + ", ".join(f"{int(i)} ({float(samples[i]):+.3f})" for i in worst))
    return {"best_k": res.best_k, "scores": res.scores, "sizes": best.sizes.cpu().numpy()}


if __name__ == "__main__":
    main()
