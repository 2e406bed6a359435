"""Clustering a gallery, and a reference vector chosen by clustering -- the reference's `get_cluster_features`
(code/search_image.py:185-232: KMeans on the encoded samples, the majority cluster, the `shots` rows nearest its centre,
their mean) at both of its scales.

Planted clusters: each gallery row is a noisy copy of one of C unit centres.  `kmeans` groups the whole gallery (every
assignment exact, no [N, K] score matrix); for one class, `reference_vector_by_clustering` turns a handful of sample
rows -- some of them outliers from another class -- into a reference vector, and `GalleryIndex.search` retrieves with it.

    python examples/cluster_gallery_synthetic.py [--rows 200000] [--classes 16] [--dim 512]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd as clip  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--shots", type=int, default=10)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    C, N, E = args.classes, args.rows, args.dim

    gen = torch.Generator().manual_seed(3)
    truth = torch.randint(0, C, (N,), generator=gen)
    centres = clip.synth.synth_unit_rows(C, E, seed=30)
    feats = centres[truth] + 0.5 * clip.synth.synth_unit_rows(N, E, seed=31)
    feats = (feats / feats.norm(dim=-1, keepdim=True)).to(torch.float16).to(dev)
    truth = truth.to(dev)

    # 1. group the gallery: spherical k-means from C sampled rows
    res = clip.kmeans(feats, C, init="sample", metric="cosine", generator=torch.Generator().manual_seed(4), max_iter=30)
    # purity: the share of rows whose cluster's majority class is their own
    table = torch.zeros(C, C, dtype=torch.int64, device=dev)
    table.index_put_((res.labels.long(), truth), torch.ones(N, dtype=torch.int64, device=dev), accumulate=True)
    purity = float(table.max(1).values.sum()) / N
    print(f"kmeans: {N} rows, K={C}, {res.n_iter} assignments, converged={res.converged}, inertia {res.inertia:.2f}, "
          f"purity {purity:.4f}, sizes {res.sizes.tolist()}")

    # 2. a reference vector for class 0 from samples polluted by another class
    own = torch.nonzero(truth == 0).reshape(-1)[:args.samples * 3 // 4]
    other = torch.nonzero(truth == 1).reshape(-1)[:args.samples - own.numel()]
    samples = feats[torch.cat([own, other])]
    vec, chosen = clip.reference_vector_by_clustering(samples, args.shots, generator=torch.Generator().manual_seed(8),
                                                      return_indices=True)
    clean = int((chosen < own.numel()).sum())
    print(f"reference vector: {clean} of the {chosen.numel()} chosen shots come from the class itself")

    # 3. retrieve with it
    index = clip.GalleryIndex(feats)
    _, idx = index.search(vec.to(dev), 50)
    hits = int((truth[idx.reshape(-1)] == 0).sum())
    print(f"search: {hits} of the top 50 rows belong to class 0")
    return {"purity": purity, "n_iter": res.n_iter, "sizes": res.sizes.cpu().numpy(), "clean_shots": clean,
            "shots": int(chosen.numel()), "hits": hits}


if __name__ == "__main__":
    main()
