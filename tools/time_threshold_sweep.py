"""Labelled threshold sweep timings on device events: three routes alternated inside one process; a table and one JSON line.

    python tools/time_threshold_sweep.py [--quick] [--out profiles/threshold_sweep_timings.txt]

Workload: N = 1M x 512 bf16 unit rows with class structure (7 centres, g = normalize(0.12 * centre[label] + unit noise)),
Q in {10, 64} class-like queries, T in {200, 1001} (the reference's linspace(min, max, 200) and step-1e-3 grids).
  (a) floor     GalleryIndex.search(q, k=10): one gallery stream plus the finalize chain
  (b) parent    similarity(gallery, q) (the [N,Q] fp32 matrix) then torch.bucketize + bincount per (query, class) on the
                device: what the code offered for the same answer before threshold_sweep (fp32 scores, so not exact)
  (c) sweep     GalleryIndex.threshold_sweep, cand_cap taken from a first call so the timed calls do not retry
10 warm-ups per route, then 5 repeats of 20 calls; each repeat runs the routes in turn.  Reported: the minimum over the
repeats (ms per call) and the spread (max - min) of each route, counts[1] / (Q*N), the gallery passes, and the memory each
route needs beyond the gallery.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd  # noqa: E402,F401
from mmr_amd import _lib, search, synth  # noqa: E402

NCLASS = 7


def labelled_gallery(n, e, dev):
    gen = torch.Generator(device=dev).manual_seed(5)
    centres = synth.synth_unit_rows(NCLASS, e, seed=5).to(dev)
    labels = torch.randint(0, NCLASS, (n,), generator=gen, device=dev, dtype=torch.int32)
    g = torch.empty(n, e, dtype=torch.bfloat16, device=dev)
    for s in range(0, n, 1 << 17):
        x = torch.randn(min(1 << 17, n - s), e, generator=gen, device=dev)
        x = 0.12 * centres[labels[s:s + x.shape[0]].long()] + x / x.norm(dim=-1, keepdim=True)
        g[s:s + x.shape[0]] = (x / x.norm(dim=-1, keepdim=True)).bfloat16()
    return g, labels, centres


def per_call_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def torch_route(g, q, labels, targets, thr32):
    """The parent's route: materialise the scores, then histogram them per (query, class) in torch."""
    T = thr32.shape[0]
    s = search.similarity(g, q, 1.0)                                    # [N,Q] fp32
    b = torch.bucketize(s.t().contiguous(), thr32, right=True)          # [Q,N] bins = thresholds <= score
    cls = (labels.unsqueeze(0) == targets.unsqueeze(1)).long()
    key = (torch.arange(q.shape[0], device=g.device).unsqueeze(1) * 2 + cls) * (T + 1) + b
    hist = torch.bincount(key.flatten(), minlength=q.shape[0] * 2 * (T + 1)).view(q.shape[0], 2, T + 1)
    return torch.flip(torch.cumsum(torch.flip(hist, [-1]), -1), [-1])[..., 1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="100k rows, 2 repeats of 3 calls (a smoke run of the tool itself)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, E = (100_000 if args.quick else 1_000_000), 512
    warm, reps, calls = (2, 2, 3) if args.quick else (10, 5, 20)
    g, labels, centres = labelled_gallery(N, E, dev)
    index = search.GalleryIndex(g)
    L = _lib.lib()
    rows, cells = [], {}
    for Q in (10, 64):
        q = torch.cat([centres, synth.synth_unit_rows(Q - NCLASS, E, seed=6).to(dev)]).bfloat16()
        targets = (torch.arange(Q, dtype=torch.int32) % NCLASS).to(dev)
        lo, hi = index.score_extent(q)
        for T, thr in ((200, np.linspace(float(lo.min()), float(hi.max()), 200)), (1001, np.arange(0, 1.001, 0.001))):
            first = index.threshold_sweep(q, labels, targets, thr)
            cands = first.counts[1]
            cap = cands + cands // 8 + 1024
            thr32 = torch.from_numpy(thr).float().to(dev)
            fns = {"a_topk10": lambda: index.search(q, 10),
                   "b_similarity_bincount": lambda: torch_route(g, q, labels, targets, thr32),
                   "c_threshold_sweep": lambda: index.threshold_sweep(q, labels, targets, thr, cand_cap=cap)}
            # the two answers agree except where an fp32 score and the fp64 dot fall on different sides of a grid point
            ge_b = fns["b_similarity_bincount"]()
            differ = int((ge_b[:, 1] != first.tp).sum() + (ge_b[:, 0] != first.fp).sum())
            for _ in range(warm):
                for f in fns.values():
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k in fns}
            for _ in range(reps):
                for k, f in fns.items():
                    times[k].append(per_call_ms(f, calls))
            per_pass = max(1, min(256, (160 * 1024 - 3 * 32 * E * 2 - 8192 - (2 * (T + 2) * 4 + 15) // 16 * 16) // (4 * (T + 1))))
            cell = {"Q": Q, "T": T, "candidate_share": cands / (Q * N), "gallery_passes": -(-Q // per_pass),
                    "grid_points_where_b_differs": differ,
                    "sweep_workspace_bytes": L.mmr_sweep_workspace_bytes(N, E, Q, T, cap, _lib.MMR_BF16, 0),
                    "b_extra_bytes": Q * N * 4 + Q * N * 8 * 2,
                    **{k + "_ms": [round(x, 4) for x in v] for k, v in times.items()}}
            mn = {k: min(v) for k, v in times.items()}
            sp = {k: max(v) - min(v) for k, v in times.items()}
            cell["c_faster_than_b_beyond_spread"] = bool(mn["b_similarity_bincount"] - mn["c_threshold_sweep"] >
                                                         max(sp["b_similarity_bincount"], sp["c_threshold_sweep"]))
            cells[f"Q{Q}_T{T}"] = cell
            rows.append(f"{Q:3d} {T:5d} | {mn['a_topk10']:8.3f} {sp['a_topk10']:6.3f} | {mn['b_similarity_bincount']:9.3f} "
                        f"{sp['b_similarity_bincount']:6.3f} | {mn['c_threshold_sweep']:8.3f} {sp['c_threshold_sweep']:6.3f} | "
                        f"{mn['b_similarity_bincount'] / mn['c_threshold_sweep']:5.2f}x | {cell['candidate_share']:6.4f} "
                        f"{cell['gallery_passes']:2d} | {cell['b_extra_bytes'] / 2 ** 20:8.1f} {cell['sweep_workspace_bytes'] / 2 ** 20:7.1f}")
    head = [f"threshold sweep, N = {N} x {E} bf16, {warm} warm-ups, min (and max - min) over {reps} repeats of {calls} calls, ms per call",
            "  Q     T | (a) top-k 10 spread | (b) similarity+bincount spread | (c) sweep spread | b / c | cand/(Q*N) passes | "
            "extra MiB (b)  (c)"]
    table = "\n".join(head + rows)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")
    print(json.dumps({"gallery": [N, E], "warm": warm, "reps": reps, "calls": calls, "cells": cells}))


if __name__ == "__main__":
    main()
