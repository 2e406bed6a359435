"""Deep top-k timings on device events: three routes alternated inside one process; a table and one JSON line.

    python tools/time_deep_topk.py [--quick] [--trace] [--out profiles/deep_topk_timings.txt]

Workload: N = 1M x 512 bf16 unit rows (synth.synth_unit_rows), cells (Q, k) = (1, 100), (16, 100), (16, 1000), (256, 100),
(256, 1000), (16, 4096), plus (16, 1000) over an fp32 gallery through a pre-split GalleryIndex.
  (a) floor   GalleryIndex.search(q, k=10): one gallery stream plus the finalize chain
  (b) before  similarity(gallery, q) (the [N,Q] fp32 matrix, fp64 dots) then torch.topk: the only route above k = 64 before
              search_deep (its tie order is torch's, so it is not the same answer where dots tie)
  (c) deep    GalleryIndex.search_deep(q, k), first capacities left at their defaults
10 warm-ups per route, then 5 repeats of 20 calls; each repeat runs the routes in turn.  Reported: the minimum over the
repeats (ms per call) and the spread (max - min) of each route, c / a, b / c, counts / (Q*k) and (b)'s score matrix in MiB.
--trace: a few calls of route (c) per cell and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd  # noqa: E402,F401
from mmr_amd import search, synth  # noqa: E402

CELLS = ((1, 100), (16, 100), (16, 1000), (256, 100), (256, 1000), (16, 4096))


def per_call_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="100k rows, 2 repeats of 3 calls (a smoke run of the tool itself)")
    ap.add_argument("--trace", action="store_true", help="route (c) alone, 3 calls per cell (run under the profiler)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, E = (100_000 if args.quick else 1_000_000), 512
    warm, reps, calls = (2, 2, 3) if args.quick else (10, 5, 20)
    g32 = synth.synth_unit_rows(N, E, seed=3)
    galleries = {"bf16": search.GalleryIndex(g32.bfloat16().to(dev)), "fp32 pre-split": search.GalleryIndex(g32.to(dev), presplit=True)}
    del g32
    rows, cells = [], {}
    for form, index, todo in (("bf16", galleries["bf16"], CELLS), ("fp32 pre-split", galleries["fp32 pre-split"], ((16, 1000),))):
        g = index.gallery
        for Q, k in todo:
            q = synth.synth_unit_rows(Q, E, seed=4).to(device=dev, dtype=g.dtype)
            if args.trace:
                for _ in range(3):
                    index.search_deep(q, k)
                torch.cuda.synchronize()
                print(f"traced {form} Q={Q} k={k}: counts {index.deep_counts}")
                continue
            fns = {"a_topk10": lambda: index.search(q, 10),
                   "b_similarity_topk": lambda: torch.topk(search.similarity(g, q, 1.0).t(), k, dim=1),
                   "c_search_deep": lambda: index.search_deep(q, k)}
            # (b) agrees with (c) wherever the k-th fp32 score is not tied
            bv, bi = fns["b_similarity_topk"]()
            cv, ci = fns["c_search_deep"]()
            listed, surv = index.deep_counts
            differ = int((bi != ci).sum())
            del bv, bi, cv, ci
            for _ in range(warm):
                for f in fns.values():
                    f()
            torch.cuda.synchronize()
            times = {n: [] for n in fns}
            for _ in range(reps):
                for n, f in fns.items():
                    times[n].append(per_call_ms(f, calls))
            mn = {n: min(v) for n, v in times.items()}
            sp = {n: max(v) - min(v) for n, v in times.items()}
            cell = {"form": form, "Q": Q, "k": k, "listed_per_Qk": listed / (Q * k), "survivors_per_Qk": surv / (Q * k),
                    "ids_where_b_differs": differ, "b_extra_bytes": Q * N * 4,
                    **{n + "_ms": [round(x, 4) for x in v] for n, v in times.items()},
                    "c_over_a": mn["c_search_deep"] / mn["a_topk10"],
                    "c_faster_than_b_beyond_spreads": bool(mn["b_similarity_topk"] - mn["c_search_deep"] >
                                                           sp["b_similarity_topk"] + sp["c_search_deep"])}
            cells[f"{form}_Q{Q}_k{k}"] = cell
            rows.append(f"{form:14s} {Q:3d} {k:5d} | {mn['a_topk10']:8.3f} {sp['a_topk10']:6.3f} | {mn['b_similarity_topk']:9.3f} "
                        f"{sp['b_similarity_topk']:7.3f} | {mn['c_search_deep']:8.3f} {sp['c_search_deep']:6.3f} | "
                        f"{cell['c_over_a']:6.2f} {mn['b_similarity_topk'] / mn['c_search_deep']:7.2f}x | "
                        f"{cell['listed_per_Qk']:6.3f} {cell['survivors_per_Qk']:6.3f} | {cell['b_extra_bytes'] / 2 ** 20:8.1f} | "
                        f"{'met' if cell['c_faster_than_b_beyond_spreads'] else 'MISSED'}")
    if args.trace:
        return
    head = [f"deep top-k, N = {N} x {E}, {warm} warm-ups, min (and max - min) over {reps} repeats of {calls} calls, ms per call",
            "gallery          Q     k | (a) top-k 10 spread | (b) similarity+topk spread | (c) search_deep spread | "
            " c / a   b / c | listed, survivors / (Q*k) | (b) score matrix MiB | bar: b - c > spread(b) + spread(c)"]
    missed = [n for n, c in cells.items() if not c["c_faster_than_b_beyond_spreads"]]
    tail = ["bar ((c) faster than (b) by more than the sum of the two spreads, every cell): " +
            ("met" if not missed else "MISSED in " + ", ".join(missed))]
    table = "\n".join(head + rows + tail)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")
    print(json.dumps({"gallery": [N, E], "warm": warm, "reps": reps, "calls": calls, "cells": cells}))


if __name__ == "__main__":
    main()
