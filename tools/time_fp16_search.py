"""fp16 gallery search timings on device events: the routes alternated inside one process; a table and one JSON line.

    python tools/time_fp16_search.py [--quick] [--out profiles/fp16_search_timings.txt]

Workload: N = 1M unit rows of E = 512 and of E = 768, top-10 of Q in {1, 32, 256} queries (128 at E = 768: one scan pass).
The same values in every route: rows generated in fp32, rounded to fp16 (routes b, c) or to bf16 (route a).
  (a)  bf16     GalleryIndex over the bf16 gallery: the route fp16 data could be cast to (it drops 3 significand bits)
  (b)  fp16     GalleryIndex over the fp16 gallery as it is: the f16 MFMA scans, same bytes and tile shapes as (a)
  (b') fp16     cosine_topk(q, g) per call on the fp16 tensor (norm bound measured per call, workspace allocated per call)
  (c)  widened  what the library did with the same fp16 tensor before it had fp16 kernels: cosine_topk per call on
                g.float() -- the copy is part of every call -- and
  (c') fp32 idx a GalleryIndex over g.float() (pre-split fp32 gallery: twice the memory, the tiered split scans)
10 warm-ups per route, then 5 repeats of 20 calls; each repeat runs the routes in turn.  Reported: the minimum over the
repeats (ms per call) and the spread (max - min) of each route.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd  # noqa: E402,F401
from mmr_amd import search  # noqa: E402


def unit_rows(n, e, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(n, e, dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 17):
        x = torch.randn(min(1 << 17, n - s), e, generator=gen, device=dev)
        out[s:s + x.shape[0]] = x / x.norm(dim=-1, keepdim=True)
    return out


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
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = 100_000 if args.quick else 1_000_000
    warm, reps, calls = (2, 2, 3) if args.quick else (10, 5, 20)
    rows, cells = [], {}
    for E, Qs in ((512, (1, 32, 256)), (768, (1, 32, 128))):
        g32 = unit_rows(N, E, dev, 7)
        g16, gbf = g32.half(), g32.bfloat16()
        del g32
        ix_bf, ix_16, ix_32 = search.GalleryIndex(gbf), search.GalleryIndex(g16), search.GalleryIndex(g16.float())
        for Q in Qs:
            q32 = unit_rows(Q, E, dev, 8)
            q16, qbf = q32.half(), q32.bfloat16()
            fns = {"a_bf16_index": lambda: ix_bf.search(qbf, 10),
                   "b_fp16_index": lambda: ix_16.search(q16, 10),
                   "b_fp16_per_call": lambda: search.cosine_topk(q16, g16, 10),
                   "c_widened_per_call": lambda: search.cosine_topk(q16.float(), g16.float(), 10),
                   "c_fp32_index": lambda: ix_32.search(q16, 10)}
            # the fp16 routes and the widened routes rank the same values: same rows, bit for bit
            ref = fns["b_fp16_index"]()
            for k in ("b_fp16_per_call", "c_widened_per_call", "c_fp32_index"):
                other = fns[k]()
                assert torch.equal(ref[1], other[1]) and torch.equal(ref[0], other[0]), k
            differs_from_bf16 = int((fns["a_bf16_index"]()[1] != ref[1]).sum())
            for _ in range(warm):
                for f in fns.values():
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k in fns}
            for _ in range(reps):
                for k, f in fns.items():
                    times[k].append(per_call_ms(f, calls))
            mn = {k: min(v) for k, v in times.items()}
            sp = {k: max(v) - min(v) for k, v in times.items()}
            cell = {"E": E, "Q": Q, "top10_slots_where_bf16_cast_differs": differs_from_bf16,
                    **{k + "_ms": [round(x, 4) for x in v] for k, v in times.items()}}
            cell["b_within_spread_of_a"] = bool(abs(mn["b_fp16_index"] - mn["a_bf16_index"]) <= max(sp["b_fp16_index"], sp["a_bf16_index"]))
            cell["b_beats_c_index_beyond_spread"] = bool(mn["c_fp32_index"] - mn["b_fp16_index"] > max(sp["c_fp32_index"], sp["b_fp16_index"]))
            cell["b_per_call_beats_c_per_call_beyond_spread"] = bool(
                mn["c_widened_per_call"] - mn["b_fp16_per_call"] > max(sp["c_widened_per_call"], sp["b_fp16_per_call"]))
            cells[f"E{E}_Q{Q}"] = cell
            rows.append(f"{E:4d} {Q:4d} | " + " | ".join(f"{mn[k]:8.3f} {sp[k]:6.3f}" for k in fns) +
                        f" | {differs_from_bf16:4d} of {Q * 10}")
        del ix_bf, ix_16, ix_32, g16, gbf
        torch.cuda.empty_cache()
    head = [f"top-10 over N = {N} unit rows, {warm} warm-ups, min (and max - min) over {reps} repeats of {calls} calls, ms per call",
            "   E    Q | (a) bf16 index spread | (b) fp16 index spread | (b') fp16 per call spread | (c) widened per call spread | "
            "(c') fp32 index spread | top-10 slots the bf16 cast changes"]
    table = "\n".join(head + rows)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")
    print(json.dumps({"N": N, "warm": warm, "reps": reps, "calls": calls, "cells": cells}))


if __name__ == "__main__":
    main()
