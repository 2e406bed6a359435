"""Nearest-centroid assignment and cluster sums on device events (warm-up first, alternating repeats, one process): a
table, then one JSON line.

    python tools/time_assign.py [--reps 5] [--quick] [--out profiles/assign_timings.txt]

A gallery of 1M x 512 unit rows, bf16 and fp16.  Every function goes through the C ABI with preallocated buffers, so no
host work sits between the events:
  assign_K256 / assign_K1024   mmr_cosine_assign with the euclidean bias, best64 included
  decide_Q256                  mmr_cosine_decide at Q = 256 on the same operands (thresholds nobody reaches): the same ring
                               and the same MFMA count as one assign pass -- the yardstick
  sums_K1024                   mmr_cluster_sums over the labels of assign_K1024
Every repeat runs each function once, in turn; per function the table gives the minimum, the median and the spread
(max - min) over the repeats, and the assign calls' ambiguous-row counts.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd  # noqa: E402,F401
from mmr_amd import _lib, search  # noqa: E402
from time_range import alternate, unit_rows  # noqa: E402


def summary(ts):
    return {"min_ms": round(min(ts), 4), "median_ms": round(statistics.median(ts), 4), "spread_ms": round(max(ts) - min(ts), 4),
            "all_ms": ts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a 100k-row gallery (a smoke run of the tool itself)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, E = (100_000 if args.quick else 1_000_000), 512
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    res = {"rows": N, "E": E, "reps": args.reps, "cases": []}
    lines = [f"nearest-centroid assignment, {N} x {E} unit rows, device events, {args.reps} alternating repeats after 2 warm-up rounds",
             f"{torch.cuda.get_device_name(dev)}; times in ms as min / median / spread (max - min)", ""]
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        g = unit_rows(N, E, 1, dtype, dev)
        code = _lib.dtype_code(dtype)
        nb = search.gallery_norm_bound(g)
        fns, keep, row = {}, [], {"gallery": [N, E, name]}
        labels_1024 = None
        for K in (256, 1024):
            c = unit_rows(K, E, 100 + K, dtype, dev)
            bias = -0.5 * c.double().square().sum(1)
            labels, _, (_, amb) = search.cosine_assign(g, c, bias, return_score=True, return_counts=True)   # sizes the list
            cap = max(amb, 1 << 16)
            ws = torch.empty(L.mmr_assign_workspace_bytes(N, E, K, cap, code), dtype=torch.uint8, device=dev)
            out = torch.empty(N, dtype=torch.int32, device=dev)
            best = torch.empty(N, dtype=torch.float64, device=dev)
            counts = torch.zeros(2, dtype=torch.int64, device=dev)
            keep.append((c, bias, ws, out, best, counts))

            def c_assign(c=c, bias=bias, ws=ws, out=out, best=best, counts=counts, K=K, cap=cap):
                _lib.check(L.mmr_cosine_assign(g.data_ptr(), c.data_ptr(), code, N, K, E, bias.data_ptr(), 0.0, nb.data_ptr(), None,
                                               cap, out.data_ptr(), best.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), st))

            fns[f"assign_K{K}"] = c_assign
            row[f"ambiguous_K{K}"] = amb
            row[f"assign_workspace_bytes_K{K}"] = ws.numel()
            if K == 256:
                Q, W = 256, (N + 31) // 32
                thr = torch.full((Q,), 0.9, dtype=torch.float64, device=dev)
                dws = torch.empty(L.mmr_decide_workspace_bytes(N, E, Q, 1 << 16, code, 0), dtype=torch.uint8, device=dev)
                words = torch.empty(Q, W, dtype=torch.int32, device=dev)
                dcounts = torch.zeros(2, dtype=torch.int64, device=dev)

                def c_decide(c=c, thr=thr, dws=dws, words=words, dcounts=dcounts, Q=Q):
                    _lib.check(L.mmr_cosine_decide(c.data_ptr(), g.data_ptr(), None, code, Q, N, E, thr.data_ptr(), 0.0,
                                                   nb.data_ptr(), None, None, 1 << 16, words.data_ptr(), dcounts.data_ptr(),
                                                   dws.data_ptr(), dws.numel(), st))

                fns["decide_Q256"] = c_decide
            else:
                labels_1024 = labels
        K = 1024
        sws = torch.empty(L.mmr_cluster_sums_workspace_bytes(N, E, K), dtype=torch.uint8, device=dev)
        sums = torch.empty(K, E, dtype=torch.float64, device=dev)
        sizes = torch.empty(K, dtype=torch.int64, device=dev)

        def c_sums():
            _lib.check(L.mmr_cluster_sums(g.data_ptr(), code, N, E, labels_1024.data_ptr(), K, sums.data_ptr(), sizes.data_ptr(),
                                          sws.data_ptr(), sws.numel(), st))

        fns["sums_K1024"] = c_sums
        t = alternate(fns, 2, args.reps)
        torch.cuda.synchronize()
        assert int(sizes.sum()) == N
        lines.append(f"== {N} x {E} {name}: ambiguous rows {row['ambiguous_K256']} (K=256), {row['ambiguous_K1024']} (K=1024)")
        for k_, v in t.items():
            row[k_] = summary(v)
            s = row[k_]
            lines.append(f"      {k_:<13s} {s['min_ms']:9.3f} / {s['median_ms']:9.3f} / {s['spread_ms']:7.3f}")
        row["assign_K256_over_decide_Q256"] = round(row["assign_K256"]["median_ms"] / row["decide_Q256"]["median_ms"], 3)
        lines.append(f"      assign_K256 / decide_Q256 (medians): {row['assign_K256_over_decide_Q256']}")
        # where one call's time goes: the library's launch profiler, one call each
        for k_ in ("assign_K256", "assign_K1024", "decide_Q256"):
            _lib.prof_enable(True)
            fns[k_]()
            torch.cuda.synchronize()
            split = {c_: round(ms, 4) for c_, (ms, n) in ((a, b) for a, b in _lib.prof_read().items() if a != "dropped") if n}
            _lib.prof_enable(False)
            row[k_ + "_split_ms"] = split
            lines.append(f"      {k_:<13s} by launch class: " + ", ".join(f"{a} {b:.3f}" for a, b in split.items()))
        res["cases"].append(row)
        del g, keep
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
