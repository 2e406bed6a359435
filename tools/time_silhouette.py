"""Silhouette sums on device events (warm-up first, alternating repeats, one process): a table, then one JSON line.

    python tools/time_silhouette.py [--reps 5] [--quick] [--out profiles/silhouette_timings.txt]

A gallery of 100 000 x 512 unit rows, bf16 and fp16, random labels at K = 2, 4 and 64, and 100 000 x 128 at K = 4.  Every
function goes through the C ABI with preallocated buffers, so no host work sits between the events:
  sil_K<k>        mmr_silhouette_sums, euclidean: the full N x N square
  sil_cos_K4      the same with the cosine epilogue (no square root)
  self_join       mmr_gallery_self_join on the same gallery at a threshold no pair reaches: the same ring over the
                  triangle, half of silhouette's pairs -- the yardstick
Every repeat runs each function once, in turn; per function the table gives the minimum, the median and the spread
(max - min) over the repeats, the ratio of the medians to the yardstick's and the pairs per second.
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
    ap.add_argument("--quick", action="store_true", help="a 20k-row gallery (a smoke run of the tool itself)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = 20_000 if args.quick else 100_000
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    res = {"rows": N, "reps": args.reps, "cases": []}
    lines = [f"silhouette sums, {N} unit rows, device events, {args.reps} alternating repeats after 2 warm-up rounds",
             f"{torch.cuda.get_device_name(dev)}; times in ms as min / median / spread (max - min)", ""]
    for E, dtype, name, ks in ((512, torch.bfloat16, "bf16", (2, 4, 64)), (512, torch.float16, "fp16", (2, 4, 64)),
                               (128, torch.bfloat16, "bf16", (4,))):
        g = unit_rows(N, E, 1, dtype, dev)
        code = _lib.dtype_code(dtype)
        nb = search.gallery_norm_bound(g)
        fns, keep, row = {}, [], {"gallery": [N, E, name]}
        for K, metric in [(k, 0) for k in ks] + [(4, 1)]:
            labels = torch.randint(0, K, (N,), generator=torch.Generator().manual_seed(K), dtype=torch.int32).to(dev)
            ws = torch.empty(L.mmr_silhouette_workspace_bytes(N, E, K, code), dtype=torch.uint8, device=dev)
            sums = torch.empty(N, K, dtype=torch.float64, device=dev)
            sizes = torch.empty(K, dtype=torch.int64, device=dev)
            keep.append((labels, ws, sums, sizes))

            def c_sil(labels=labels, ws=ws, sums=sums, sizes=sizes, K=K, metric=metric):
                _lib.check(L.mmr_silhouette_sums(g.data_ptr(), code, N, E, labels.data_ptr(), K, metric, sums.data_ptr(),
                                                 sizes.data_ptr(), ws.data_ptr(), ws.numel(), st))

            fns[f"sil_cos_K{K}" if metric else f"sil_K{K}"] = c_sil
        cap = 1 << 16
        jws = torch.empty(L.mmr_range_workspace_bytes(N, E, 0, cap, code, 0), dtype=torch.uint8, device=dev)
        oi, oj = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
        osc = torch.empty(cap, dtype=torch.float32, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)

        def c_join():
            _lib.check(L.mmr_gallery_self_join(g.data_ptr(), None, code, N, E, 1.5, 1.0, 0.0, nb.data_ptr(), None, cap, cap,
                                               oi.data_ptr(), oj.data_ptr(), osc.data_ptr(), None, counts.data_ptr(),
                                               jws.data_ptr(), jws.numel(), st))

        fns["self_join"] = c_join
        t = alternate(fns, 2, args.reps)
        torch.cuda.synchronize()
        assert counts.tolist() == [0, 0] and int(keep[0][3].sum()) == N
        lines.append(f"== {N} x {E} {name}")
        for k_, v in t.items():
            row[k_] = summary(v)
        base = row["self_join"]["median_ms"]
        for k_ in t:
            s = row[k_]
            pairs = N * N if k_ != "self_join" else N * (N - 1) // 2
            s["over_self_join"] = round(s["median_ms"] / base, 3)
            s["gpairs_per_s"] = round(pairs / s["median_ms"] / 1e6, 2)
            lines.append(f"      {k_:<11s} {s['min_ms']:9.3f} / {s['median_ms']:9.3f} / {s['spread_ms']:7.3f}   "
                         f"x{s['over_self_join']:<6.2f} of self_join   {s['gpairs_per_s']:8.2f} Gpairs/s")
        # where one call's time goes: the library's launch profiler, one call
        k_ = f"sil_K{ks[-1]}"
        _lib.prof_enable(True)
        fns[k_]()
        torch.cuda.synchronize()
        split = {c_: round(ms, 4) for c_, (ms, n) in ((a, b) for a, b in _lib.prof_read().items() if a != "dropped") if n}
        _lib.prof_enable(False)
        row[k_ + "_split_ms"] = split
        lines.append(f"      {k_:<11s} by launch class: " + ", ".join(f"{a} {b:.3f}" for a, b in split.items()))
        res["cases"].append(row)
        del g, keep
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
