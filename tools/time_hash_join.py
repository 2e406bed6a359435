"""Perceptual-hash self-join timings on device events (warm-up first, alternating repeats): a table, then one JSON line.

    python tools/time_hash_join.py [--rows 1000000] [--reps 5] [--quick] [--out profiles/hash_join_timings.txt]

N rows of H = 3 random 64-bit hashes (W = 1), thresholds 5 / 5 / 5 -- the reference's same-folder rule:
  random    nothing matches (an accidental pair within distance 5 has probability about 5e-13 per pair and kind)
  planted   1 % of the rows are near copies of other rows (up to 5 flipped bits per hash): N / 100 matching pairs
mmr_hash_self_join is called through the C ABI with preallocated buffers, so no host work sits between the events; the
time covers the join kernel, the radix sort of the `cap` slots and the emit.  Every repeat runs each case once, in turn.

Beside the times: pair evaluations per second (the kernel evaluates whole tiles: tiles x 1024^2 pairs, the diagonal
tiles in full) and the fraction of the VALU-issue bound, from the hot loop's instruction count read off the compiled
kernel (tests/test_hash_join_isa.py pins it: 133 VALU instructions per step of 8 pairs) -- a wave's VALU instruction
occupies its SIMD for 2 cycles, 4 SIMDs per CU, so a CU retires 128 lane-instructions per cycle -- at the clock the
device reports (its nominal maximum; the clock held under load is lower, so the fraction understates how close to its
own bound the kernel runs).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd  # noqa: E402,F401
from mmr_amd import _lib  # noqa: E402
from time_range import alternate  # noqa: E402

TILE = 1024
VALU_PER_PAIR = 133 / 8             # H = 3, W = 1: tests/test_hash_join_isa.py
LANES_PER_CU_CYCLE = 128            # 4 SIMDs x 64 lanes / 2 cycles per wave instruction


def random_hashes(n, H, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    hi, lo = (torch.randint(0, 2 ** 32, (n, H, 1), dtype=torch.int64, device=dev, generator=g) for _ in range(2))
    return (hi << 32) | lo


def plant(h, pairs, seed):
    """rows dst = rows src with up to 5 bits flipped in every hash"""
    dev = h.device
    g = torch.Generator(device=dev).manual_seed(seed)
    idx = torch.randperm(h.shape[0], generator=g, device=dev)[:2 * pairs]
    src, dst = idx[:pairs], idx[pairs:]
    flips = torch.zeros(pairs, h.shape[1], 1, dtype=torch.int64, device=dev)
    for _ in range(5):
        flips |= torch.ones_like(flips) << torch.randint(0, 64, flips.shape, generator=g, device=dev)
    h[dst] = h[src] ^ flips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="100k rows (a smoke run of the tool itself)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H, W = (100_000 if args.quick else args.rows), 3, 1
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    props = torch.cuda.get_device_properties(dev)
    cus = props.multi_processor_count
    khz = getattr(props, "clock_rate", 0)
    ghz = khz / 1e6 if khz else 2.4
    clock_src = "reported by the device" if khz else "not reported: the 2.4 GHz of the data sheet"

    cap = 1 << 16
    thr = (ctypes.c_int32 * H)(5, 5, 5)
    ws = torch.empty(L.mmr_hash_join_workspace_bytes(0, N, H, W, cap), dtype=torch.uint8, device=dev)
    oi, oj = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
    od = torch.empty(cap, dtype=torch.int64, device=dev)
    counts = {}
    data = {"random": random_hashes(N, H, 1, dev), "planted": random_hashes(N, H, 2, dev)}
    plant(data["planted"], N // 100, 3)

    def call(name):
        h = data[name]
        c = counts.setdefault(name, torch.zeros(1, dtype=torch.int64, device=dev))
        return lambda: _lib.check(L.mmr_hash_self_join(h.data_ptr(), N, H, W, thr, None, cap, oi.data_ptr(), oj.data_ptr(),
                                                       od.data_ptr(), c.data_ptr(), ws.data_ptr(), ws.numel(), st))

    times = alternate({k: call(k) for k in data}, 2, args.reps)
    torch.cuda.synchronize()
    ntile = (N + TILE - 1) // TILE
    evals = ntile * (ntile + 1) // 2 * TILE * TILE
    bound_ms = evals * VALU_PER_PAIR / (cus * LANES_PER_CU_CYCLE * ghz * 1e9) * 1e3
    res = {"rows": N, "H": H, "W": W, "thresholds": [5, 5, 5], "cap": cap, "reps": args.reps, "device": props.name, "cus": cus,
           "clock_ghz": ghz, "clock_source": clock_src, "pairs": N * (N - 1) // 2, "pair_evaluations": evals,
           "valu_per_pair": VALU_PER_PAIR, "valu_bound_ms": round(bound_ms, 3), "cases": {}}
    lines = [f"hash self-join, {N} rows x {H} hashes x {W} word, thr 5/5/5, cap {cap}; device events, {args.reps} alternating "
             "repeats after 2 warm-up rounds",
             f"{props.name}: {cus} CUs, {ghz:.3f} GHz ({clock_src}); {evals:.4g} pair evaluations in {ntile * (ntile + 1) // 2} tiles "
             f"for {N * (N - 1) // 2:.4g} pairs; VALU-issue bound {bound_ms:.2f} ms at {VALU_PER_PAIR:.3f} VALU per pair",
             "times in ms as min / median / spread (max - min)", ""]
    for name, ts in times.items():
        m = counts[name].item()
        assert m <= cap, (name, m)
        best = min(ts)
        row = {"matches": m, "min_ms": best, "median_ms": round(statistics.median(ts), 4), "spread_ms": round(max(ts) - best, 4),
               "all_ms": ts, "pair_evaluations_per_s": evals / (best * 1e-3), "pairs_per_s": res["pairs"] / (best * 1e-3),
               "fraction_of_valu_bound": round(bound_ms / best, 4)}
        res["cases"][name] = row
        lines.append(f"  {name:<8s} {m:>7d} matches  {best:9.3f} / {row['median_ms']:9.3f} / {row['spread_ms']:7.3f}   "
                     f"{row['pair_evaluations_per_s']:.4g} pair evaluations/s   {row['fraction_of_valu_bound']:.3f} of the VALU bound")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
