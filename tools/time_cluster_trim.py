"""mmr_cluster_rank + mmr_cluster_percentile_trim timings on device events (warm-up first, alternating repeats): a table,
then one JSON line.

    python tools/time_cluster_trim.py [--rows 1000000] [--dim 512] [--reps 5] [--quick] [--out profiles/cluster_trim_timings.txt]

N bf16 rows drawn around 64 unit centres, random labels in [0, K) for K = 1, 10 and 1000, cosine metric, q = 95.  The two C
calls run through the ABI with preallocated buffers, so no host work sits between the events.  Beside them:
  * mmr_cluster_sums on the same rows and labels -- also a whole-row gather by sorted id, the yardstick from before
    these calls existed;
  * the time 2 N E bytes take at the HBM rate the scans reach (5.85 TB/s), as a fraction of the
    call -- 1.0 would be a call that does nothing but stream the gallery once;
  * the whole Python ``trimmed_centers`` (cluster_sums -> rank -> trim -> cluster_sums, with its allocations).
Every repeat runs each case once, in turn.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmr_amd  # noqa: E402,F401
from mmr_amd import _lib, cluster  # noqa: E402
from time_kmeanspp import rows_around_centres  # noqa: E402
from time_range import alternate  # noqa: E402

HBM_TBS = 5.85
KS = (1, 10, 1000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="100k rows, 2 repeats (a smoke run of the tool itself)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = 100_000 if args.quick else args.rows
    reps = 2 if args.quick else args.reps
    E = args.dim
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    props = torch.cuda.get_device_properties(dev)
    g = rows_around_centres(N, E, dev, 10 + E)

    fns, keep = {}, []
    for K in KS:
        lab = torch.randint(0, K, (N,), device=dev, generator=torch.Generator(device=dev).manual_seed(K)).to(torch.int32)
        sums, sizes = cluster.cluster_sums(g, lab, K)
        c32 = (sums / sizes.clamp(min=1).to(torch.float64)[:, None]).to(torch.float32).contiguous()
        ws = torch.empty(L.mmr_cluster_rank_workspace_bytes(N, E, K), dtype=torch.uint8, device=dev)
        ws_s = torch.empty(L.mmr_cluster_sums_workspace_bytes(N, E, K), dtype=torch.uint8, device=dev)
        dist = torch.empty(N, dtype=torch.float64, device=dev)
        order = torch.empty(N, dtype=torch.int32, device=dev)
        start = torch.empty(K + 1, dtype=torch.int64, device=dev)
        thr = torch.empty(K, dtype=torch.float64, device=dev)
        trimmed = torch.empty(N, dtype=torch.int32, device=dev)
        kept = torch.empty(K, dtype=torch.int64, device=dev)
        keep.append((lab, c32, ws, ws_s, dist, order, start, thr, trimmed, kept, sums, sizes))

        def rank(K=K, lab=lab, c32=c32, ws=ws, dist=dist, order=order, start=start):
            _lib.check(L.mmr_cluster_rank(g.data_ptr(), _lib.MMR_BF16, N, E, lab.data_ptr(), K, c32.data_ptr(), 1, dist.data_ptr(),
                                          order.data_ptr(), start.data_ptr(), ws.data_ptr(), ws.numel(), st))

        def rank_trim(K=K, lab=lab, rank=rank, dist=dist, order=order, start=start, thr=thr, trimmed=trimmed, kept=kept):
            rank()
            _lib.check(L.mmr_cluster_percentile_trim(dist.data_ptr(), order.data_ptr(), start.data_ptr(), lab.data_ptr(), N, K, 95.0,
                                                     thr.data_ptr(), trimmed.data_ptr(), kept.data_ptr(), st))

        def sums_only(K=K, lab=lab, ws_s=ws_s, sums=sums, sizes=sizes):
            _lib.check(L.mmr_cluster_sums(g.data_ptr(), _lib.MMR_BF16, N, E, lab.data_ptr(), K, sums.data_ptr(), sizes.data_ptr(),
                                          ws_s.data_ptr(), ws_s.numel(), st))

        def whole(K=K, lab=lab):
            cluster.trimmed_centers(g, lab, K)

        fns[f"K{K}-rank"] = rank
        fns[f"K{K}-rank+trim"] = rank_trim
        fns[f"K{K}-cluster_sums"] = sums_only
        fns[f"K{K}-trimmed_centers"] = whole

    times = alternate(fns, 2, reps)
    torch.cuda.synchronize()
    hbm_ms = 2.0 * N * E / (HBM_TBS * 1e12) * 1e3
    res = {"rows": N, "E": E, "reps": reps, "device": props.name, "hbm_tbs": HBM_TBS, "hbm_ms": round(hbm_ms, 4), "cases": {}}
    lines = [f"cluster rank + percentile trim, {N} x {E} bf16, cosine, q = 95; device events, {reps} alternating repeats after 2 "
             f"warm-up rounds; {props.name}",
             f"ms as min / median; HBM share = (2 N E bytes at {HBM_TBS} TB/s = {hbm_ms:.3f} ms) / min", ""]
    for K in KS:
        row = {}
        for part in ("rank", "rank+trim", "cluster_sums", "trimmed_centers"):
            ts = times[f"K{K}-{part}"]
            row[part] = {"min_ms": min(ts), "median_ms": round(statistics.median(ts), 4), "all_ms": ts}
        rt, cs = row["rank+trim"]["min_ms"], row["cluster_sums"]["min_ms"]
        row["hbm_share"] = round(hbm_ms / rt, 4)
        row["vs_cluster_sums"] = round(rt / cs, 3)
        res["cases"][f"K{K}"] = row
        lines.append(f"  K={K:<5d} rank {row['rank']['min_ms']:8.3f} / {row['rank']['median_ms']:8.3f}   rank + trim {rt:8.3f} / "
                     f"{row['rank+trim']['median_ms']:8.3f}   HBM share {row['hbm_share']:.3f}   cluster_sums {cs:8.3f} / "
                     f"{row['cluster_sums']['median_ms']:8.3f} ({row['vs_cluster_sums']:.2f}x of it)   trimmed_centers "
                     f"{row['trimmed_centers']['min_ms']:8.3f} / {row['trimmed_centers']['median_ms']:8.3f}")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
