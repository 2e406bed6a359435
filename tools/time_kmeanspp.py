"""k-means++ seeding timings on device events (warm-up first, alternating repeats): a table, then one JSON line.

    python tools/time_kmeanspp.py [--rows 1000000] [--reps 5] [--quick] [--no-sklearn] [--out profiles/kmeanspp_timings.txt]

N bf16 rows drawn around 64 unit centres, E in (512, 768), K in (8, 64), L = 2 + int(ln K) trials per step, euclidean.
mmr_kmeanspp_seed is called through the C ABI with preallocated buffers and the norm bound as a device scalar, so no
host work sits between the events; the time covers the whole call (3 launches per step).  Every repeat runs each case
once, in turn.  Beside the times: the time per step, and the time the step's gallery bytes (2 N E) take at the HBM rate
the scans reach (5.7-6.0 TB/s; 5.85 is used) as a fraction of it -- 1.0 would be a pass that does
nothing but stream the gallery.  The step also writes 8 L bytes of trial weights per row and reads 16.

--sklearn (default when sklearn imports): sklearn.cluster.kmeans_plusplus on the same rows as fp32, one run per case, on
OMP_NUM_THREADS threads (unset: the CPUs the process may use).
Then, with no pass mark: on assign_helpers.planted_clusters at N = 100k (E = 128, 16 clusters, bf16) the Lloyd iterations
and the final inertia of kmeans from "k-means++" and from "sample", averaged over 8 generators.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mmr_amd  # noqa: E402,F401
from mmr_amd import _lib, cluster, search  # noqa: E402
from time_range import alternate  # noqa: E402

HBM_TBS = 5.85


def rows_around_centres(N, E, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(64, E, device=dev, generator=g), dim=-1)
    out = torch.empty(N, E, dtype=torch.bfloat16, device=dev)
    for s in range(0, N, 1 << 17):
        n = min(1 << 17, N - s)
        x = centres[torch.randint(0, 64, (n,), device=dev, generator=g)] + 2.5 * torch.randn(n, E, device=dev, generator=g) / E ** 0.5
        out[s:s + n] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="100k rows, 2 repeats (a smoke run of the tool itself)")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = 100_000 if args.quick else args.rows
    reps = 2 if args.quick else args.reps
    L_ = _lib.lib()
    st = _lib.stream_ptr(dev)
    props = torch.cuda.get_device_properties(dev)
    try:
        from sklearn.cluster import kmeans_plusplus as sk_kpp
    except ImportError:
        sk_kpp = None
    if args.no_sklearn:
        sk_kpp = None

    cases, keep = {}, []
    galleries = {E: rows_around_centres(N, E, dev, 10 + E) for E in (512, 768)}
    for E, g in galleries.items():
        nb = search.gallery_norm_bound(g)
        for K in (8, 64):
            L = cluster.kmeanspp_trials(K)
            var = cluster.kmeanspp_variates(K, L, torch.Generator().manual_seed(K + E)).to(dev)
            ws = torch.empty(L_.mmr_kmeanspp_workspace_bytes(N, E, K, L), dtype=torch.uint8, device=dev)
            idx = torch.empty(K, dtype=torch.int32, device=dev)
            pot = torch.empty(K, dtype=torch.int64, device=dev)
            sh = torch.empty(1, dtype=torch.int32, device=dev)
            cen = torch.empty(K, E, dtype=g.dtype, device=dev)
            keep.append((nb, var, ws, idx, pot, sh, cen))

            def call(g=g, E=E, K=K, L=L, nb=nb, var=var, ws=ws, idx=idx, pot=pot, sh=sh, cen=cen):
                _lib.check(L_.mmr_kmeanspp_seed(g.data_ptr(), _lib.MMR_BF16, N, E, K, L, 0, None, var.data_ptr(), 0.0, nb.data_ptr(),
                                                idx.data_ptr(), pot.data_ptr(), sh.data_ptr(), cen.data_ptr(), ws.data_ptr(),
                                                ws.numel(), st))
            cases[f"E{E}-K{K}"] = (call, E, K, L, ws.numel())

    times = alternate({k: v[0] for k, v in cases.items()}, 2, reps)
    torch.cuda.synchronize()
    threads = int(os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0)))       # what sklearn's BLAS and OpenMP use
    res = {"rows": N, "reps": reps, "device": props.name, "hbm_tbs": HBM_TBS, "cpus": threads,
           "sklearn": sk_kpp is not None, "cases": {}}
    lines = [f"k-means++ seeding, {N} bf16 rows, euclidean; device events, {reps} alternating repeats after 2 warm-up rounds; {props.name}",
             f"whole call in ms as min / median / spread (max - min); per step = min / K; HBM share = (2 N E bytes at {HBM_TBS} TB/s) / per step",
             ""]
    for name, ts in times.items():
        _, E, K, L, wsb = cases[name]
        best = min(ts)
        step_us = best / K * 1e3
        hbm_us = 2.0 * N * E / (HBM_TBS * 1e12) * 1e6
        row = {"E": E, "K": K, "L": L, "min_ms": best, "median_ms": round(statistics.median(ts), 4), "spread_ms": round(max(ts) - best, 4),
               "all_ms": ts, "step_us": round(step_us, 2), "hbm_us": round(hbm_us, 2), "hbm_share": round(hbm_us / step_us, 4),
               "workspace_mb": round(wsb / 2 ** 20, 1)}
        line = (f"  E={E} K={K:<3d} L={L}  {best:9.3f} / {row['median_ms']:9.3f} / {row['spread_ms']:7.3f}   {step_us:8.1f} us per step   "
                f"{row['hbm_share']:.3f} of it is the gallery at the HBM rate ({hbm_us:.0f} us)   workspace {row['workspace_mb']} MiB")
        if sk_kpp is not None:
            X = galleries[E].float().cpu().numpy()
            t0 = time.perf_counter()
            sk_kpp(X, K, random_state=0)
            row["sklearn_s"] = round(time.perf_counter() - t0, 3)
            row["speedup_vs_sklearn"] = round(row["sklearn_s"] * 1e3 / best, 1)
            line += f"   sklearn on {res['cpus']} CPU threads {row['sklearn_s']:.2f} s ({row['speedup_vs_sklearn']:.0f}x)"
            del X
        res["cases"][name] = row
        lines.append(line)
    if sk_kpp is None:
        lines.append("  sklearn.cluster.kmeans_plusplus was not timed (" + ("--no-sklearn" if args.no_sklearn else "sklearn is not installed here") + ")")

    # Lloyd from the two starts, no pass mark
    import assign_helpers as A
    g = A.planted_clusters(100_000, 128, 16, 321, torch.bfloat16)[0].to(dev)
    lloyd = {}
    for init in ("k-means++", "sample"):
        runs = [cluster.kmeans(g, 16, init=init, generator=torch.Generator().manual_seed(500 + i)) for i in range(8)]
        lloyd[init] = {"n_iter": [r.n_iter for r in runs], "inertia": [round(r.inertia, 3) for r in runs],
                       "converged": [bool(r.converged) for r in runs],
                       "empty_clusters": [int((r.sizes == 0).sum()) for r in runs]}
        lines.append(f"  kmeans(N=100000, E=128, K=16, planted_clusters) from {init!r:<12s}: mean iterations "
                     f"{statistics.mean(lloyd[init]['n_iter']):.1f} (of {lloyd[init]['n_iter']}), mean inertia "
                     f"{statistics.mean(lloyd[init]['inertia']):.2f} (min {min(lloyd[init]['inertia']):.2f}, max {max(lloyd[init]['inertia']):.2f})")
    res["lloyd"] = lloyd
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
