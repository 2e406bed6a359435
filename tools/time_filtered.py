"""Row-mask filtered search against the unmasked call, alternating in one process (development aid; bench.py is the
contract).  Device events, min of REPS repeats of ITERS calls each.

Shapes: 1M x 512 bf16 at Q = 1 / 16 / 256, 1M x 768 bf16 at Q = 128, the 1M x 512 fp32 pre-split index at Q = 128,
range search at Q = 16 and the self-join (on a smaller gallery, SJ_N rows); masks at densities 1.0, 0.5 and 0.01,
applied as deletions of a GalleryIndex (the live-row buffer every later search passes).  Also times what compaction
costs instead: gallery[keep] + the norm-bound pass (+ the split for fp32) + one search on the copy.

    python tools/time_filtered.py            # env: N, REPS, ITERS, SJ_N, ONLY=topk,range,join,compact
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mmr_amd import search

dev = torch.device("cuda:0")
N = int(os.environ.get("N", 1_000_000))
REPS, ITERS = int(os.environ.get("REPS", 5)), int(os.environ.get("ITERS", 10))
SJ_N = int(os.environ.get("SJ_N", 200_000))
ONLY = set(os.environ.get("ONLY", "topk,range,join,compact").split(","))
DENS = (1.0, 0.5, 0.01)


def unit(n, e, dtype, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, e, device=dev, generator=gen)
    return (x / x.norm(dim=-1, keepdim=True)).to(dtype)


def timed(fns, reps=REPS, iters=ITERS):
    """min over reps of the mean ms per call, the callables alternating rep by rep"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    best = [float("inf")] * len(fns)
    for _ in range(reps):
        for i, f in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                f()
            e.record()
            torch.cuda.synchronize()
            best[i] = min(best[i], s.elapsed_time(e) / iters)
    return best


def masked_index(g, dens, seed, presplit=None):
    ix = search.GalleryIndex(g, presplit=presplit)
    if dens < 1.0:
        gen = torch.Generator(device=dev).manual_seed(seed)
        dead = torch.nonzero(torch.rand(g.shape[0], device=dev, generator=gen) >= dens).flatten()
        ix.delete_rows(dead)
    else:
        ix.delete_rows(torch.empty(0, dtype=torch.int64))     # density 1.0 through the masked path (all-ones mask)
    return ix


def row(label, plain, masked):
    print(f"{label:44s} unmasked {plain:8.3f} ms  masked {masked:8.3f} ms  ratio {masked / plain:6.3f}", flush=True)


if "topk" in ONLY:
    for E, dtype, Qs, presplit in ((512, torch.bfloat16, (1, 16, 256), None), (768, torch.bfloat16, (128,), None),
                                   (512, torch.float32, (128,), True)):
        g = unit(N, E, dtype, 1)
        plain = search.GalleryIndex(g, presplit=presplit)
        for dens in DENS:
            ix = masked_index(g, dens, 2, presplit)
            for Q in Qs:
                q = unit(Q, E, dtype, 3)
                a, b = timed([lambda: plain.search(q, 10), lambda: ix.search(q, 10)])
                row(f"top-k {N}x{E} {str(dtype)[6:]} Q={Q} density {dens}", a, b)
            del ix
        del plain, g
        torch.cuda.empty_cache()

if "range" in ONLY:
    g = unit(N, 512, torch.bfloat16, 1)
    q = unit(16, 512, torch.bfloat16, 3)
    plain = search.GalleryIndex(g)
    for dens in DENS:
        ix = masked_index(g, dens, 2)
        a, b = timed([lambda: plain.range_search(q, 0.3, cand_cap=1 << 20),
                      lambda: ix.range_search(q, 0.3, cand_cap=1 << 20)])
        row(f"range {N}x512 bf16 Q=16 t=0.3 density {dens}", a, b)
    del plain, g
    torch.cuda.empty_cache()

if "join" in ONLY:
    g = unit(SJ_N, 512, torch.bfloat16, 1)
    plain = search.GalleryIndex(g)
    for dens in DENS:
        ix = masked_index(g, dens, 2)
        a, b = timed([lambda: plain.near_duplicates(0.5, cand_cap=1 << 20),
                      lambda: ix.near_duplicates(0.5, cand_cap=1 << 20)], reps=3, iters=2)
        row(f"self-join {SJ_N}x512 bf16 t=0.5 density {dens}", a, b)
    del plain, g
    torch.cuda.empty_cache()

if "compact" in ONLY:
    for E, dtype in ((512, torch.bfloat16), (512, torch.float32)):
        g = unit(N, E, dtype, 1)
        keep = torch.rand(N, device=dev) < 0.5
        ix = search.GalleryIndex(g, presplit=dtype == torch.float32)
        ix.delete_rows(torch.nonzero(~keep).flatten())
        q = unit(128, E, dtype, 3)

        def compact():
            c = search.GalleryIndex(g[keep], presplit=dtype == torch.float32)   # copy + norm bound (+ split)
            c.search(q, 10)

        a, b = timed([compact, lambda: ix.search(q, 10)], reps=3, iters=2)
        print(f"compaction {N}x{E} {str(dtype)[6:]} 50%: gallery[keep] + norm bound"
              f"{' + split' if dtype == torch.float32 else ''} + search {a:8.3f} ms; one masked search {b:8.3f} ms",
              flush=True)
        del ix, g
        torch.cuda.empty_cache()
