"""A row mask per query (``row_masks=``) against what serves the same result without it (development aid; bench.py is the
contract).  Device events, min over REPS repeats of the mean of ITERS calls, the callables alternating in one process.

Per shape and Q, three timings:
  (a) per-query   one call with Q masks: ``search_deep(q, k, row_masks=m)`` / ``threshold_sweep(..., row_masks=m)``
  (b) loop        Q calls of the single-mask form, one query and one mask each -- each streams the whole gallery
  (c) shared      ONE single-mask call with all Q queries and one mask: the same gallery bytes as (a), no per-query words
and the ratios (a)/(c) -- what the per-query words cost -- and (b)/(a) -- what the one pass saves.

Shapes: 1M x 512 bf16 and 1M x 768 bf16 at Q = 6 / 24 / 32 / 256; deep top-k at k = 10 and k = 100, the labelled
threshold sweep at T = 200.  Masks: random, half the rows live per query.

    python tools/time_query_masks.py            # env: N, REPS, ITERS, QS=6,24,32,256
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mmr_amd import search

dev = torch.device("cuda:0")
N = int(os.environ.get("N", 1_000_000))
REPS, ITERS = int(os.environ.get("REPS", 3)), int(os.environ.get("ITERS", 5))
QS = tuple(int(x) for x in os.environ.get("QS", "6,24,32,256").split(","))
T = 200


def unit(n, e, dtype, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, e, device=dev, generator=gen)
    return (x / x.norm(dim=-1, keepdim=True)).to(dtype)


def timed(fns, iters):
    for f in fns:
        f()
    torch.cuda.synchronize()
    best = [float("inf")] * len(fns)
    for _ in range(REPS):
        for i, (f, it) in enumerate(zip(fns, iters)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(it):
                f()
            e.record()
            torch.cuda.synchronize()
            best[i] = min(best[i], s.elapsed_time(e) / it)
    return best


def row(label, a, b, c):
    print(f"{label:46s} (a) per-query {a:9.3f} ms  (b) loop {b:9.3f} ms  (c) shared {c:9.3f} ms   a/c {a / c:6.3f}  b/a {b / a:7.2f}",
          flush=True)


print(f"N={N} REPS={REPS} ITERS={ITERS} (the loop: 1 iteration per repeat); masks: random, 50 % live per query", flush=True)
for E in (512, 768):
    g = unit(N, E, torch.bfloat16, 1)
    ix = search.GalleryIndex(g)
    labels = torch.randint(0, 6, (N,), device=dev, dtype=torch.int32)
    grid = np.linspace(-0.2, 0.2, T)
    for Q in QS:
        q = unit(Q, E, torch.bfloat16, 3)
        gen = torch.Generator(device=dev).manual_seed(4)
        keep = torch.rand(Q, N, device=dev, generator=gen) < 0.5
        m = search.DecisionMasks.from_bool(keep)
        targets = (torch.arange(Q, device=dev) % 6).to(torch.int32)
        for k in (10, 100):
            a, b, c = timed([lambda: ix.search_deep(q, k, row_masks=m),
                             lambda: [ix.search_deep(q[i:i + 1], k, row_mask=keep[i]) for i in range(Q)],
                             lambda: ix.search_deep(q, k, row_mask=keep[0])], (ITERS, 1, ITERS))
            row(f"deep top-k {N}x{E} bf16 Q={Q} k={k}", a, b, c)
        a, b, c = timed([lambda: ix.threshold_sweep(q, labels, targets, grid, row_masks=m),
                         lambda: [ix.threshold_sweep(q[i:i + 1], labels, targets[i:i + 1], grid, row_mask=keep[i]) for i in range(Q)],
                         lambda: ix.threshold_sweep(q, labels, targets, grid, row_mask=keep[0])], (ITERS, 1, ITERS))
        row(f"sweep T={T} {N}x{E} bf16 Q={Q}", a, b, c)
        del keep, m
    del ix, g
    torch.cuda.empty_cache()
