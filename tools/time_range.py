"""Threshold search and gallery self-join timings on device events (warm-up first, alternating repeats); one JSON line.

    python tools/time_range.py [--reps 3] [--quick]

  range:      mmr_cosine_range over 1M x 512 bf16 at Q in {1, 16, 256} with a threshold that leaves about 1e4 matches in
              all, against GalleryIndex.search (cosine_topk, k = 10) on the same index; the C call is timed with
              preallocated buffers so no host work sits between the events
  self-join:  1M x 512 bf16 (both work orders) and 200k x 768 bf16 with planted duplicates, 1M x 512 fp32 through a
              pre-split GalleryIndex; whole Python call (includes the read of the 16-byte counts)
  torch:      chunked torch.mm + (>= tau) + nonzero over the same galleries (upper triangle for the self-join)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd  # noqa: E402,F401
from mmr_amd import _lib, search  # noqa: E402


def unit_rows(n, e, seed, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(n, e, dtype=dtype, device=dev)
    for s in range(0, n, 131072):
        x = torch.randn(min(n, s + 131072) - s, e, generator=g, device=dev)
        out[s:s + x.shape[0]] = (x / x.norm(dim=-1, keepdim=True)).to(dtype)
    return out


def plant(g, pairs, seed):
    gen = torch.Generator(device=g.device).manual_seed(seed)
    idx = torch.randperm(g.shape[0], generator=gen, device=g.device)[:2 * pairs]
    src, dst = idx[:pairs], idx[pairs:]
    x = g[src].float() + torch.randn(pairs, g.shape[1], generator=gen, device=g.device) * (0.05 / g.shape[1] ** 0.5)
    g[dst] = (x / x.norm(dim=-1, keepdim=True)).to(g.dtype)


def ev(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def alternate(fns, warm, reps):
    """{name: [ms, ...]}: every repeat runs each function once, in turn."""
    for _ in range(warm):
        for f in fns.values():
            ev(f)
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(round(ev(f)[0], 4))
    return times


def torch_range(q, g, tau, chunk=131072):
    out = []
    for s in range(0, g.shape[0], chunk):
        sc = q @ g[s:s + chunk].t()
        nz = torch.nonzero(sc >= tau)
        nz[:, 1] += s
        out.append(nz)
    return torch.cat(out)


def torch_self_join(g, tau, chunk=1024):       # chunk x N < 2^31: torch.nonzero counts in int32
    out = []
    for s in range(0, g.shape[0], chunk):
        sc = g[s:s + chunk] @ g[s:].t()
        nz = torch.nonzero(sc >= tau)
        nz = nz[nz[:, 1] > nz[:, 0]]
        nz[:, 0] += s
        nz[:, 1] += s
        out.append(nz)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="100k-row galleries (a smoke run of the tool itself)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = 100_000 if args.quick else 1_000_000
    E = 512
    res = {"gallery": [N, E], "reps": args.reps}
    L = _lib.lib()
    st = _lib.stream_ptr(dev)

    # ---- range search
    g = unit_rows(N, E, 1, torch.bfloat16, dev)
    index = search.GalleryIndex(g)
    rng = {}
    for Q in (1, 16, 256):
        q = unit_rows(Q, E, 100 + Q, torch.bfloat16, dev)
        sc = (q.float() @ g.float().t()).flatten()
        tau = float(torch.topk(sc, 10_000).values[-1])
        del sc
        cand_cap = 1 << 16
        ws = torch.empty(L.mmr_range_workspace_bytes(N, E, Q, cand_cap, _lib.MMR_BF16, 0), dtype=torch.uint8, device=dev)
        outs = [torch.empty(cand_cap, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32, torch.float64)]
        counts = torch.zeros(2, dtype=torch.int64, device=dev)

        def c_range():
            _lib.check(L.mmr_cosine_range(q.data_ptr(), g.data_ptr(), None, _lib.MMR_BF16, Q, N, E, tau, 1.0, 0.0,
                                          index.norm_bound_dev.data_ptr(), None, cand_cap, cand_cap,
                                          *[o.data_ptr() for o in outs], counts.data_ptr(), ws.data_ptr(), ws.numel(), st))

        t = alternate({"range_c": c_range, "range_py": lambda: index.range_search(q, tau),
                       "topk10": lambda: index.search(q, 10), "torch": lambda: torch_range(q, g, tau)}, 2, args.reps)
        torch.cuda.synchronize()
        m, c = counts.tolist()
        want = torch_range(q.float(), g.float(), tau).shape[0]
        rng[f"Q{Q}"] = {"tau": tau, "matches": m, "candidates": c, "torch_fp32_matches": want,
                        **{k + "_ms": v for k, v in t.items()},
                        **{k + "_min_ms": min(v) for k, v in t.items()}}
    res["range_1M_bf16"] = rng
    del index

    # ---- self-join, 1M x 512 bf16, both work orders
    plant(g, 1000, 7)
    sj = {}
    for order in ("chunk", "block"):
        os.environ["MMR_RANGE_ORDER"] = order
        ev(lambda: search.gallery_self_join(g, 0.9))
        ts = [round(ev(lambda: search.gallery_self_join(g, 0.9))[0], 2) for _ in range(args.reps)]
        sj[f"order_{order}_ms"] = ts
    os.environ.pop("MMR_RANGE_ORDER")
    i, j, _, _ = search.gallery_self_join(g, 0.9)
    sj["pairs"] = int(i.numel())
    ev(lambda: torch_self_join(g, 0.9))
    tt, nz = ev(lambda: torch_self_join(g, 0.9))
    sj["torch_ms"] = round(tt, 2)
    sj["torch_pairs"] = int(nz.shape[0])
    best = min(sj["order_chunk_ms"])
    sj["tflops_chunk_order"] = round(N * (N - 1) / 2 * E * 2 / (best * 1e-3) / 1e12, 1)
    res["self_join_1M_512_bf16"] = sj
    del g

    # ---- self-join, 200k x 768 bf16
    n2 = N // 5
    g2 = unit_rows(n2, 768, 2, torch.bfloat16, dev)
    plant(g2, 500, 8)
    t = alternate({"mmr": lambda: search.gallery_self_join(g2, 0.9), "torch": lambda: torch_self_join(g2, 0.9)}, 1, args.reps)
    i, _, _, _ = search.gallery_self_join(g2, 0.9)
    res["self_join_200k_768_bf16"] = {"pairs": int(i.numel()), **{k + "_ms": v for k, v in t.items()}}
    del g2

    # ---- self-join, 1M x 512 fp32 through a pre-split GalleryIndex
    g3 = unit_rows(N, E, 3, torch.float32, dev)
    plant(g3, 1000, 9)
    ix = search.GalleryIndex(g3)
    ev(lambda: ix.near_duplicates(0.9))
    ts = [round(ev(lambda: ix.near_duplicates(0.9))[0], 2) for _ in range(args.reps)]
    i, _, _, _ = ix.near_duplicates(0.9)
    res["self_join_1M_512_fp32_index"] = {"pairs": int(i.numel()), "mmr_ms": ts}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
