"""Decision-mask timings on device events (warm-up first, alternating repeats): a table, then one JSON line.

    python tools/time_decide.py [--reps 5] [--quick] [--out profiles/decide_timings.txt]

Galleries of 1M unit rows: 512-d bf16, 512-d fp16, 768-d bf16; Q in {10, 64, 256} queries.
  (a) thresholds nobody reaches (0.9): mmr_cosine_decide against mmr_cosine_range at the same queries and the same
      threshold, both through the C ABI with preallocated buffers so no host work sits between the events, and
      GalleryIndex.decide against GalleryIndex.range_search (whole Python calls, each with its read of the counts).
      The two scans differ by the deciding epilogue: one shuffle and one word store per query and tile.
  (b) Q = 10, thresholds that pass about 1/6 of the rows of each query (decide: each query's own quantile; range search:
      the one threshold that passes 1/6 of all pairs).  Range search's workspace for the candidate count is computed
      first; when it does not fit in free device memory the comparison is skipped and that is recorded.
Every repeat runs each function once, in turn; per function the table gives the minimum, the median and the spread
(max - min) over the repeats.
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
    ap.add_argument("--quick", action="store_true", help="100k-row galleries (a smoke run of the tool itself)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = 100_000 if args.quick else 1_000_000
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    res = {"rows": N, "reps": args.reps, "cases": []}
    lines = [f"decision masks vs range search, {N} unit rows, device events, {args.reps} alternating repeats after 2 warm-up rounds",
             f"{torch.cuda.get_device_name(dev)}; times in ms as min / median / spread (max - min)", ""]

    for E, dtype, name in ((512, torch.bfloat16, "bf16"), (512, torch.float16, "fp16"), (768, torch.bfloat16, "bf16")):
        g = unit_rows(N, E, 1, dtype, dev)
        index = search.GalleryIndex(g)
        code = _lib.dtype_code(dtype)
        W = (N + 31) // 32
        nb = index.norm_bound_dev.data_ptr()
        lines.append(f"== {N} x {E} {name}")
        for Q in (10, 64, 256):
            q = unit_rows(Q, E, 100 + Q, dtype, dev)
            cases = [("a: nobody passes", torch.full((Q,), 0.9, dtype=torch.float64, device=dev), 0.9)]
            if Q == 10:
                sc = q.float() @ g.float().t()
                k = N // 6
                per_query = torch.topk(sc, k, dim=1).values[:, -1].double()
                shared = float(torch.topk(sc.flatten(), Q * k).values[-1])
                cases.append(("b: 1/6 of the rows pass", per_query, shared))
                del sc
            for label, thr_dev, tau in cases:
                # one eager call of each sizes the buffers (and says whether range search fits at all)
                dm = index.decide(q, thr_dev)
                cands = dm.counts[1]
                dcap = max(cands, 1 << 16)
                dws = torch.empty(L.mmr_decide_workspace_bytes(N, E, Q, dcap, code, 0), dtype=torch.uint8, device=dev)
                words = torch.empty(Q, W, dtype=torch.int32, device=dev)
                dcounts = torch.zeros(2, dtype=torch.int64, device=dev)

                def c_decide():
                    _lib.check(L.mmr_cosine_decide(q.data_ptr(), g.data_ptr(), None, code, Q, N, E, thr_dev.data_ptr(), 0.0, nb,
                                                   None, None, dcap, words.data_ptr(), dcounts.data_ptr(), dws.data_ptr(),
                                                   dws.numel(), st))

                fns = {"decide_c": c_decide, "decide_py": lambda: index.decide(q, thr_dev, cand_cap=dcap)}
                passed = int(dm.num_set().sum())
                row = {"gallery": [N, E, name], "Q": Q, "case": label, "decide_candidates": cands, "decide_bits_set": passed,
                       "decide_workspace_bytes": dws.numel(), "decide_output_bytes": Q * W * 4}
                # range search needs room for every pair that passes plus the margin's candidates
                rcap = max(int(1.05 * passed) + cands + 4096, 1 << 16)
                rws_bytes = L.mmr_range_workspace_bytes(N, E, Q, rcap, code, 0)
                out_bytes = rcap * (4 + 4 + 4 + 8)
                free = torch.cuda.mem_get_info(dev)[0]
                row["range_workspace_bytes"], row["range_output_bytes"] = rws_bytes, out_bytes
                if rws_bytes + out_bytes > 0.8 * free:
                    row["range"] = f"skipped: needs {rws_bytes + out_bytes} bytes, {free} free"
                else:
                    rws = torch.empty(rws_bytes, dtype=torch.uint8, device=dev)
                    outs = [torch.empty(rcap, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32, torch.float64)]
                    rcounts = torch.zeros(2, dtype=torch.int64, device=dev)

                    def c_range():
                        _lib.check(L.mmr_cosine_range(q.data_ptr(), g.data_ptr(), None, code, Q, N, E, tau, 1.0, 0.0, nb, None,
                                                      rcap, rcap, *[o.data_ptr() for o in outs], rcounts.data_ptr(),
                                                      rws.data_ptr(), rws.numel(), st))

                    fns["range_c"] = c_range
                    fns["range_py"] = lambda: index.range_search(q, tau, cap=rcap, cand_cap=rcap)
                t = alternate(fns, 2, args.reps)
                torch.cuda.synchronize()
                assert dcounts.tolist()[1] <= dcap
                if "range_c" in fns:
                    m, c = rcounts.tolist()
                    assert c <= rcap and m <= rcap
                    row["range_matches"], row["range_candidates"] = m, c
                    if label.startswith("a"):
                        assert m == passed == 0
                for k_, v in t.items():
                    row[k_] = summary(v)
                res["cases"].append(row)
                lines.append(f"  Q={Q:<3d} {label}: decide sets {passed} bits, {cands} candidates, workspace {dws.numel()} B, "
                             f"masks {Q * W * 4} B; range search workspace {rws_bytes} B + outputs {out_bytes} B")
                for k_ in fns:
                    s = row[k_]
                    lines.append(f"      {k_:<10s} {s['min_ms']:9.3f} / {s['median_ms']:9.3f} / {s['spread_ms']:7.3f}")
                if "range" in row:
                    lines.append(f"      range search {row['range']}")
                del dws, words
        del index, g
        lines.append("")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
