"""Time of the Tip-Adapter (beta, alpha) grid search: the device call (tip_adapter_grid: three launches per chunk of beta
and one read of the status word) against what the package offered before it -- a host loop that calls tip_adapter_logits
once per grid point, copies the logits to the host and runs the reference's threshold search and confusion matrix there
(tests/tip_grid_helpers.py, in its faster histogram formulation, which is bit-identical to the literal loop).  Device
events around each whole search, warm-up first, alternating repeats, the minimum; a table, then one JSON line.

    python tools/time_tip_grid.py [--reps 3] [--grids 50x20,200x20] [--device-only] [--out profiles/tip_grid_timings.txt]

Size: the reference's own, N = 2000 rows, S = 96 (6 classes x 16 shots), C = 6, E = 512, bf16.  The reference ships no
config, so the grid sizes are this tool's choice: 50 x 20 and 200 x 20 over search_scale = [7, 3].  For the three
kernels' own durations give rocprofv3 the device call alone, in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/time_tip_grid.py --device-only --grids 50x20
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mmr_amd as clip  # noqa: E402
import tip_grid_helpers as G  # noqa: E402
from time_range import alternate  # noqa: E402

N, S, C, E = 2000, 96, 6, 512


def host_loop(d, labels_np, betas, alphas):
    """The search as the parent of this call could run it: one fused scoring call per grid point, metrics on the host."""
    best, pick = 0.0, (0, 0)
    for beta in betas:
        for alpha in alphas:
            logits = clip.tip_adapter_logits(d["features"], d["clip_weights"], d["cache_keys"], d["cache_values"], alpha, beta)
            logits = logits.cpu().numpy()
            f1 = G.threshold_table(logits, labels_np, G.find_thresholds_hist)["f1"]
            G.confusion(logits, labels_np)
            score = G.mean_f1(f1, range(C - 1))
            if score > best:
                best, pick = score, (beta, alpha)
    return pick


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grids", default="50x20,200x20")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    inp = G.make_inputs(N, S, C, E, dtype=torch.bfloat16)
    d = {k: v.to(dev) for k, v in inp.items()}
    labels_np = inp["labels"].numpy()
    rows, lines = [], []
    for spec in args.grids.split(","):
        nb, na = (int(x) for x in spec.split("x"))
        cfg = dict(search_hp=True, search_scale=[7, 3], search_step=[nb, na])
        betas, alphas = clip.tip_adapter.search_lists(cfg)

        def device():
            return clip.search_hp(cfg, d["cache_keys"], d["cache_values"], d["features"], d["labels"], d["clip_weights"])

        fns = {"device": device}
        if not args.device_only:
            fns["host_loop"] = lambda: host_loop(d, labels_np, betas, alphas)
        times = alternate(fns, 1, args.reps)
        row = dict(grid=spec, N=N, S=S, C=C, E=E, device_ms=min(times["device"]), device_all=times["device"])
        picks = {"device": device()}
        if not args.device_only:
            row.update(host_loop_ms=min(times["host_loop"]), host_loop_all=times["host_loop"],
                       ratio=round(min(times["host_loop"]) / min(times["device"]), 1))
            picks["host_loop"] = fns["host_loop"]()
        row["picks"] = {k: [float(v[0]), float(v[1])] for k, v in picks.items()}
        rows.append(row)
        lines.append(f"grid {spec:>7}: device {row['device_ms']:9.3f} ms"
                     + ("" if args.device_only else f"   host loop {row['host_loop_ms']:10.1f} ms   x{row['ratio']}")
                     + f"   picks {row['picks']}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(tool="time_tip_grid", rows=rows)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
