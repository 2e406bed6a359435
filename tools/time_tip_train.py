"""Device time of one Tip-Adapter-F step: the fused call (mmr_tip_adapter_f_step, two launches) against the same step written
in eager torch (fp32 autograd + torch.optim.AdamW, the reference's own path, code/main_custom.py:172-189) on the same GPU
in the same process.  Device events around windows of --steps steps, warm-up first, alternating repeats; a table, then one
JSON line.

    python tools/time_tip_train.py [--steps 1000] [--reps 5] [--quick] [--out profiles/tip_train_timings.txt]

A window is enqueued back to back and the device is never waited on inside it, so a figure is the rate at which steps
complete: the larger of the device time of a step and the host's time to enqueue one (for the fused call one ctypes call;
for eager torch its two dozen launches).  For the two kernels' own durations give rocprofv3 the fused steps alone, in a
run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/time_tip_train.py --fused-only --shape 0

Shapes (B,S,C,E): (256,96,6,512), the reference's (6 classes x 16 shots, batch 256, ViT-B), and (1024,1024,64,768).  bf16
features for the fused call (widened exactly to fp32 inside); the eager step gets the same values as fp32 tensors, so it
does no conversion.  Both paths keep every tensor on the device and read nothing back inside the window.  The eager
step's kernel launches are counted with torch.profiler in a pass of their own, after the timing.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mmr_amd as clip  # noqa: E402
import tip_train_helpers as H  # noqa: E402
from time_range import alternate  # noqa: E402

SHAPES = ((256, 96, 6, 512), (1024, 1024, 64, 768))
ALPHA, BETA, LR0 = 1.0, 5.5, 1e-3


class EagerStep:
    """run_tip_adapter_F's loop body in fp32 torch on the device."""

    def __init__(self, inp, dev, total_steps):
        self.f, self.y = inp["features"].float().to(dev), inp["targets"].to(dev)
        self.wc, self.v = inp["clip_weights"].float().to(dev), inp["cache_values"].to(dev)
        E, S = inp["cache_keys"].shape
        self.adapter = torch.nn.Linear(E, S, bias=False).to(dev)
        self.adapter.weight = torch.nn.Parameter(inp["cache_keys"].t().float().contiguous().to(dev))
        self.opt = torch.optim.AdamW(self.adapter.parameters(), lr=LR0, eps=1e-4)
        self.sched = torch.optim.lr_scheduler.CosineAnnealingLR(self.opt, total_steps)

    def step(self):
        affinity = self.adapter(self.f)
        cache_logits = ((-1) * (BETA - BETA * affinity)).exp() @ self.v * 10
        tip_logits = 100. * self.f @ self.wc + cache_logits * ALPHA
        loss = torch.nn.functional.cross_entropy(tip_logits, self.y)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        self.sched.step()
        return loss


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000, help="steps per timed window")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="20 steps, 2 repeats (a smoke run of the tool itself)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--fused-only", action="store_true", help="200 fused steps per shape and nothing else (for a profiler)")
    ap.add_argument("--shape", type=int, default=None, help="with --fused-only: 0 or 1, that shape alone")
    args = ap.parse_args()
    if args.fused_only:
        dev = torch.device("cuda:0")
        for B, S, C, E in (SHAPES if args.shape is None else SHAPES[args.shape:args.shape + 1]):
            inp = H.make_inputs(B, S, C, E, seed=1)
            t = clip.TipAdapterF(inp["cache_keys"].to(dev), inp["cache_values"].to(dev), inp["clip_weights"].to(dev), ALPHA,
                                 BETA, lr=LR0, total_steps=200)
            f, y = inp["features"].to(dev), inp["targets"].to(dev)
            for _ in range(200):
                t.step(f, y)
            torch.cuda.synchronize()
            print(f"({B},{S},{C},{E}): 200 fused steps done")
        return
    dev = torch.device("cuda:0")
    steps, reps = (20, 2) if args.quick else (args.steps, args.reps)
    total = steps * (reps + 3) + 8
    props = torch.cuda.get_device_properties(dev)

    fns, objs = {}, {}
    for B, S, C, E in SHAPES:
        inp = H.make_inputs(B, S, C, E, seed=1)
        t = clip.TipAdapterF(inp["cache_keys"].to(dev), inp["cache_values"].to(dev), inp["clip_weights"].to(dev), ALPHA, BETA,
                             lr=LR0, total_steps=total)
        f, y = inp["features"].to(dev), inp["targets"].to(dev)
        eager = EagerStep(inp, dev, total)
        objs[(B, S, C, E)] = (t, f, y, eager)

        def fused(t=t, f=f, y=y):
            for _ in range(steps):
                t.step(f, y)

        def torch_eager(eager=eager):
            for _ in range(steps):
                eager.step()

        fns[f"{B},{S},{C},{E} fused"] = fused
        fns[f"{B},{S},{C},{E} eager"] = torch_eager

    times = alternate(fns, 2, reps)
    torch.cuda.synchronize()
    res = {"steps_per_window": steps, "reps": reps, "device": props.name, "cases": {}}
    lines = [f"Tip-Adapter-F step, device events around windows of {steps} steps, {reps} alternating repeats after 2 warm-up "
             f"windows; {props.name}", "us per step as min / median over the windows", ""]
    for shape in SHAPES:
        B, S, C, E = shape
        t, f, y, eager = objs[shape]
        row = {}
        for part in ("fused", "eager"):
            ts = [1e3 * ms / steps for ms in times[f"{B},{S},{C},{E} {part}"]]
            row[part] = {"min_us": round(min(ts), 2), "median_us": round(statistics.median(ts), 2)}
        try:
            row["eager"]["launches"] = count_launches(eager.step)
            row["fused"]["launches"] = count_launches(lambda: t.step(f, y))
        except Exception as e:       # the profiler is optional equipment: the times stand without it
            row["launches_error"] = repr(e)
        row["speedup_min"] = round(row["eager"]["min_us"] / row["fused"]["min_us"], 2)
        res["cases"][f"{B},{S},{C},{E}"] = row
        lines.append(f"  (B,S,C,E) = ({B},{S},{C},{E}): fused {row['fused']['min_us']:8.2f} / {row['fused']['median_us']:8.2f} us, "
                     f"{row['fused'].get('launches', '?')} launches;  eager torch {row['eager']['min_us']:8.2f} / "
                     f"{row['eager']['median_us']:8.2f} us, {row['eager'].get('launches', '?')} launches;  x{row['speedup_min']}")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(table + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
