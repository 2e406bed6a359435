"""Device time of mmr_image_hashes (development aid): B uint8 [H,W,3] images -> phash, dhash, whash.

    python tools/time_image_hash.py [--out profiles/image_hash_timings.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o image_hash -- python tools/time_image_hash.py --calls 20     # per-kernel split

Protocol: one prepared call (dedup.ImageHashPlan: descriptors and tables uploaded once), device events, 10 warm-ups, the
minimum and max - min over 5 repeats of 20 calls, the variants alternated inside each repeat.  Beside it: a device copy of
the same bytes (the rate a pure streaming kernel reaches on this GPU), dedup.image_hashes end to end (host descriptor
build included) and, for information, the PIL oracle's time per image on this host.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmr_amd import dedup  # noqa: E402


def _events(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--calls", type=int, default=0, help="profile mode: this many calls of the three-kind plan, nothing else")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    B, H, W = args.batch, args.height, args.width
    imgs = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
    nbytes = imgs.numel()
    if args.calls:
        plan = dedup.ImageHashPlan(imgs, 8)
        for _ in range(args.calls):
            plan.run()
        torch.cuda.synchronize()
        return 0

    variants = {}
    for hs in (8, 16):
        variants[f"all three kinds, hash_size {hs}"] = dedup.ImageHashPlan(imgs, hs).run
        variants[f"dhash only,      hash_size {hs}"] = dedup.ImageHashPlan(imgs, hs, kinds=("dhash",)).run
    copy_dst = torch.empty_like(imgs)
    variants["device copy of the pixels (read + write)"] = lambda: copy_dst.copy_(imgs)
    variants["dedup.image_hashes end to end, hash_size 8"] = lambda: dedup.image_hashes(imgs, 8)
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(5):
        for k, fn in variants.items():
            times[k].append(_events(fn, 20))

    import PIL
    from PIL import Image
    one = Image.fromarray(imgs[0].cpu().numpy(), "RGB")
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        L = one.convert("L")
        for size in ((9, 8), (32, 32), (256, 256)):
            L.resize(size, Image.LANCZOS)
    pil_ms = (time.perf_counter() - t0) / reps * 1e3

    copy_ms = min(times["device copy of the pixels (read + write)"])
    rate = 2 * nbytes / copy_ms / 1e9                       # TB/s: bytes / ms / 1e9
    lines = [f"image hashes, {B} images of {H} x {W} x 3 uint8 ({nbytes / 1e6:.0f} MB); device events, 10 warm-ups, min (max - min) over 5 "
             f"repeats of 20 calls, variants alternated; {torch.cuda.get_device_name(0)}",
             f"stream time = the pixels read once at the device copy's rate ({rate:.2f} TB/s) = {nbytes / rate / 1e9:.3f} ms", ""]
    for k, v in times.items():
        lo = min(v)
        lines.append(f"  {k:46s} {lo:8.3f} ms ({max(v) - lo:.3f})   {B / lo * 1e3:10.0f} images/s   {nbytes / lo / 1e9:6.3f} TB/s of pixels"
                     f"   {lo / (nbytes / rate / 1e9):6.1f} x stream time")
    lines += ["", f"for information: Pillow {PIL.__version__} on this host, convert('L') + the three LANCZOS resizes of hash_size 8 "
                  f"(no DCT, no median): {pil_ms:.2f} ms per image, one thread"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
