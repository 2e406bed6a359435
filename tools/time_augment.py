"""Device time of one augmented pass (development aid): 256 random-resized crops -> [256,3,224,224], split into the tables
launch (mmr_augment_tables), the resample launch pair (mmr_augment_resample) and the batch-256 encode next to them.

    python tools/time_augment.py [--out profiles/augment_timings.txt]

Protocol: boxes from preprocess.random_resized_crop_params (seed 0), descriptors and workspace prepared once, device
events, 10 warm-ups, the minimum and max - min over 5 repeats of 20 calls, the variants alternated inside each repeat.
Sources: 256 VGA images (480 x 640) and 256 images of 1500 x 2000.  Beside them: preprocess.augment_batch end to end (host
descriptor build, allocation and upload included) and, for comparison, the host time preprocess.resample_tables takes
to build the same crops' tables (one thread, its cache cleared).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd  # noqa: E402
from mmr_amd import _lib, preprocess as P  # noqa: E402


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
    ap.add_argument("--model", default="ViT-B/32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    B, S = args.batch, 224
    model, _ = mmr_amd.load(args.model, device=dev, weights="synthetic")       # times do not depend on the weights
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    norm = [float(v) for v in P.CLIP_MEAN] + [float(v) for v in P.CLIP_STD]
    variants, host_ms, notes = {}, {}, {}
    keep = []
    for name, (H, W) in (("VGA 480 x 640", (480, 640)), ("1500 x 2000", (1500, 2000))):
        imgs = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
        images = list(imgs)
        boxes = P.random_resized_crop_params([(H, W)] * B, generator=torch.Generator().manual_seed(0))
        bx = boxes.numpy().astype(np.int64)
        sizes = np.array([[H, W]] * B, dtype=np.int64)
        ptrs = np.array([im.data_ptr() for im in images], dtype=np.int64)
        desc, kmax, max_ch, max_cw, scratch_bytes = P.crop_descriptors(ptrs, sizes, bx, S)
        tb = P.augment_tables_bytes(B, S, kmax)
        desc_d = torch.from_numpy(desc).to(dev)
        tables = torch.empty(tb, dtype=torch.uint8, device=dev)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(B, 3, S, S, dtype=torch.bfloat16, device=dev)
        keep.append((imgs, desc_d, tables, scratch, out))

        def tables_call(desc_d=desc_d, kmax=kmax, tables=tables, tb=tb):
            _lib.check(L.mmr_augment_tables(desc_d.data_ptr(), B, S, kmax, tables.data_ptr(), tb, st))

        def resample_call(desc_d=desc_d, kmax=kmax, max_ch=max_ch, max_cw=max_cw, tables=tables, tb=tb, scratch=scratch,
                          scratch_bytes=scratch_bytes, out=out):
            _lib.check(L.mmr_augment_resample(desc_d.data_ptr(), B, S, kmax, max_ch, max_cw, tables.data_ptr(), tb,
                                              scratch.data_ptr(), scratch_bytes, *norm, out.data_ptr(), _lib.MMR_BF16, 0, st))

        variants[f"{name}: tables launch"] = tables_call
        variants[f"{name}: resample launch pair"] = resample_call
        variants[f"{name}: augment_batch end to end"] = lambda images=images, boxes=boxes: P.augment_batch(images, boxes, S, out_dtype=torch.bfloat16)
        notes[name] = (f"kmax {kmax}, tables {tb / 1e6:.1f} MB, scratch {scratch_bytes / 1e6:.1f} MB, crop pixels "
                       f"{int((bx[:, 2] * bx[:, 3]).sum()) * 3 / 1e6:.0f} MB")
        P.resample_tables.cache_clear()
        t0 = time.perf_counter()
        for b in bx:
            P.resample_tables(int(b[3]), S, 0, S)
            P.resample_tables(int(b[2]), S, 0, S)
        host_ms[name] = (time.perf_counter() - t0) * 1e3
    px = torch.randn(B, 3, S, S, device=dev).bfloat16()
    model.to(torch.bfloat16)
    variants[f"encode_image, batch {B}, {args.model}"] = lambda: model.encode_image(px)

    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(5):
        for k, fn in variants.items():
            times[k].append(_events(fn, 20))
    lines = [f"one augmented pass: {B} random-resized crops (scale 0.5-1, ratio 3/4-4/3, seed 0) -> [{B},3,{S},{S}] bf16; device events, "
             f"10 warm-ups, min (max - min) over 5 repeats of 20 calls, variants alternated; {torch.cuda.get_device_name(0)}", ""]
    for k, v in times.items():
        lines.append(f"  {k:46s} {min(v):8.3f} ms ({max(v) - min(v):.3f})")
    lines.append("")
    for name in notes:
        lines.append(f"  {name}: {notes[name]}; host resample_tables for the same {2 * B} tables: {host_ms[name]:.0f} ms, one thread")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
