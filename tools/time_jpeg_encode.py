"""Rates of the JPEG encode (development aid): 256 VGA images at quality 95, 4:2:0 -- the decodes of the decode timer's files.

    python tools/time_jpeg_encode.py [--out profiles/jpeg_encode.json]

In one run:
  (a) what callers do today: the download of the pixels, then Image.fromarray(x).save(buf, "JPEG", quality=95) on 16
      threads -- the baseline;
  (b) the two kernels of one prepared call (jpeg.JpegEncodePlan.run), device events, 10 warm-ups, the minimum and max - min
      over 5 repeats of 20 calls, beside a device copy of as many bytes as the kernels must move (pixels in, planes out and
      back in, coefficients out: about 7.5 B/px at 4:2:0) -- the rate a pure streaming kernel reaches on this GPU;
  (c) the host Huffman stage (mmr_jpeg_entropy_encode) on 16 threads, images/s, and the download of the coefficients;
  (d) encode_jpeg_batches end to end over --batches batches, images/s, and the ratio (d) / (a).
The files of (d) are compared with those of (a) byte for byte.  Host clocks end in a device synchronise.  Needs a GPU:
there is nothing to time without one.
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mmr_amd import jpeg  # noqa: E402
from time_jpeg_decode import _events, make_files  # noqa: E402


def _pillow_save(px):
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, "JPEG", quality=95, subsampling="4:2:0")
    return buf.getvalue()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("time_jpeg_encode needs the GPU")
    dev = torch.device("cuda:0")
    B, H, W = args.images, args.height, args.width
    images = [x.clone() for x in jpeg.decode_jpeg(make_files(B, H, W), device=dev, on_unsupported="raise")]
    torch.cuda.synchronize()
    res = {"device": torch.cuda.get_device_name(0), "images": B, "height": H, "width": W, "quality": 95, "subsampling": "4:2:0",
           "threads": args.threads, "protocol": "host clocks around work that ends in a device synchronise, min of 3; kernels: device "
           "events, 10 warm-ups, min (max - min) over 5 repeats of 20 calls"}

    # (a) download + Pillow on 16 threads
    ta = []
    with ThreadPoolExecutor(max_workers=args.threads) as pool:
        for _ in range(3):
            t0 = time.perf_counter()
            theirs = list(pool.map(_pillow_save, [x.cpu().numpy() for x in images]))
            ta.append(time.perf_counter() - t0)
    res["a_download_plus_pillow_threads_images_per_s"] = B / min(ta)
    res["file_bytes"] = sum(len(f) for f in theirs)

    # (b) the two kernels
    plan = jpeg.JpegEncodePlan(images, 95, "4:2:0").run()
    torch.cuda.synchronize()
    planes = plan.total_blocks * 64
    moved = 3 * B * H * W + 2 * planes + plan.coef_bytes
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    variants = {"kernels": plan.run, "copy": lambda: dst.copy_(src)}
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(5):
        for k, fn in variants.items():
            times[k].append(_events(fn, 20))
    kms, cms = min(times["kernels"]), min(times["copy"])
    res.update(b_two_kernels_ms=kms, b_two_kernels_spread_ms=max(times["kernels"]) - kms, b_bytes_moved=moved,
               b_bytes_per_pixel=moved / (B * H * W), b_device_copy_of_as_many_bytes_ms=cms,
               b_device_copy_rate_TB_per_s=moved / cms / 1e9, b_fraction_of_the_copy_rate=cms / kms,
               b_kernels_images_per_s=B / kms * 1e3)

    # (c) the download of the coefficients and the host Huffman stage
    pinned = torch.empty(plan.coef_dev.numel(), dtype=torch.int16, pin_memory=True)
    tdl = []
    for _ in range(4):
        t0 = time.perf_counter()
        pinned.copy_(plan.coef_dev, non_blocking=True)
        torch.cuda.synchronize()
        tdl.append(time.perf_counter() - t0)
    res.update(c_coefficient_bytes=plan.coef_bytes, c_coefficient_download_ms=min(tdl[1:]) * 1e3)
    coef = pinned.numpy()
    tc = []
    for _ in range(4):
        t0 = time.perf_counter()
        files, status = jpeg.entropy_encode(coef, plan.coef_off, plan.infos, plan.qt, threads=args.threads)
        tc.append(time.perf_counter() - t0)
    assert not status.any() and files == theirs, "files differ from Pillow's"
    res["c_entropy_stage_images_per_s"] = B / min(tc[1:])

    # (d) end to end, overlapped
    td, gaps = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        n, stamps = 0, []
        for files in jpeg.encode_jpeg_batches((images for _ in range(args.batches)), threads=args.threads):
            n += len(files)
            stamps.append(time.perf_counter())
        torch.cuda.synchronize()
        td.append(time.perf_counter() - t0)
        gaps += list(np.diff(stamps[1:]))              # batch to batch, once the pipeline is full
    assert files == theirs, "encode_jpeg_batches: files differ from Pillow's"
    res["d_encode_jpeg_batches_images_per_s"] = n / min(td)
    if gaps:
        res["d_first_result_ms"] = (stamps[0] - t0) * 1e3
        res["d_steady_state_images_per_s"] = B / float(np.median(gaps))
    res["ratio_d_over_a"] = res["d_encode_jpeg_batches_images_per_s"] / res["a_download_plus_pillow_threads_images_per_s"]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
