"""Rates of the JPEG decode (development aid): 256 VGA 4:2:0 quality-85 files of smooth synthetic content.

    python tools/time_jpeg_decode.py [--out profiles/jpeg_decode.json]

In one run:
  (a) what callers do today: Image.open(f).convert("RGB") on 16 threads, then the upload of the pixels -- the baseline;
  (b) the entropy stage (mmr_jpeg_entropy_decode) on 16 threads, images/s;
  (c) the two kernels of one prepared call (jpeg.JpegPlan.run), device events, 10 warm-ups, the minimum and max - min over 5
      repeats of 20 calls, beside a device copy of as many bytes as the kernels must move (coefficients in, planes out and
      back in, RGB out: about 9 B/px at 4:2:0) -- the rate a pure streaming kernel reaches on this GPU;
  (d) decode_jpeg_batches end to end over --batches batches, images/s, and the ratio (d) / (a);
  (e) the device entropy stage alone (jpeg.DeviceEntropyResult.run, one workgroup per image), device events as in (c), at
      subseq_bytes 64, 128, 256 and 512 with the rounds the images took, its coefficients compared with (b)'s, and the host
      work that is left in front of it (headers, packing the scan bytes);
  (f) decode_jpeg_batches(entropy="device") end to end, as (d).
Host clocks end in a device synchronise.  Needs a GPU: there is nothing to time without one.
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
from mmr_amd import jpeg  # noqa: E402


def make_files(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    files = []
    for _ in range(n):
        low = Image.fromarray(rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8))
        buf = io.BytesIO()
        low.resize((w, h), Image.BICUBIC).save(buf, "JPEG", quality=85, subsampling="4:2:0")
        files.append(buf.getvalue())
    return files


def _pillow(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


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
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("time_jpeg_decode needs the GPU")
    dev = torch.device("cuda:0")
    B, H, W = args.images, args.height, args.width
    files = make_files(B, H, W)
    res = {"device": torch.cuda.get_device_name(0), "images": B, "height": H, "width": W, "file_bytes": sum(len(f) for f in files),
           "threads": args.threads, "protocol": "host clocks around work that ends in a device synchronise, min of 3; kernels: device "
           "events, 10 warm-ups, min (max - min) over 5 repeats of 20 calls"}

    # (a) Pillow on 16 threads + upload
    ta = []
    with ThreadPoolExecutor(max_workers=args.threads) as pool:
        for _ in range(3):
            t0 = time.perf_counter()
            up = [torch.from_numpy(a).to(dev) for a in pool.map(_pillow, files)]
            torch.cuda.synchronize()
            ta.append(time.perf_counter() - t0)
    res["a_pillow_threads_plus_upload_images_per_s"] = B / min(ta)

    # (b) the entropy stage
    tb, store = [], {}

    def reuse(n):           # one buffer for every repeat, as decode_jpeg_batches reuses its staging: fresh pages are not the stage's cost
        if store.get("buf") is None or store["buf"].size < n:
            store["buf"] = np.zeros(n, dtype=np.int16)
        return store["buf"]

    for _ in range(4):
        t0 = time.perf_counter()
        host = jpeg.entropy_decode(files, threads=args.threads, alloc=reuse)
        tb.append(time.perf_counter() - t0)
    assert not host.status.any()
    res["b_entropy_stage_images_per_s"] = B / min(tb[1:])

    # (c) the two kernels
    plan = jpeg.JpegPlan(host, dev).upload()
    ours = plan.run().images()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(ours, up)), "decoded pixels differ from Pillow's"
    planes = plan.total_blocks * 64
    moved = host.coef_bytes + 2 * planes + 3 * B * H * W
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
    res.update(c_two_kernels_ms=kms, c_two_kernels_spread_ms=max(times["kernels"]) - kms, c_bytes_moved=moved,
               c_bytes_per_pixel=moved / (B * H * W), c_device_copy_of_as_many_bytes_ms=cms,
               c_device_copy_rate_TB_per_s=moved / cms / 1e9, c_fraction_of_the_copy_rate=cms / kms,
               c_kernels_images_per_s=B / kms * 1e3)

    # (d) end to end, overlapped
    td = []
    for _ in range(3):
        t0 = time.perf_counter()
        n = 0
        for imgs in jpeg.decode_jpeg_batches((files for _ in range(args.batches)), device=dev, on_unsupported="raise", threads=args.threads):
            n += len(imgs)
        torch.cuda.synchronize()
        td.append(time.perf_counter() - t0)
    res["d_decode_jpeg_batches_images_per_s"] = n / min(td)
    res["ratio_d_over_a"] = res["d_decode_jpeg_batches_images_per_s"] / res["a_pillow_threads_plus_upload_images_per_s"]

    # (e) the device entropy stage alone
    tp = []
    for _ in range(4):
        t0 = time.perf_counter()
        prep = jpeg.ScanBatch(files)
        tp.append(time.perf_counter() - t0)
    res["e_host_headers_and_packing_images_per_s"] = B / min(tp[1:])
    res["e_scan_bytes_uploaded"] = int(prep.desc["scan_bytes"].sum())
    want = torch.from_numpy(host.coef[: host.coef_bytes // 2]).to(dev)
    per_size = {}
    for S in (64, 128, 256, 512):
        stage = jpeg.DeviceEntropyResult(prep, dev, subseq_bytes=S).upload().run()
        assert not stage.status.any(), stage.status
        assert torch.equal(stage.coef_dev[: want.numel()], want), "device coefficients differ from the host stage's"
        for _ in range(10):
            stage.run()
        torch.cuda.synchronize()
        ts = [_events(stage.run, 20) for _ in range(5)]
        per_size[S] = dict(ms=min(ts), spread_ms=max(ts) - min(ts), images_per_s=B / min(ts) * 1e3, rounds_min=int(stage.rounds.min()),
                           rounds_mean=float(stage.rounds.mean()), rounds_max=int(stage.rounds.max()), subsequences_mean=float(stage.subsequences.mean()))
    best = min(per_size, key=lambda S: per_size[S]["ms"])
    res.update(e_device_entropy_by_subseq_bytes={str(S): v for S, v in per_size.items()}, e_best_subseq_bytes=best, e_default_subseq_bytes=jpeg.SUBSEQ_BYTES,
               e_device_entropy_ms=per_size[jpeg.SUBSEQ_BYTES]["ms"], e_device_entropy_spread_ms=per_size[jpeg.SUBSEQ_BYTES]["spread_ms"],
               e_device_entropy_images_per_s=per_size[jpeg.SUBSEQ_BYTES]["images_per_s"])

    # (f) end to end with the entropy stage on the device
    tf = []
    for _ in range(3):
        t0 = time.perf_counter()
        n = 0
        for imgs in jpeg.decode_jpeg_batches((files for _ in range(args.batches)), device=dev, on_unsupported="raise", threads=args.threads, entropy="device"):
            n += len(imgs)
        torch.cuda.synchronize()
        tf.append(time.perf_counter() - t0)
    assert all(torch.equal(x, y) for x, y in zip(imgs, up)), "entropy=\"device\": decoded pixels differ from Pillow's"
    res["f_decode_jpeg_batches_entropy_device_images_per_s"] = n / min(tf)
    res["ratio_f_over_d"] = res["f_decode_jpeg_batches_entropy_device_images_per_s"] / res["d_decode_jpeg_batches_images_per_s"]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
