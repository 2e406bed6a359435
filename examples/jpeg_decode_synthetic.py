"""The image path from FILES instead of from decoded pixels, and proof that nothing changes:

    synthetic pixels -> Pillow-written JPEG bytes (quality 95, as tool/Image format conversion.py:62 writes them)
        -> decode_jpeg (Huffman stage on host threads, everything after it on the GPU; and once more with
           entropy="device", the Huffman stage on the GPU as well)
        -> image_hashes, preprocess_batch -> encode_image

and the same steps from ``Image.open(f).convert("RGB")`` pixels, the call every image flow of the reference starts with.
The pixels, the hashes and the features of the two paths are asserted equal bit for bit.  One progressive file rides
along: the device decoder reports it and ``decode_jpeg`` hands it to Pillow, so the list is complete either way.

    python examples/jpeg_decode_synthetic.py [--images 24] [--model tiny-test] [--seed 0]
"""
import argparse
import io
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd  # noqa: E402
from mmr_amd import jpeg, preprocess  # noqa: E402


def synthetic_files(n, seed=0):
    """n JPEG files of a few sizes and samplings: smooth structure plus a little texture, one greyscale, one progressive"""
    rng = np.random.default_rng(seed)
    shapes = [(120, 160), (160, 120), (97, 131), (144, 144), (75, 200)]
    files = []
    for r in range(n):
        h, w = shapes[r % len(shapes)]
        low = Image.fromarray(rng.integers(0, 256, (h // 16 + 2, w // 16 + 2, 3), dtype=np.uint8))
        px = np.asarray(low.resize((w, h), Image.BICUBIC)).astype(np.int16) + rng.integers(-5, 6, (h, w, 3))
        im = Image.fromarray(np.clip(px, 0, 255).astype(np.uint8))
        save = dict(quality=95)
        if r % 7 == 3:
            im = im.convert("L")
        elif r % 7 == 5:
            save["progressive"] = True
        else:
            save["subsampling"] = ("4:2:0", "4:2:2", "4:4:4")[r % 3]
        buf = io.BytesIO()
        im.save(buf, "JPEG", **save)
        files.append(buf.getvalue())
    return files


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--model", default="tiny-test")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    files = synthetic_files(args.images, args.seed)

    ours, status = jpeg.decode_jpeg(files, device=dev, return_status=True)
    theirs = []
    for f in files:
        with Image.open(io.BytesIO(f)) as im:
            theirs.append(torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8)).to(dev))
    assert all(torch.equal(a, b) for a, b in zip(ours, theirs)), "decoded pixels differ from Pillow's"
    # the same call with the Huffman stage on the GPU too: only scan bytes and Huffman tables go up; same pixels, same statuses
    on_gpu, status_gpu = jpeg.decode_jpeg(files, device=dev, return_status=True, entropy="device")
    assert np.array_equal(status, status_gpu) and all(torch.equal(a, b) for a, b in zip(ours, on_gpu)), "entropy=\"device\" differs"

    model, _ = mmr_amd.load(args.model, device=dev)
    n_px = model.cfg.vision.image_size
    out = []
    for imgs in (ours, theirs):
        hashes = mmr_amd.image_hashes(imgs)
        feats = model.encode_image(preprocess.preprocess_batch(imgs, n_px))
        out.append((hashes, feats))
    assert torch.equal(out[0][0], out[1][0]), "hashes differ"
    assert torch.equal(out[0][1], out[1][1]), "features differ"

    on_device = int((status == 0).sum())
    print(f"{len(files)} files, {sum(len(f) for f in files)} bytes: {on_device} decoded on the device, {len(files) - on_device} handed to "
          f"Pillow (status {sorted(set(status[status != 0].tolist()))}); pixels, hashes {tuple(out[0][0].shape)} and features "
          f"{tuple(out[0][1].shape)} equal those of the Pillow path bit for bit")
    return ours, status, out[0][0], out[0][1]


if __name__ == "__main__":
    main()
