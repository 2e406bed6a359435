"""The reference's format converter (tool/Image format conversion.py:41-62) with the pixels on the GPU:

    synthetic RGBA / RGB / greyscale images (what Image.open hands over for png, bmp, gif, tiff, webp sources)
        -> encode_jpeg (RGBA pasted over white while it is loaded; colour, downsampling, DCT and quantisation in two
           kernels, the Huffman coder on host threads), quality 95 as the tool writes
        -> the files Pillow writes from the same pixels, asserted equal byte for byte
        -> decode_jpeg of our files against Pillow's decode of Pillow's files, asserted equal bit for bit

and the same batch once more through ``encode_jpeg_batches`` and ``save_jpeg``.

    python examples/jpeg_encode_synthetic.py [--images 12] [--seed 0] [--out DIR]
"""
import argparse
import io
import os
import sys
import tempfile

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmr_amd import jpeg  # noqa: E402


def synthetic_images(n, seed=0):
    """n uint8 arrays of a few sizes: smooth structure plus a little texture; every third RGBA, every seventh greyscale"""
    rng = np.random.default_rng(seed)
    shapes = [(120, 160), (160, 120), (97, 131), (144, 144), (75, 200)]
    out = []
    for r in range(n):
        h, w = shapes[r % len(shapes)]
        ch = 1 if r % 7 == 6 else (4 if r % 3 == 1 else 3)
        low = Image.fromarray(rng.integers(0, 256, (h // 16 + 2, w // 16 + 2, 4), dtype=np.uint8))
        px = np.asarray(low.resize((w, h), Image.BICUBIC)).astype(np.int16) + rng.integers(-5, 6, (h, w, 4))
        px = np.clip(px, 0, 255).astype(np.uint8)
        out.append(np.ascontiguousarray(px[:, :, 0] if ch == 1 else px[:, :, :ch]))
    return out


def pillow_convert(px, quality=95):
    """what the tool does with one opened image: RGBA over white, everything else to RGB (greyscale stays 'L' here), then save"""
    im = Image.fromarray(px)
    if im.mode == "RGBA":
        background = Image.new("RGB", im.size, (255, 255, 255))
        background.paste(im, mask=im.split()[3])
        im = background
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=12)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    pixels = synthetic_images(args.images, args.seed)
    on_gpu = [torch.from_numpy(p).to(dev) for p in pixels]

    ours = jpeg.encode_jpeg(on_gpu, quality=95)                  # Pillow's default subsampling at quality 95 is 4:2:0, ours too
    theirs = [pillow_convert(p) for p in pixels]
    same = [a == b for a, b in zip(ours, theirs)]
    assert all(same), f"files differ from Pillow's: {[i for i, s in enumerate(same) if not s]}"

    decoded = jpeg.decode_jpeg(ours, device=dev, on_unsupported="raise")
    for d, f in zip(decoded, theirs):
        with Image.open(io.BytesIO(f)) as im:
            assert torch.equal(d.cpu(), torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8))), "decoded pixels differ from Pillow's"

    half = (len(on_gpu) + 1) // 2
    batched = [f for files in jpeg.encode_jpeg_batches([on_gpu[:half], on_gpu[half:]] if len(on_gpu) > 1 else [on_gpu], quality=95) for f in files]
    assert batched == ours, "encode_jpeg_batches differs from encode_jpeg"

    with tempfile.TemporaryDirectory() as tmp:
        folder = args.out or tmp
        os.makedirs(folder, exist_ok=True)
        paths = [os.path.join(folder, f"image_{i:03d}.jpg") for i in range(len(on_gpu))]
        sizes = jpeg.save_jpeg(on_gpu, paths, quality=95)
        for p, f in zip(paths, ours):
            with open(p, "rb") as fh:
                assert fh.read() == f

    kinds = {1: "greyscale", 3: "RGB", 4: "RGBA"}
    count = {k: sum(1 for p in pixels if (1 if p.ndim == 2 else p.shape[2]) == c) for c, k in kinds.items()}
    print(f"{len(ours)} images ({count}), {sum(p.size for p in pixels)} pixel bytes -> {sum(sizes)} file bytes: every file equals Pillow's byte for "
          f"byte, and decodes on the GPU to Pillow's pixels")
    return ours, theirs, decoded


if __name__ == "__main__":
    main()
