"""tool/find_repeated_in_same_folder.py from decoded pixels to the duplicate list, all on the GPU:

    pixels -> dedup.image_hashes (phash, dhash, whash; Pillow's LANCZOS bytes)  ->  dedup.hash_duplicate_pairs (any Hamming
    distance <= 5)  ->  dedup.keep_first (largest file first)          = dedup.find_image_duplicates

The images are synthetic: smooth random structure plus texture, with planted copies of three kinds -- re-noised (a
re-encode), rescaled by 0.9 (a thumbnail) and brightness-shifted.  The planted pairs and what was found are printed side
by side; a planted copy is not guaranteed to be found (the rule is imagehash's, not this example's), the originals of
different images must not be confused.

    python examples/image_hash_dedup_synthetic.py [--images 60] [--copies 18] [--hash-size 8]
"""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmr_amd import dedup  # noqa: E402


def _structure(rng, h, w):
    low = Image.fromarray(rng.integers(0, 256, (h // 24 + 2, w // 24 + 2, 3), dtype=np.uint8), "RGB")
    return np.asarray(low.resize((w, h), Image.BICUBIC)).astype(np.int16)


def _noisy(rng, base, amp):
    return np.clip(base + rng.integers(-amp, amp + 1, base.shape), 0, 255).astype(np.uint8)


def planted_set(images=60, copies=18, seed=0):
    """-> (keys, [uint8 RGB arrays], file sizes, [(copy key, original key, kind)]): ``images`` originals of a few sizes and
    ``copies`` planted copies of some of them, shuffled"""
    rng = np.random.default_rng(seed)
    shapes = [(120, 160), (160, 120), (144, 144), (97, 131), (200, 300)]
    items = []
    for r in range(images):
        h, w = shapes[r % len(shapes)]
        items.append((f"img_{r:04d}.jpg", _noisy(rng, _structure(rng, h, w), 6)))
    planted = []
    for c in range(copies):
        key, img = items[int(rng.integers(0, images))]
        kind = ("renoised", "rescaled", "brighter")[c % 3]
        if kind == "renoised":
            copy = _noisy(rng, img.astype(np.int16), 4)
        elif kind == "rescaled":
            h, w = img.shape[:2]
            copy = np.asarray(Image.fromarray(img, "RGB").resize((int(w * 0.9), int(h * 0.9)), Image.BICUBIC))
        else:
            copy = np.clip(img.astype(np.int16) + 12, 0, 255).astype(np.uint8)
        items.append((f"copy_{c:03d}_{kind}.jpg", copy))
        planted.append((items[-1][0], key, kind))
    order = rng.permutation(len(items))
    items = [items[i] for i in order]
    keys = [k for k, _ in items]
    arrays = [np.ascontiguousarray(a) for _, a in items]
    sizes = np.array([a.size + (0 if k.startswith("img") else -1) for k, a in items])     # an original outweighs its equal-sized copy
    return keys, arrays, sizes, planted


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=60)
    ap.add_argument("--copies", type=int, default=18)
    ap.add_argument("--hash-size", type=int, default=8)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    keys, arrays, sizes, planted = planted_set(args.images, args.copies)
    imgs = [torch.from_numpy(np.array(a)).to(dev) for a in arrays]

    hashes, status = dedup.image_hashes(imgs, hash_size=args.hash_size, return_status=True)
    i, j, dist = dedup.hash_duplicate_pairs(hashes, 5)
    order = np.argsort(-sizes, kind="stable")                       # the reference visits the largest file first
    keep, dup = dedup.keep_first(len(keys), i, j, order)
    found = [(keys[r], keys[int(dup[r])]) for r in order.tolist() if not keep[r]]
    assert found == dedup.find_image_duplicates(keys, imgs, 5, order=order, hash_size=args.hash_size)

    hexes = dedup.hashes_to_hex(hashes, args.hash_size)
    print(f"{len(keys)} images ({args.images} originals, {args.copies} planted copies), hash_size {args.hash_size}: "
          f"{int(i.numel())} similar pairs, {len(found)} duplicates, {int((status != 0).sum())} images with a status flag")
    print(f"    {keys[0]}: phash {hexes[0][0]} dhash {hexes[0][1]} whash {hexes[0][2]}")
    found_map = dict(found)
    hit = 0
    for copy, original, kind in planted:
        got = found_map.get(copy)
        hit += got == original
        print(f"    planted {copy} of {original}: " + (f"found, duplicates {got}" if got else "not found"))
    wrong = [(d, k) for d, k in found if d.startswith("img") or (d, k) not in {(c, o) for c, o, _ in planted}]
    print(f"planted copies found: {hit} of {len(planted)}; reports that are not a planted pair: {len(wrong)}")
    for d, k in wrong[:5]:
        print(f"    {d} duplicates {k}")
    return True


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
