"""The reference's two clean-up tools over synthetic perceptual hashes, each printed against a brute-force check:

  same folder   tool/find_repeated_in_same_folder.py: every image carries (phash, dhash, whash); two images are duplicates
                when ANY of the three Hamming distances is <= 5; images are visited largest file first and a duplicate
                is reported against the first kept image it matches  ->  dedup.find_hash_duplicates
  cross set     tool/delete repeated.py: a train image is dropped when its dhash equals (threshold 0) a test image's
                ->  dedup.cross_set_duplicates

The hashes here are random 64-bit words with planted near copies; a real caller computes them next to the image decode
and packs the hex strings the reference prints with dedup.hashes_from_hex.

    python examples/hash_dedup_synthetic.py [--rows 3000] [--copies 200]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmr_amd import dedup  # noqa: E402


def _hex(v):
    return f"{int(v):016x}"


def _near_copy(rng, row, max_bits):
    out = row.copy()
    for k in range(row.size):
        for b in rng.choice(64, size=rng.integers(0, max_bits + 1), replace=False):
            out[k] ^= np.uint64(1) << np.uint64(b)
    return out


def _distances(rows, row):
    """Hamming distances [k, H] of uint64 rows [k, H] to one row [H]"""
    x = np.ascontiguousarray(rows ^ row[None])
    return np.unpackbits(x.view(np.uint8), axis=1).reshape(x.shape[0], x.shape[1], 64).sum(-1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=3000)
    ap.add_argument("--copies", type=int, default=200)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    n = args.rows

    # ---- same folder: (phash, dhash, whash) per image, near copies planted, file sizes for the visit order
    words = rng.integers(0, 2 ** 64, size=(n, 3), dtype=np.uint64)
    rows = rng.permutation(n)
    for p in range(args.copies):
        words[rows[2 * p + 1]] = _near_copy(rng, words[rows[2 * p]], 7)          # some within 5 bits, some not
    keys = [f"img_{r:05d}.jpg" for r in range(n)]
    sizes = rng.integers(10_000, 5_000_000, size=n)
    hashes = dedup.hashes_from_hex([tuple(_hex(v) for v in row) for row in words]).to(dev)
    order = np.argsort(-sizes, kind="stable")
    found = dedup.find_hash_duplicates(keys, hashes, 5, order=order)

    kept, brute = [], []                                                          # the reference's loop, on the host
    for r in order.tolist():
        hits = np.flatnonzero(_distances(words[kept], words[r]).min(axis=1) <= 5) if kept else []
        if len(hits) == 0:
            kept.append(r)
        else:
            brute.append((keys[r], keys[kept[hits[0]]]))
    same = found == brute
    print(f"same folder: {n} images, {args.copies} planted near copies -> {len(found)} duplicates reported; "
          f"brute-force loop {'equal' if same else 'DIFFERENT'}")
    for dup, of in found[:3]:
        print(f"    {dup} duplicates {of}")

    # ---- cross set: dhash only, threshold 0; test images planted into the train set (some twice, some one bit off)
    m = max(n // 10, 10)
    test = rng.integers(0, 2 ** 64, size=(m, 1), dtype=np.uint64)
    train = rng.integers(0, 2 ** 64, size=(n, 1), dtype=np.uint64)
    spots = rng.permutation(n)[:m]
    for t, r in enumerate(spots.tolist()):
        train[r] = test[t] if t % 3 else _near_copy(rng, test[t], 1)
    test[1] = test[0]                                                             # equal test hashes: the lowest row is reported
    train[spots[1]] = test[0]
    train_h = dedup.hashes_from_hex([(_hex(v[0]),) for v in train]).to(dev)
    test_h = dedup.hashes_from_hex([(_hex(v[0]),) for v in test]).to(dev)
    is_dup, match = dedup.cross_set_duplicates(train_h, test_h, 0)

    first = {}
    for t in range(m - 1, -1, -1):
        first[int(test[t, 0])] = t
    brute_match = np.array([first.get(int(v[0]), -1) for v in train])
    same_cross = np.array_equal(match.cpu().numpy(), brute_match) and np.array_equal(is_dup.cpu().numpy(), brute_match >= 0)
    print(f"cross set: {n} train x {m} test dhashes, threshold 0 -> {int(is_dup.sum())} train images to drop; "
          f"brute-force lookup {'equal' if same_cross else 'DIFFERENT'}")
    return same and same_cross


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
