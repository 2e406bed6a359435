"""The augmented half of the reference's Tip-Adapter-F flow on synthetic images: `build_cache_model` (code/utils.py:99-132)
encodes the few-shot set `augment_epoch` times under RandomResizedCrop + RandomHorizontalFlip (code/custom.py:24-29) and
averages; `run_tip_adapter_F` (code/main_custom.py:160-170) re-encodes the freshly augmented set every epoch and takes
AdamW steps on the cache keys.  Here the decoded uint8 images stay on the GPU: the boxes are drawn on the host, the crops
are cut, resized (Pillow's bicubic, bit for bit), flipped and normalised on the device, encoded, and fed to TipAdapterF.

    python examples/tip_adapter_augment_synthetic.py [--seed 0] [--model tiny-test]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd as clip  # noqa: E402

CLASSES, SHOTS, AUGMENT_EPOCH, TRAIN_EPOCHS, BATCH = 3, 4, 3, 4, 8
LR, ALPHA, BETA = 1e-3, 1.0, 5.5


def synthetic_images(seed):
    """CLASSES x SHOTS decoded images of different sizes: each class a colour gradient of its own, plus noise."""
    rng = np.random.default_rng(seed)
    images, targets = [], []
    for c in range(CLASSES):
        for _ in range(SHOTS):
            h, w = int(rng.integers(80, 200)), int(rng.integers(80, 260))
            yy, xx = np.mgrid[0:h, 0:w]
            ramp = [xx * 255 // (w - 1), yy * 255 // (h - 1), (xx + yy) * 255 // (h + w - 2)]
            img = np.stack([ramp[(c + k) % 3] for k in range(3)], axis=2) + rng.integers(-40, 41, size=(h, w, 3))
            images.append(torch.from_numpy(np.clip(img, 0, 255).astype(np.uint8)))
            targets.append(c)
    return images, torch.tensor(targets)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--model", default="tiny-test")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    model, _ = clip.load(args.model, device=dev)
    images, targets = synthetic_images(args.seed)
    images = [im.to(dev) for im in images]
    g = torch.Generator().manual_seed(args.seed)

    keys, values = clip.build_cache_model_augmented(model, images, targets, AUGMENT_EPOCH, CLASSES, generator=g, batch_size=BATCH)
    # a stand-in for the text classifier: the mean key of each class, normalised
    E = keys.shape[0]
    clip_weights = clip.l2_normalize((keys @ values).t().contiguous()).t().contiguous().bfloat16()      # [E,C]
    per_epoch = (len(images) + BATCH - 1) // BATCH
    t = clip.TipAdapterF(keys, values, clip_weights, ALPHA, BETA, lr=LR, total_steps=TRAIN_EPOCHS * per_epoch)
    losses = []
    for _ in range(TRAIN_EPOCHS):                                    # main_custom.py:166-170: fresh crops every epoch
        feats, labels = clip.augmented_features(model, images, targets, g, batch_size=BATCH)
        for s in range(0, len(images), BATCH):
            losses.append(t.step(feats[s:s + BATCH], labels[s:s + BATCH]))
    t.check()
    losses = torch.stack(losses).cpu().tolist()
    print(f"{CLASSES} classes x {SHOTS} shots, E = {E}: cache from {AUGMENT_EPOCH} augmented passes, "
          f"{TRAIN_EPOCHS} epochs of {per_epoch} steps on fresh crops")
    print("losses: " + " ".join(f"{v:.4f}" for v in losses))
    return keys, values, losses


if __name__ == "__main__":
    main()
