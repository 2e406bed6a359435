"""The flow of the reference's `run_tip_adapter_F` (code/main_custom.py:148-247) on synthetic features: build the cache from
the shots, score the held-out set with the fixed cache (Tip-Adapter), make the cache keys learnable and train them with
AdamW(eps=1e-4) under a cosine schedule for 20 epochs (Tip-Adapter-F), score again with the trained keys.

The encoder is frozen in the reference, so training sees only its output features; here they are synthetic: each class a
unit prototype, a feature `normalize(proto[y] + 3 randn / sqrt(E))` rounded to bf16, a classifier row
`normalize(proto + 1.5 randn / sqrt(E))`.  Every step is two kernel launches; nothing is read back until the end.

    python examples/tip_adapter_f_synthetic.py [--seed 0] [--dim 128]
"""
import argparse
import math
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd as clip  # noqa: E402

CLASSES, SHOTS, TRAIN_ROWS, BATCH, EPOCHS, TEST_ROWS = 6, 16, 256, 64, 20, 2048
LR, ALPHA, BETA = 1e-3, 1.0, 5.5


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dim", type=int, default=128)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    E = args.dim
    g = torch.Generator().manual_seed(args.seed)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)
    proto = unit(torch.randn(CLASSES, E, generator=g))

    def draw(labels):
        return unit(proto[labels] + 3.0 * torch.randn(len(labels), E, generator=g) / math.sqrt(E)).bfloat16()

    clip_weights = unit(proto + 1.5 * torch.randn(CLASSES, E, generator=g) / math.sqrt(E)).bfloat16().t().contiguous()    # [E,C]
    shot_labels = torch.arange(CLASSES).repeat_interleave(SHOTS)
    cache_keys = draw(shot_labels).t().contiguous()                                    # [E,S], S = 6 * 16
    cache_values = torch.nn.functional.one_hot(shot_labels, CLASSES).float()           # [S,C]
    train_y = torch.randint(0, CLASSES, (TRAIN_ROWS,), generator=g)
    train_f = draw(train_y)
    test_y = torch.randint(0, CLASSES, (TEST_ROWS,), generator=g)
    test_f = draw(test_y).to(dev)

    per_epoch = (TRAIN_ROWS + BATCH - 1) // BATCH
    t = clip.TipAdapterF(cache_keys.to(dev), cache_values.to(dev), clip_weights.to(dev), ALPHA, BETA, lr=LR,
                         total_steps=EPOCHS * per_epoch)                               # the reference's AdamW: eps 1e-4, wd 0.01

    def accuracy():
        return float((t.logits(test_f).argmax(dim=1).cpu() == test_y).float().mean())

    acc_before = accuracy()                                                            # Tip-Adapter: the cache as built
    losses = t.fit(train_f.to(dev), train_y.to(dev), BATCH, EPOCHS, generator=torch.Generator().manual_seed(args.seed + 1))
    t.check()                                                                          # the one read of the status word
    epoch_losses = losses.view(EPOCHS, per_epoch).mean(dim=1).cpu().tolist()
    acc_after = accuracy()                                                             # Tip-Adapter-F: the trained keys

    with tempfile.TemporaryDirectory() as cache_dir:                                   # main_custom.py:212,214
        t.save(cache_dir, SHOTS)
        again = clip.TipAdapterF.load_weight(cache_dir, SHOTS, device=dev)
        assert torch.equal(again, t.weight)
    print(f"{CLASSES} classes x {SHOTS} shots, E = {E}: {EPOCHS} epochs of {per_epoch} steps ({TRAIN_ROWS} rows, batches of {BATCH})")
    for e in (0, EPOCHS // 2, EPOCHS - 1):
        print(f"epoch {e:2d}: mean loss {epoch_losses[e]:.4f}")
    print(f"held-out accuracy over {TEST_ROWS} rows: Tip-Adapter {acc_before:.4f} -> Tip-Adapter-F {acc_after:.4f}")
    return epoch_losses, acc_before, acc_after


if __name__ == "__main__":
    main()
