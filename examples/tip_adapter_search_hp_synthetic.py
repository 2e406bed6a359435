"""The end of the reference's `run_tip_adapter` / `run_tip_adapter_F` (code/main_custom.py:132,234) on synthetic features:
build a few-shot cache, optionally train its keys for two epochs (Tip-Adapter-F), then run `search_hp` -- the (beta, alpha)
grid of code/utils.py:159-206, every point scored by the best threshold F1 of each class but the last -- in one device call
of three launches, and print the chosen pair with its per-class F1.

Features are synthetic as in tip_adapter_f_synthetic.py: each class a unit prototype, a feature
`normalize(proto[y] + 3 randn / sqrt(E))` rounded to bf16.

    python examples/tip_adapter_search_hp_synthetic.py [--seed 0] [--dim 128] [--train]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmr_amd as clip  # noqa: E402

CLASSES, SHOTS, TRAIN_ROWS, BATCH, EPOCHS, TEST_ROWS = 6, 16, 256, 64, 2, 1024
CFG = dict(search_hp=True, search_scale=[7, 3], search_step=[10, 6], init_beta=5.5, init_alpha=1.0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--train", action="store_true", help="two epochs of TipAdapterF.fit before the search")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    E = args.dim
    g = torch.Generator().manual_seed(args.seed)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)
    proto = unit(torch.randn(CLASSES, E, generator=g))

    def draw(labels):
        return unit(proto[labels] + 3.0 * torch.randn(len(labels), E, generator=g) / math.sqrt(E)).bfloat16()

    clip_weights = unit(proto + 1.5 * torch.randn(CLASSES, E, generator=g) / math.sqrt(E)).bfloat16().t().contiguous().to(dev)
    shot_labels = torch.arange(CLASSES).repeat_interleave(SHOTS)
    cache_keys = draw(shot_labels).t().contiguous().to(dev)                            # [E,S]
    cache_values = torch.nn.functional.one_hot(shot_labels, CLASSES).float().to(dev)   # [S,C]
    train_y = torch.randint(0, CLASSES, (TRAIN_ROWS,), generator=g)
    train_f = draw(train_y)
    test_y = torch.randint(0, CLASSES, (TEST_ROWS,), generator=g).to(dev)
    test_f = draw(test_y.cpu()).to(dev)

    adapter = None
    if args.train:
        per_epoch = (TRAIN_ROWS + BATCH - 1) // BATCH
        adapter = clip.TipAdapterF(cache_keys, cache_values, clip_weights, CFG["init_alpha"], CFG["init_beta"], lr=1e-3,
                                   total_steps=EPOCHS * per_epoch)
        adapter.fit(train_f.to(dev), train_y.to(dev), BATCH, EPOCHS, generator=torch.Generator().manual_seed(args.seed + 1))
        adapter.check()

    beta, alpha = clip.search_hp(CFG, cache_keys, cache_values, test_f, test_y, clip_weights, adapter=adapter)
    # the same grid once more, kept, to show what the search saw at its pick
    betas, alphas = clip.tip_adapter.search_lists(CFG)
    grid = clip.tip_adapter_grid(test_f, test_y, clip_weights, cache_keys, cache_values, betas, alphas, adapter=adapter)
    b, a, score = grid.best(classes=range(CLASSES - 1))
    assert (beta, alpha) == (betas[b], alphas[a])
    per_class = grid.f1[b, a].cpu().tolist()
    print(f"{CLASSES} classes x {SHOTS} shots, E = {E}, {TEST_ROWS} rows, grid {len(betas)} x {len(alphas)}"
          f"{', keys trained for 2 epochs' if args.train else ''}")
    print(f"best beta {beta:.4f}, alpha {alpha:.4f}: mean threshold F1 of classes 0..{CLASSES - 2} = {score:.4f}")
    for c, f1 in enumerate(per_class):
        print(f"  class {c}: F1 {f1:.4f} at threshold {float(grid.threshold[b, a, c]):.3f} "
              f"(tp {int(grid.tp[b, a, c])}, fp {int(grid.fp[b, a, c])}, fn {int(grid.fn[b, a, c])})")
    print(f"macro-F1 {float(grid.macro_f1()[b, a]):.2f}, accuracy without the last class "
          f"{float(grid.accuracy(exclude_class=CLASSES - 1)[b, a]):.2f}")
    return beta, alpha, score, per_class


if __name__ == "__main__":
    main()
