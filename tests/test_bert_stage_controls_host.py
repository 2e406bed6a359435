"""Failing controls for tests/test_bert_stages_gpu.py, without a device: every comparison that file makes between the
device and tests/bert_stage_ref.py is made here between the reference and a copy of it with one mistake planted
(``mut=``), on the same fixtures and with the same bound.  Each must FAIL; that is what shows the pins would notice a
subtly wrong kernel.  The last test shows why the pins exist: three of the mistakes, pushed through the whole tower, stay
inside the 1 - 1e-4 cosine guard that was all tests/test_bert_gpu.py had.
"""
import pytest
import torch

import bert_stage_ref as R
from test_bert_gpu import _cos, _ids
from test_bert_stages_gpu import BLOCK_GUARD

SHAPE = pytest.mark.parametrize("N,T", R.SHAPES, ids=[f"{n}x{t}" for n, t in R.SHAPES])
WIDTH = pytest.mark.parametrize("width", R.WIDTHS)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name", ["tiny-bert-test", "stage-128", "stage-1024"])
def test_stages_compose_to_the_oracle(name):
    """embed -> block x layers -> tail with no mutation and no rounding point is oracle/bert_ref.py's forward, which
    runs in fp32: the two agree to fp32 rounding (2e-5 of the largest entry, the figure DESIGN section 2 gives for the
    fp32 oracle against HF), at every stage the oracle records and in both call forms."""
    from mmr_amd import weights
    from mmr_amd.config import get_bert_config
    from oracle import bert_ref
    if name == "tiny-bert-test":
        cfg = get_bert_config(name)
        w = weights.make_bert_weights(cfg)
        ids = _ids(cfg, 5, 33)
        mask = (ids != 0).int()
        types = (torch.arange(33)[None, :] >= 16).int() * mask
    else:
        cfg, w = R.stage_weights(int(name.split("-")[1]))
        ids, mask, types = R.stage_batch(5, 33)
    for m, t in ((None, None), (mask, types)):
        st = {}
        with torch.no_grad():
            want = bert_ref.bert_logits(w, cfg, ids, stages=st, attention_mask=None if m is None else m.long(),
                                        token_type_ids=None if t is None else t.long())
        h = R.embed(w, cfg, ids, t, rounding=False)
        pairs = [("embed", h, st["embed"])]
        for i in range(cfg.layers):
            h = R.block(w, cfg, i, h, m, rounding=False)
            pairs.append((f"layer{i}", h, st[f"layer{i}"]))
        pairs.append(("logits", R.tail(w, cfg, h, False, torch.float32, rounding=False), want))
        assert torch.equal(pairs[-1][1], R.logits(w, cfg, ids, m, t))
        for what, got, ref in pairs:
            e = R.frac_of_max(got, ref)
            print(f"{name} {'ids-only' if m is None else 'masked'} {what}: {e:.2e} of max |oracle|")
            assert e <= 2e-5, (what, e)


def test_unknown_mutation_is_refused():
    cfg, w = R.stage_weights(128)
    ids, mask, types = R.stage_batch(3, 1)
    with pytest.raises(ValueError):
        R.embed(w, cfg, ids, types, mut="typo")
    assert set(R.EMBED_MUTATIONS + R.BLOCK_MUTATIONS + R.TAIL_MUTATIONS) == set(R.MUTATIONS)


# ------------------------------------------------------------------------------------------------ controls
@WIDTH
@SHAPE
def test_every_control_fails_the_pin_of_its_stage(width, N, T):
    cfg, w = R.stage_weights(width)
    ids, mask, types = R.stage_batch(N, T)
    what = f"d={width} {N}x{T}"

    # 1. embedding: derived bound.  One token per sequence has no position 1 and no second token type
    h = R.embed(w, cfg, ids, types)
    bound = R.embed_bound(w, cfg, ids, types, h)
    for mut in R.EMBED_MUTATIONS:
        if T == 1 and mut in ("pos_shift", "types_ignored"):
            continue
        excess = ((R.embed(w, cfg, ids, types, mut) - h).abs() / bound).max().item()
        print(f"CONTROL {what} embed {mut}: {excess:.3g}x the derived bound")
        assert excess > 10.0, (mut, excess)

    # 3. blocks: the measured guard, in the masked form (one token per sequence has nothing to mask)
    for i in range(cfg.layers):
        ref = R.block(w, cfg, i, h, mask)
        floor = R.frac_of_max(R.block(w, cfg, i, h, mask, rounding=False), ref)
        for mut in R.BLOCK_MUTATIONS:
            if T == 1 and mut in ("mask_off_by_one", "mask_ignored"):
                continue
            e = R.frac_of_max(R.block(w, cfg, i, h, mask, mut), ref)
            print(f"CONTROL {what} block {i} {mut}: {e:.3e} of max |ref| = {e / BLOCK_GUARD[width]:.1f}x the guard, "
                  f"{e / floor:.1f}x the rounding points' own {floor:.2e}")
            assert e > BLOCK_GUARD[width], (mut, e)
            assert e > 3 * floor, (mut, e, floor)
        h = ref

    # 4. tail: derived bound, every output form
    for normalize in (False, True):
        for dt in DTYPES:
            ref, bound = R.tail(w, cfg, h, normalize, dt), R.tail_bound(w, cfg, h, normalize, dt)
            for mut in R.TAIL_MUTATIONS:
                if T == 1 and mut == "pool_token1":
                    continue
                excess = ((R.tail(w, cfg, h, normalize, dt, mut) - ref).abs() / bound).max().item()
                if dt == torch.float32:
                    print(f"CONTROL {what} tail normalize={normalize} {mut}: {excess:.3g}x the derived bound")
                assert excess > 1.5, (mut, normalize, dt, excess)
    if T > 1:                                                               # the rows a wrong gather would take
        first = h[:, :1]
        ref, bound = R.tail(w, cfg, first, False, torch.float32), R.tail_bound(w, cfg, first, False, torch.float32)
        flat = h.reshape(N * T, -1)
        for name, rows in R.wrong_pool_rows(N, T):
            apart = ((R.tail(w, cfg, flat[rows][:, None], False, torch.float32) - ref).abs() / bound).max(dim=-1).values
            apart = apart[rows != torch.arange(N) * T]
            print(f"CONTROL {what} tail pooled from {name}: {apart.min().item():.3g}x the derived bound")
            assert apart.min().item() > 2.0, (name, apart)


@WIDTH
def test_wrong_eps_fails_the_layernorm_pins(width):
    """On rows whose standard deviation is 1e-3 (var = 1e-6) eps = 1e-5 instead of 1e-12, or the reverse, moves
    LayerNorm's result by a factor 3.3, far outside both bounds test_layernorm_inplace uses."""
    d = width
    g = torch.Generator().manual_seed(d)
    w, b = torch.randn(d, generator=g), torch.randn(d, generator=g)
    h = torch.randn(37, d, generator=g) * 1e-3
    for eps, wrong in ((1e-12, 1e-5), (1e-5, 1e-12)):
        ref, bad = R.ln64(h.double(), w, b, eps), R.ln64(h.double(), w, b, wrong)
        e_h = ((bad - ref).abs() / R.ln_h_bound(h, w, ref, d, eps)).max().item()
        e_x = ((bad.float().bfloat16().double() - ref).abs() / R.ln_x_bound(ref)).max().item()
        print(f"CONTROL layernorm d={d} eps {wrong:g} for {eps:g}: h {e_h:.3g}x, x {e_x:.3g}x the bound")
        assert e_h > 1e3 and e_x > 50.0
    # and the bounds are not vacuous on the rows they are used on: a relative 1e-5 for h, 2^-7 for x at the largest
    for h in (torch.randn(37, d, generator=g) * 3 + 0.5, h):
        ref = R.ln64(h.double(), w, b, 1e-12)
        assert (R.ln_h_bound(h, w, ref, d, 1e-12) / ref.abs().max()).max().item() < 1e-5
        assert (R.ln_x_bound(ref) / ref.abs().max()).max().item() < 2.0 ** -7


# ------------------------------------------------------------------------------------------------ what the old guard saw
def test_the_cosine_guard_does_not_see_three_of_them():
    """tests/test_bert_gpu.py held the tower by cos(logits) >= 1 - 1e-4 and one tap after block 0.  On its own fixture
    (tiny-bert-test, stock weights, padded ids, token types 1 on the second half) a mask that is off by one, eps = 1e-5
    and QuickGELU all stay inside that cosine; the stage pins above catch each of them."""
    from mmr_amd import weights
    from mmr_amd.config import get_bert_config
    cfg = get_bert_config("tiny-bert-test")
    w = weights.make_bert_weights(cfg)
    ids = _ids(cfg, 4, 64)
    mask = (ids != 0).int()
    types = (torch.arange(64)[None, :] >= 32).int() * mask
    ref = R.logits(w, cfg, ids, mask, types)
    for mut in ("mask_off_by_one", "eps_1e-5", "quickgelu"):
        gap = 1 - _cos(R.logits(w, cfg, ids, mask, types, mut=mut), ref).min().item()
        print(f"tiny-bert-test end to end, {mut}: 1 - cos = {gap:.2e}")
        assert 0 < gap < 1e-4, (mut, gap)
    # a mistake the cosine does see, so that the lines above are not a blunt instrument's silence
    assert 1 - _cos(R.logits(w, cfg, ids, mask, types, mut="pool_bias_dropped"), ref).min().item() > 1e-4
