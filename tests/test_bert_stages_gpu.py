"""Per-stage pins of the BERT text tower (Taiyi), through the taps of mmr_bert_forward_masked and one debug entry.

  1. embed_bert_kernel                          tap -1                          derived bound
  2. layernorm_inplace_kernel                   mmr_debug_layernorm_inplace     derived bounds; x == bf16(h) and constant rows exact
  3. each block                                 tap i-1 -> tap i                measured guard, per width
  4. gather_first_rows, pooler, classifier,
     finish_kernel                              tap layers-1 -> logits          derived bound
  5. batches cut into slices of max_batch       mask and type pointer offsets   exact

Every comparison is per element against tests/bert_stage_ref.py: the fp64 restatement of that one stage, applied to the
input the device itself tapped, never the end-to-end output.  tests/test_bert_stage_controls_host.py shows on the CPU
that each of these comparisons fails when the reference is made wrong on purpose (a shifted position row, a mask off by
one, QuickGELU for erf-GELU, ...), on the same fixtures and with the same bounds.
"""
import pytest
import torch

import bert_stage_ref as R
import mmr_amd

pytestmark = pytest.mark.gpu

# Residual stream after a block against block() of the stream tapped before it, largest error as a fraction of the largest
# |reference| entry, per width.  Measured, not derived: the attention kernel's inner roundings are its own.
# 3x the largest value over both blocks, every shape of R.SHAPES, masked and ids-only (MI355X, 2026-10-18, against the fp64
# stage reference): width 128 3.70e-4, 512 7.09e-4, 768 9.97e-4, 1024 1.151e-3.  With one token per sequence, where
# attention is the identity, the same comparison measures 2e-6 .. 4e-6 (4e-4 where one bf16 value rounds the other way):
# what is measured here is the attention kernel's bf16 probabilities, not the GEMMs or the LayerNorms.  The smallest
# control (QuickGELU for erf-GELU) stands 3.1x (widths 768, 1024) to 4.3x above these constants, the mask controls 20x and
# more (tests/test_bert_stage_controls_host.py prints every ratio).
BLOCK_GUARD = {128: 1.1e-3, 512: 2.1e-3, 768: 3.0e-3, 1024: 3.5e-3}

SHAPE = pytest.mark.parametrize("N,T", R.SHAPES, ids=[f"{n}x{t}" for n, t in R.SHAPES])
WIDTH = pytest.mark.parametrize("width", R.WIDTHS)

_ENC = {}


@pytest.fixture(scope="module")
def L(device):
    from mmr_amd import _lib
    return _lib


def _enc(width, device):
    if width not in _ENC:
        cfg, w = R.stage_weights(width)
        _ENC[width] = mmr_amd.bert.BertTextEncoder(cfg, w, device)
    return _ENC[width]


def _forward(enc, ids, mask, types, tap_after, normalize=False):
    """One call -> (tapped residual stream [N,T,d], logits), both on the CPU.  ids / mask / types go over as they are, so
    device-resident ones stay unchecked by the host."""
    N, T = ids.shape
    tap = torch.full((N * T, enc.cfg.width), float("nan"), device=enc.device)
    dev = lambda t: None if t is None else t.to(enc.device)                 # noqa: E731
    out = enc.logits(dev(ids), attention_mask=dev(mask), token_type_ids=dev(types), normalize=normalize,
                     tap_after=tap_after, tap=tap)
    torch.cuda.synchronize(enc.device)
    return tap.cpu().view(N, T, -1), out.cpu()


def _status(enc):
    return int(enc._ws[:4].view(torch.int32)[0])


# ------------------------------------------------------------------------------------------------ 1. embedding
def _check_embed(enc, w, ids, types, what, expect_ids=None, expect_types=None):
    got, _ = _forward(enc, ids, None, types, -1)
    e_ids, e_types = (ids if expect_ids is None else expect_ids), (types if expect_types is None else expect_types)
    ref = R.embed(w, enc.cfg, e_ids, e_types)
    bound = R.embed_bound(w, enc.cfg, e_ids, e_types, ref)
    assert torch.isfinite(got).all()
    excess = ((got.double() - ref).abs() / bound).max().item()
    print(f"MEASURED bert embed {what}: {excess:.3e} of the derived per-element bound, "
          f"{R.frac_of_max(got, ref):.3e} of max |ref|")
    assert excess <= 1.0, f"{what}: error is {excess:.2f}x the derived bound"


@WIDTH
@SHAPE
def test_embedding(device, width, N, T):
    """(word + type) + position -> LayerNorm, eps 1e-12: both ends of the word table, both token types inside a row,
    types absent, a row of nothing but padding, and at 160 tokens the last position row."""
    cfg, w = R.stage_weights(width)
    enc = _enc(width, device)
    ids, mask, types = R.stage_batch(N, T)
    if T > 1:
        ids[N - 1] = 0                                                      # an all-pad row (at T = 1 row 0 is one already)
    kept = ids[mask.bool()]
    assert int(kept.min()) == 0 and int(kept.max()) == cfg.vocab - 1
    assert T == 1 or ((types * mask).sum(1) > 0).any() and (((1 - types) * mask).sum(1) > 0).all()
    _check_embed(enc, w, ids, types, f"d={width} {N}x{T} types")
    _check_embed(enc, w, ids, None, f"d={width} {N}x{T} types=None")
    assert _status(enc) == 0 and not enc.id_errors()


@WIDTH
def test_embedding_clamps_and_reports_device_ids(device, width):
    """Ids and types that already live on the GPU are not read by the host: embed_bert_kernel clamps them (id < 0 -> 0,
    id >= vocab -> vocab - 1, type < 0 -> 0, type > 1 -> 1) and raises bit 0 of the status word; the next clean call
    clears it."""
    cfg, w = R.stage_weights(width)
    enc = _enc(width, device)
    V = cfg.vocab
    ids, mask, types = R.stage_batch(5, 33)
    bad_i, ok_i, bad_t, ok_t = ids.clone(), ids.clone(), types.clone(), types.clone()
    for (n, t), v, c in (((0, 2), -1, 0), ((1, 0), V, V - 1), ((4, 32), V + 9, V - 1)):
        bad_i[n, t], ok_i[n, t] = v, c
    for (n, t), v, c in (((0, 5), 2, 1), ((3, 31), -1, 0)):
        bad_t[n, t], ok_t[n, t] = v, c
    _check_embed(enc, w, ids, types, f"d={width} clean")
    assert _status(enc) == 0
    _check_embed(enc, w, bad_i, types, f"d={width} bad ids", expect_ids=ok_i)
    assert _status(enc) & 1 and enc.id_errors()
    _check_embed(enc, w, ids, bad_t, f"d={width} bad types", expect_types=ok_t)
    assert _status(enc) & 1 and enc.id_errors()
    _check_embed(enc, w, ids, types, f"d={width} clean again")
    assert _status(enc) == 0 and not enc.id_errors()
    # the clamped rows are not the unclamped neighbours': the reference of id 1 / V - 2 / the other type is far outside
    ref = R.embed(w, cfg, ok_i, ok_t)
    near_i = ok_i.clone()
    near_i[0, 2], near_i[1, 0], near_i[4, 32] = 1, V - 2, V - 2
    bound = R.embed_bound(w, cfg, ok_i, ok_t, ref)
    for (n, t) in ((0, 2), (1, 0), (4, 32)):
        assert ((R.embed(w, cfg, near_i, ok_t) - ref).abs() / bound)[n, t].max().item() > 100.0
    for (n, t) in ((0, 5), (3, 31)):
        assert ((R.embed(w, cfg, ok_i, 1 - ok_t) - ref).abs() / bound)[n, t].max().item() > 100.0


# ------------------------------------------------------------------------------------------------ 2. LayerNorm in place
CANARY = 8


def _ln_inplace(L, device, h, w, b, eps):
    """Launch on h [rows,d] followed by CANARY rows of 7.0 in both buffers -> (h_out, x_out) with the canary rows."""
    rows, d = h.shape
    hd = torch.cat([h, torch.full((CANARY, d), 7.0)]).to(device)
    xd = torch.full((rows + CANARY, d), 7.0, dtype=torch.bfloat16, device=device)
    wd, bd = w.to(device), b.to(device)
    L.check(L.lib().mmr_debug_layernorm_inplace(hd.data_ptr(), wd.data_ptr(), bd.data_ptr(), xd.data_ptr(), rows, d, eps,
                                                L.stream_ptr(device)))
    torch.cuda.synchronize(device)
    return hd.cpu(), xd.cpu()


@pytest.mark.parametrize("rows", [1, 37, 130])
@WIDTH
def test_layernorm_inplace(L, device, width, rows):
    """The only LayerNorm the BERT tower runs.  Ordinary rows; rows whose standard deviation is 1e-3, where eps = 1e-5 against
    1e-12 changes the result by a factor 3.3 (var = 1e-6), so the wrong eps cannot pass either; constant rows."""
    d = width
    g = torch.Generator().manual_seed(7 * d + rows)
    w, b = torch.randn(d, generator=g), torch.randn(d, generator=g)
    families = {"ordinary": torch.randn(rows, d, generator=g) * 3 + 0.5, "std 1e-3": torch.randn(rows, d, generator=g) * 1e-3}
    for eps in (1e-12, 1e-5):
        eps32 = torch.tensor(eps, dtype=torch.float32).item()               # the value the C call receives
        for name, h in families.items():
            h_out, x_out = _ln_inplace(L, device, h, w, b, eps)
            ref = R.ln64(h.double(), w, b, eps32)
            e_h = ((h_out[:rows].double() - ref).abs() / R.ln_h_bound(h, w, ref, d, eps32)).max().item()
            e_x = ((x_out[:rows].double() - ref).abs() / R.ln_x_bound(ref)).max().item()
            print(f"MEASURED bert layernorm_inplace d={d} rows={rows} {name} eps={eps:g}: h {e_h:.3e} of its derived bound "
                  f"({R.frac_of_max(h_out[:rows], ref):.3e} of max |ref|), x {e_x:.3e} of test_layernorm's bound")
            assert e_h <= 1.0, f"{name} eps={eps:g}: h error is {e_h:.2f}x the derived fp32 bound"
            assert e_x <= 1.0, f"{name} eps={eps:g}: x error is {e_x:.2f}x the bound"
            assert torch.equal(x_out[:rows], h_out[:rows].bfloat16()), "x is not bf16(h)"                       # exact
            assert torch.equal(h_out[rows:], torch.full((CANARY, d), 7.0)), "h stored past the last row"
            assert torch.equal(x_out[rows:].float(), torch.full((CANARY, d), 7.0)), "x stored past the last row"
            other = R.ln64(h.double(), w, b, 1e-5 if eps == 1e-12 else 1e-12)
            if name == "std 1e-3":                                          # the other eps is far outside both bounds
                assert ((other - ref).abs() / R.ln_x_bound(ref)).max().item() > 50.0
        # constant rows: with these values every partial sum of the row is exact in fp32, so mean = c, x - mean = 0 and the
        # result is beta, bit for bit, whatever eps is
        c = torch.tensor([0.5, -2.0, 1.5, 0.0, 96.0])[torch.arange(rows) % 5]
        h_out, x_out = _ln_inplace(L, device, c[:, None].expand(rows, d).contiguous(), w, b, eps)
        assert torch.equal(h_out[:rows], b.expand(rows, d)), f"constant rows, eps={eps:g}: LayerNorm is not beta"
        assert torch.equal(x_out[:rows], b.bfloat16().expand(rows, d))
        assert torch.equal(h_out[rows:], torch.full((CANARY, d), 7.0)) and torch.equal(x_out[rows:].float(), torch.full((CANARY, d), 7.0))


def test_layernorm_inplace_rejects_bad_arguments(L, device):
    h = torch.zeros(4, 192, device=device)
    x = torch.zeros(4, 192, dtype=torch.bfloat16, device=device)
    w = torch.ones(192, device=device)
    lib, st = L.lib(), L.stream_ptr(device)
    assert lib.mmr_debug_layernorm_inplace(h.data_ptr(), w.data_ptr(), w.data_ptr(), x.data_ptr(), 4, 192, 1e-12, st) == -95
    assert lib.mmr_debug_layernorm_inplace(0, w.data_ptr(), w.data_ptr(), x.data_ptr(), 4, 128, 1e-12, st) == -22
    assert lib.mmr_debug_layernorm_inplace(h.data_ptr(), w.data_ptr(), w.data_ptr(), x.data_ptr(), 0, 128, 1e-12, st) == 0


# ------------------------------------------------------------------------------------------------ 3. blocks
@pytest.mark.parametrize("masked", [True, False], ids=["masked", "ids-only"])
@WIDTH
@SHAPE
def test_each_block_from_its_tapped_input(device, width, N, T, masked):
    """Block i of the device against block() of the stream the device tapped before it (block 0: the embedding tap), in
    the tokenizer-output form (key mask and token types; sequences of length T, 1, 17, T-1, 5 side by side) and in the
    ids-only form, where the pads attend and are attended to."""
    cfg, w = R.stage_weights(width)
    enc = _enc(width, device)
    ids, mask, types = R.stage_batch(N, T)
    if not masked:
        mask = types = None
    taps = [_forward(enc, ids, mask, types, i)[0] for i in range(-1, cfg.layers)]
    assert all(torch.isfinite(t).all() for t in taps)
    for i in range(cfg.layers):
        ref = R.block(w, cfg, i, taps[i], mask)
        e = R.frac_of_max(taps[i + 1], ref)
        print(f"MEASURED bert block d={width} {N}x{T} {'masked' if masked else 'ids-only'} block {i}: {e:.3e} (of max |ref|)")
        assert e <= BLOCK_GUARD[width], f"block {i}: {e:.3e} of max |ref| is above the guard {BLOCK_GUARD[width]:.1e}"


# ------------------------------------------------------------------------------------------------ 4. tail
OUT = pytest.mark.parametrize("normalize,out_dtype", [(nz, dt) for nz in (False, True)
                                                      for dt in (torch.float32, torch.bfloat16, torch.float16)])


def _set_dtype(enc, dt):
    return {torch.float32: enc.float, torch.bfloat16: enc.bfloat16, torch.float16: enc.half}[dt]()


@WIDTH
@OUT
def test_tail_from_the_tapped_residual_stream(device, width, normalize, out_dtype):
    """First-row gather, tanh pooler, classifier and finish_kernel against tail() of the stream tapped after the last
    block, in the same call."""
    cfg, w = R.stage_weights(width)
    enc = _enc(width, device)
    try:
        _set_dtype(enc, out_dtype)
        for N, T in ((5, 33), (3, 130), (3, 1)):
            ids, mask, types = R.stage_batch(N, T)
            h_last, out = _forward(enc, ids, mask, types, cfg.layers - 1, normalize)
            assert out.dtype == out_dtype and torch.isfinite(h_last).all()
            ref = R.tail(w, cfg, h_last, normalize, out_dtype)
            excess = ((out.double() - ref).abs() / R.tail_bound(w, cfg, h_last, normalize, out_dtype)).max().item()
            print(f"MEASURED bert tail d={width} {N}x{T} normalize={normalize} {out_dtype}: {excess:.3e} of the derived bound, "
                  f"{R.frac_of_max(out, ref):.3e} of max |ref|")
            assert excess <= 1.0, f"{N}x{T}: error is {excess:.2f}x the derived bound"
    finally:
        enc.float()


@WIDTH
def test_tail_pools_the_first_row_of_every_sequence(device, width):
    """gather_first_rows is a copy of row n*T.  Every sequence here starts with the same token, so the first rows are one
    family and the other rows another; the logits must be those of T = 1 sequences made of the first rows alone, and
    must not be those of any row a wrong stride or offset would take: row n of the flat stream, the row after the
    first, the last row of the sequence."""
    cfg, w = R.stage_weights(width)
    enc = _enc(width, device)
    for N, T in ((5, 33), (2, 160)):
        ids, mask, types = R.stage_batch(N, T)
        assert (ids[:, 0] == ids[0, 0]).all()
        h_last, out = _forward(enc, ids, mask, types, cfg.layers - 1)
        first = h_last[:, :1]                                               # N sequences of one token
        ref, bound = R.tail(w, cfg, first, False, torch.float32), R.tail_bound(w, cfg, first, False, torch.float32)
        assert torch.equal(ref, R.tail(w, cfg, h_last, False, torch.float32))
        assert ((out.double() - ref).abs() / bound).max().item() <= 1.0
        flat = h_last.reshape(N * T, -1)
        n = torch.arange(N)
        for what, rows in R.wrong_pool_rows(N, T):
            wrong = R.tail(w, cfg, flat[rows][:, None], False, torch.float32)
            apart = ((wrong - ref).abs() / bound).max(dim=-1).values
            differs = rows != n * T                                         # "row n" of sequence 0 IS its first row
            assert apart[differs].min().item() > 2.0, f"{what}: only {apart[differs].min().item():.1f} bounds from the first row's"


# ------------------------------------------------------------------------------------------------ 5. slicing
def test_slices_of_a_large_batch_offset_mask_and_types(device):
    """N = 10 through max_batch = 4 runs as slices of 4, 4 and 2 sequences: the ids, the key mask and the token types of a
    slice all start at row s of their tensors.  Every sequence has its own length and type boundary, so a slice that
    read another slice's mask or types cannot give the bits of the one-call result."""
    cfg, w = R.stage_weights(128)
    whole = _enc(128, device)
    sliced = mmr_amd.bert.BertTextEncoder(cfg, w, device)
    sliced.max_batch = 4
    N, T = 10, 33
    g = torch.Generator().manual_seed(12)
    lens = torch.tensor([33, 1, 17, 32, 5, 9, 33, 2, 21, 12])
    split = torch.tensor([16, 1, 3, 30, 2, 9, 1, 1, 11, 6])
    mask = (torch.arange(T)[None, :] < lens[:, None]).int()
    types = (torch.arange(T)[None, :] >= split[:, None]).int() * mask
    ids = torch.randint(1, cfg.vocab, (N, T), generator=g, dtype=torch.int32) * mask
    dev = [t.to(device) for t in (ids, mask, types)]
    a = whole.logits(dev[0], attention_mask=dev[1], token_type_ids=dev[2])
    b = sliced.logits(dev[0], attention_mask=dev[1], token_type_ids=dev[2])
    assert torch.equal(a, b), "slices of 4 differ from the one-call result"
    assert not sliced.id_errors()
    # the one-call result is the stage reference's, so both are; and it does depend on every row's own mask and types
    h_last, out = _forward(whole, ids, mask, types, cfg.layers - 1)
    assert torch.equal(out, a.cpu())
    assert ((out.double() - R.tail(w, cfg, h_last, False, torch.float32)).abs()
            / R.tail_bound(w, cfg, h_last, False, torch.float32)).max().item() <= 1.0
    rolled = whole.logits(dev[0], attention_mask=dev[1].roll(4, 0), token_type_ids=dev[2].roll(4, 0))
    assert not torch.equal(rolled[4:8], a[4:8])
    # an out-of-range id, or type, in slice 0 is still reported after slices 1 and 2 zeroed the status word again
    bad = dev[0].clone()
    bad[1, 0] = cfg.vocab + 9
    out_bad = sliced.logits(bad, attention_mask=dev[1], token_type_ids=dev[2])
    assert sliced.id_errors()
    keep = [0, 2, 3, 4, 5, 6, 7, 8, 9]
    assert torch.equal(out_bad[keep], a[keep])
    bad_t = dev[2].clone()
    bad_t[2, 4] = 2
    sliced.logits(dev[0], attention_mask=dev[1], token_type_ids=bad_t)
    assert sliced.id_errors()
    sliced.logits(dev[0], attention_mask=dev[1], token_type_ids=dev[2])
    assert not sliced.id_errors()
