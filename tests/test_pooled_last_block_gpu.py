"""GPU: the pooled-row form of the last transformer block (mmr_tower_forward) against the full block.

The forward returns one row per input, so from 2 048 padded token rows on the last block computes Q, the attention
output, out-proj, LN2 and the MLP for the pooled row of each input alone.  Every kernel involved is row-independent with
a fixed K order, so the bar is torch.equal against the same tower with mmr_tower_set_full_last_block(1), which runs the
launch sequence of the full block."""
import pytest
import torch

import mmr_amd
from mmr_amd import synth

pytestmark = pytest.mark.gpu


def _full(model, on):
    for t in (model.visual, model.text):
        t.set_full_last_block(on)


def _ab(model, fn):
    """fn() with the pooled path, then with the full last block forced; the switch is left off."""
    pooled = fn()
    _full(model, True)
    try:
        full = fn()
    finally:
        _full(model, False)
    torch.cuda.synchronize()
    return pooled, full


def _eot_ids(n, T, V, seed):
    """clip.tokenize-shaped ids whose first four rows pin the pooled position: EOT at 0, at T-1, in the middle, and a
    duplicated maximum (positions 10 and 30: the first one is the pooled row)."""
    ids = synth.synth_token_ids(n, T, V, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    ids[:4] = torch.randint(1, V - 2, (4, T), generator=g, dtype=torch.int32)
    ids[0, 0] = V - 1
    ids[1, T - 1] = V - 1
    ids[2, T // 2] = V - 1
    ids[3, 10] = V - 1
    ids[3, 30] = V - 1
    return ids


@pytest.mark.parametrize("out_dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("normalize", [True, False])
def test_tiny_towers_pooled_equals_full(device, out_dtype, normalize):
    model, _ = mmr_amd.load("tiny-test", device=device)
    model.bfloat16() if out_dtype == "bf16" else model.float()
    S, T, V = model.input_resolution, model.cfg.text.tokens, model.cfg.text.vocab
    px = synth.synth_images(131, S, seed=3).to(device)                  # 131 x 17 rows: past the gate, ragged padding
    a, b = _ab(model, lambda: model.encode_image(px, normalize=normalize))
    assert a.dtype == (torch.bfloat16 if out_dtype == "bf16" else torch.float32)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    ids = _eot_ids(37, T, V, seed=4).to(device)                          # 37 x 77 rows
    a, b = _ab(model, lambda: model.encode_text(ids, normalize=normalize))
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)


@pytest.mark.parametrize("out_dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("normalize", [True, False])
def test_vitb32_image_batch_256_pooled_equals_full(device, out_dtype, normalize):
    model, _ = mmr_amd.load("ViT-B/32", device=device, weights="synthetic")
    model.bfloat16() if out_dtype == "bf16" else model.float()
    px = synth.synth_images(256, 224, seed=2).bfloat16().to(device)
    a, b = _ab(model, lambda: model.encode_image(px, normalize=normalize))
    assert a.shape == (256, 512) and torch.isfinite(a.float()).all() and torch.equal(a, b)


def test_vitb32_text_batch_256_eot_positions(device):
    """EOT at position 0, at T-1, in the middle, and a duplicated maximum id.  Causal attention makes the first
    occurrence checkable on its own: the row at position 10 sees keys 0..10 only, so replacing the SECOND maximum
    (position 30) by an ordinary id must leave that input's features unchanged."""
    model, _ = mmr_amd.load("ViT-B/32", device=device, weights="synthetic")
    T, V = model.cfg.text.tokens, model.cfg.text.vocab
    ids = _eot_ids(256, T, V, seed=6).to(device)
    for normalize in (True, False):
        a, b = _ab(model, lambda: model.encode_text(ids, normalize=normalize))
        assert torch.isfinite(a).all() and torch.equal(a, b)
    single = ids.clone()
    single[3, 30] = 5
    a, _ = _ab(model, lambda: model.encode_text(ids, normalize=True))
    c, d = _ab(model, lambda: model.encode_text(single, normalize=True))
    assert torch.equal(a[3], c[3]) and torch.equal(c, d)
    # the four pinned inputs do not depend on their batch: the same rows through a batch below the gate (full block)
    small = model.encode_text(ids[:4], normalize=True)
    assert torch.equal(a[:4], small)


def test_vitl14_336_streaming_attention_pooled_equals_full(device):
    """T = 577 (streaming attention); 4 images = 2 308 token rows, just past the gate."""
    model, _ = mmr_amd.load("ViT-L/14@336px", device=device, weights="synthetic")
    px = synth.synth_images(4, 336, seed=8).bfloat16().to(device)
    for normalize in (True, False):
        a, b = _ab(model, lambda: model.encode_image(px, normalize=normalize))
        assert torch.isfinite(a).all() and torch.equal(a, b)
    three = model.encode_image(px[:3], normalize=True)                  # 1 731 rows: below the gate
    assert torch.equal(model.encode_image(px, normalize=True)[:3], three)


@pytest.mark.parametrize("name,below,above", [("ViT-B/32", 40, 41), ("tiny-test", 120, 121)])
def test_both_sides_of_the_batch_gate_give_the_same_bits(device, name, below, above):
    """The pooled path starts above 2 048 padded token rows (ViT-B/32: 40 x 50 = 2 000 -> 2 048 stays full, 41 x 50 =
    2 050 -> 2 176 is pooled; tiny-test: 120 / 121 x 17).  Same inputs, same bits on either side and under the switch."""
    kw = {"weights": "synthetic"} if name != "tiny-test" else {}
    model, _ = mmr_amd.load(name, device=device, **kw)
    S = model.input_resolution
    px = synth.synth_images(above, S, seed=12).to(device)
    lo_pooled, lo_full = _ab(model, lambda: model.encode_image(px[:below], normalize=True))
    hi_pooled, hi_full = _ab(model, lambda: model.encode_image(px, normalize=True))
    assert torch.equal(lo_pooled, lo_full) and torch.equal(hi_pooled, hi_full)
    assert torch.equal(hi_pooled[:below], lo_pooled)
    vis = model.visual
    assert vis.L.mmr_tower_workspace_bytes(vis.handle, above) > vis.L.mmr_tower_workspace_bytes(vis.handle, below)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("T", [20, 50, 77, 130, 200])
def test_pooled_attention_row_equals_full_kernel_bitwise(device, T, causal):
    """Every pooled instantiation (the 32-, 64- and 96-token instances, a two-block stream and a stream with a partial
    last block, plain and causal -- the towers reach only half of them) against the full kernel on the same qkv: the
    first row, the last row, mid-sequence and both sides of a 16-query block edge.  Ten (sequence, head) pairs: the third
    workgroup has two idle waves."""
    from mmr_amd import _lib as L
    B, heads = 5, 2
    d = heads * 64
    g = torch.Generator().manual_seed(T + causal)
    qkv = (torch.randn(B * T, 3 * d, generator=g) * 1.5).bfloat16().to(device)
    picks = torch.tensor([0, T - 1, T // 2, min(15, T - 1), min(16, T - 1)], dtype=torch.int32, device=device)
    rows = torch.arange(B, device=device) * T + picks.long()
    q = qkv[rows, :d].contiguous()
    o_full = torch.zeros(B * T, d, dtype=torch.bfloat16, device=device)
    o_pooled = torch.zeros(B, d, dtype=torch.bfloat16, device=device)
    L.check(L.lib().mmr_debug_attention(qkv.data_ptr(), o_full.data_ptr(), B, T, heads, causal, L.stream_ptr(device)))
    L.check(L.lib().mmr_debug_attention_pooled(q.data_ptr(), qkv.data_ptr(), picks.data_ptr(), o_pooled.data_ptr(), B, T, heads,
                                               causal, L.stream_ptr(device)))
    torch.cuda.synchronize(device)
    assert torch.isfinite(o_full.float()).all() and torch.isfinite(o_pooled.float()).all()
    for b in range(B):
        assert torch.equal(o_pooled[b], o_full[int(rows[b])]), f"T={T} causal={causal}: sequence {b}, query {int(picks[b])}"


def test_tap_of_the_last_block_keeps_the_full_path(device):
    """A tap after the last block needs every row of the residual stream: the forward must fill it, and the features
    are the pooled path's."""
    model, _ = mmr_amd.load("tiny-test", device=device)
    vis = model.visual
    B, T, d, layers = 131, vis.cfg.tokens, vis.cfg.width, vis.cfg.layers
    px = synth.synth_images(B, model.input_resolution, seed=3).to(device)
    feats = vis.forward(px, torch.float32, True)
    taps = []
    for on in (False, True):
        vis.set_full_last_block(on)
        tap = torch.full((B * T, d), float("nan"), device=device)
        f = vis.forward(px, torch.float32, True, tap_after=layers - 1, tap=tap)
        assert torch.equal(f, feats) and torch.isfinite(tap).all()
        taps.append(tap)
    vis.set_full_last_block(False)
    assert torch.equal(taps[0], taps[1])
    # an earlier tap does not hold the pooled path back
    tap = torch.full((B * T, d), float("nan"), device=device)
    assert torch.equal(vis.forward(px, torch.float32, True, tap_after=layers - 2, tap=tap), feats)
    assert torch.isfinite(tap).all()


def test_two_lanes_in_flight_under_shared_chip(device):
    model, _ = mmr_amd.load("ViT-B/32", device=device, weights="synthetic")
    model.bfloat16()
    S, T, V = model.input_resolution, model.cfg.text.tokens, model.cfg.text.vocab
    px = [synth.synth_images(256, S, seed=s).bfloat16().to(device) for s in (20, 21)]
    ids = [_eot_ids(256, T, V, seed=s).to(device) for s in (22, 23)]
    _full(model, True)
    ref = [(model.encode_image(px[k], normalize=True), model.encode_text(ids[k], normalize=True)) for k in range(2)]
    _full(model, False)
    torch.cuda.synchronize(device)
    streams = [torch.cuda.Stream(device) for _ in range(2)]
    main = torch.cuda.current_stream(device)
    with model.shared_chip():
        for st in streams:
            st.wait_stream(main)
        out = [None, None]
        for step in range(6):                                       # interleaved submission: lane 0, lane 1, lane 0, ...
            k = step & 1
            with torch.cuda.stream(streams[k]):
                out[k] = (model.encode_image(px[k], normalize=True, lane=k), model.encode_text(ids[k], normalize=True, lane=k))
        for st in streams:
            main.wait_stream(st)
        torch.cuda.synchronize(device)
    for k in range(2):
        assert torch.equal(out[k][0], ref[k][0]) and torch.equal(out[k][1], ref[k][1])


def test_pooled_forward_is_graph_capturable(device):
    """The pick runs on the device: capture and replay of a batch past the gate, text tower included."""
    model, _ = mmr_amd.load("tiny-test", device=device)
    T, V = model.cfg.text.tokens, model.cfg.text.vocab
    px = synth.synth_images(131, model.input_resolution, seed=3).to(device)
    ids = _eot_ids(37, T, V, seed=4).to(device)
    ref = (model.encode_image(px, normalize=True).clone(), model.encode_text(ids, normalize=True).clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.encode_image(px, normalize=True); model.encode_text(ids, normalize=True)   # warm
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = (model.encode_image(px, normalize=True), model.encode_text(ids, normalize=True))
    torch.cuda.current_stream().wait_stream(side)
    ids2 = ids.clone()
    ids2[5] = torch.roll(ids[5], 7)                                  # replay reads the ids of the moment: a moved EOT
    want = model.encode_text(ids2, normalize=True).clone()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
    ids.copy_(ids2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[1], want)
