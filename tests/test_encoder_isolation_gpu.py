"""Nothing leaks into an encoder result from the workspace, from the other rows of the batch or from the previous call.

A tower forward runs every GEMM over padded row counts of a torch.empty workspace that LayerNorm, attention, im2col and
the pooling kernel never write; the fused patch gather re-reads the last patch for its padding rows; attention stages
rows past T from row T-1 and prefetches the next (sequence, head) pair.  Every comparison here is bitwise (exact): the
two runs of a pair use the same batch size, hence the same launch geometry.  NaN and 3e38 are ordinary values to the
hardware and every access stays inside the allocated buffers.
"""
import dataclasses

import pytest
import torch

import mmr_amd
from mmr_amd import synth, weights

pytestmark = pytest.mark.gpu

FOLD = pytest.mark.parametrize("fold", [False, True], ids=["ln", "ln-folded"])
LAYERS = 2          # the shipped widths and token counts, two blocks deep: every kernel of a block runs twice over stale data


@pytest.fixture(scope="module")
def L(device):
    from mmr_amd import _lib
    return _lib


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu()


_towers = {}


def _tower(device, name, kind, fold):
    """A two-block tower of the named model's width and token count, cached for the module."""
    key = (name, kind, fold)
    if key not in _towers:
        from mmr_amd.clip import _Tower
        ccfg = mmr_amd.get_config(name)
        cfg = dataclasses.replace(ccfg.vision if kind == "v" else ccfg.text, layers=LAYERS)
        w = weights.make_vision_weights(cfg, seed=4) if kind == "v" else weights.make_text_weights(cfg, seed=4)
        _towers[key] = _Tower(cfg, w, device, fold_ln=fold)
    return _towers[key]


def _forward(tower, inp):
    """-> (feature bits, last-block tap [B,T,d] fp32 on the CPU, status word)."""
    cfg = tower.cfg
    B = inp.shape[0]
    tap = torch.full((B * cfg.tokens, cfg.width), float("nan"), device=tower.device)
    feat = tower.forward(inp, torch.float32, True, cfg.layers - 1, tap)
    torch.cuda.synchronize(tower.device)
    return feat.cpu(), tap.cpu().view(B, cfg.tokens, cfg.width), tower.status_word()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _input(tower, B, dtype, seed):
    cfg = tower.cfg
    if cfg.kind == "vision":
        return synth.synth_images(B, cfg.image_size, seed=seed).to(dtype).to(tower.device)
    return synth.synth_token_ids(B, cfg.tokens, cfg.vocab, seed=seed).to(tower.device)


# ------------------------------------------------------------------ workspace poison
# every padded extent is really padded: B*T and B are no multiples of 128; 6 500 / 4 620 / 15 000 rows take the 256-row
# padding rule (M >= 4096); 300 bf16 images take the fused patch gather with padding rows; patch 14 has K padded 588 -> 640
POISON_CASES = [("ViT-B/32", "v", 5, torch.float32), ("ViT-B/32", "v", 130, torch.float32),
                ("ViT-B/32", "v", 300, torch.bfloat16), ("ViT-L/14", "v", 5, torch.float32),
                ("ViT-B/32", "t", 3, None), ("ViT-B/32", "t", 60, None)]


@pytest.mark.parametrize("name,kind,B,dtype", POISON_CASES)
@FOLD
def test_tower_forward_ignores_workspace_contents(device, name, kind, B, dtype, fold):
    tower = _tower(device, name, kind, fold)
    T = tower.cfg.tokens
    assert (B * T) % 128 and B % 128
    inp = _input(tower, B, dtype, seed=60 + B)
    ws = tower.workspace(B)
    feat0, tap0, st0 = _forward(tower, inp)
    assert tower.workspace(B).data_ptr() == ws.data_ptr()
    assert torch.isfinite(feat0).all() and torch.isfinite(tap0).all() and st0 == 0
    for fill in (0x00, 0xFF):                                 # 0xFF: NaN as fp32 and as bf16, -1 as the status word
        ws.fill_(fill)
        feat, tap, st = _forward(tower, inp)
        assert _same(feat, feat0), f"features depend on the workspace contents (fill {fill:#x})"
        assert _same(tap, tap0), f"the residual stream depends on the workspace contents (fill {fill:#x})"
        assert st == 0, "the status word was not cleared by the forward"


@pytest.mark.parametrize("N,T", [(3, 19), (70, 64)])          # 57 rows; 4 480 rows (256-row padding rule)
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_bert_forward_ignores_workspace_contents(device, N, T, masked):
    enc = mmr_amd.load_text_encoder("tiny-bert-test", device=device)
    cfg = enc.cfg
    g = torch.Generator().manual_seed(N + T)
    ids = torch.randint(0, cfg.vocab, (N, T), generator=g, dtype=torch.int32).to(device)
    mask = None
    if masked:
        lens = torch.randint(1, T + 1, (N,), generator=g)
        mask = (torch.arange(T)[None, :] < lens[:, None]).int().to(device)

    def run():
        tap = torch.full((N * T, cfg.width), float("nan"), device=device)
        out = enc.logits(ids, attention_mask=mask, tap_after=cfg.layers - 1, tap=tap)
        torch.cuda.synchronize(device)
        return out.cpu(), tap.cpu(), enc.id_errors()

    out0, tap0, err0 = run()
    assert torch.isfinite(out0).all() and torch.isfinite(tap0).all() and not err0
    for fill in (0x00, 0xFF):
        enc._ws.fill_(fill)
        out, tap, err = run()
        assert _same(out, out0) and _same(tap, tap0) and not err, f"fill {fill:#x}"


# ------------------------------------------------------------------ batch-mate independence
def _others(B, keep):
    return [i for i in range(B) if i != keep]


# The in-register attention kernels (T <= 96) run a persistent grid of at most (CUs x resident workgroups per CU) workgroups
# -- 1 280 on the MI355X for T <= 64, 768 for T <= 96 -- and a workgroup with a second (sequence, head) pair prefetches it
# while it works on the first.  130 images x 12 heads = 1 560 pairs and 130 prompts x 8 heads = 1 040 pairs are above
# those caps, so there a kept sequence's workgroup also loads a batch mate's pair; at 7 every workgroup has one pair.
@pytest.mark.parametrize("name,B", [("ViT-B/32", 7),          # T = 50: the 64-token in-register kernel, one pair per workgroup
                                    ("ViT-B/32", 130),        # ... and two pairs per workgroup: the next-pair prefetch runs
                                    ("ViT-B/16", 4)])         # T = 197: the streaming kernel
@FOLD
def test_image_embedding_does_not_depend_on_its_batch_mates(device, name, B, fold):
    tower = _tower(device, name, "v", fold)
    px = _input(tower, B, torch.float32, seed=70)
    feat0, tap0, _ = _forward(tower, px)
    assert torch.isfinite(feat0).all()
    for keep in (0, B // 2, B - 1):
        for what in ("nan", "3e38", "other"):
            mod = _input(tower, B, torch.float32, seed=71) if what == "other" else \
                torch.full_like(px, float("nan") if what == "nan" else 3e38)
            if what == "3e38":
                mod[:, :, ::2] = -3e38
            mod[keep] = px[keep]
            feat, tap, _ = _forward(tower, mod)
            assert _same(feat[keep], feat0[keep]), f"image {keep}: feature changed when its batch mates became {what}"
            assert _same(tap[keep], tap0[keep]), f"image {keep}: residual rows changed when its batch mates became {what}"


@pytest.mark.parametrize("N", [7, 130])                       # 130: two pairs per workgroup (see above)
@FOLD
def test_text_embedding_does_not_depend_on_its_batch_mates(device, fold, N):
    tower = _tower(device, "ViT-B/32", "t", fold)             # T = 77 causal: the 96-token kernel
    V = tower.cfg.vocab
    ids = _input(tower, N, None, seed=72)
    feat0, tap0, st0 = _forward(tower, ids)
    assert torch.isfinite(feat0).all() and st0 == 0
    for keep in (0, N // 2, N - 1):
        for what in ("other", "out-of-range"):
            mod = _input(tower, N, None, seed=73)
            if what == "out-of-range":
                mod[:, 1::3] = V + 5
                mod[:, 2::3] = -1
            mod[keep] = ids[keep]
            feat, tap, st = _forward(tower, mod)
            assert _same(feat[keep], feat0[keep]) and _same(tap[keep], tap0[keep]), f"prompt {keep} changed with {what} batch mates"
            assert st == (1 if what == "out-of-range" else 0)


def test_bert_row_does_not_depend_on_the_other_rows_masks(device):
    enc = mmr_amd.load_text_encoder("tiny-bert-test", device=device)
    cfg = enc.cfg
    N, T = 5, 33
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, cfg.vocab, (N, T), generator=g, dtype=torch.int32).to(device)
    lens = torch.randint(1, T + 1, (N,), generator=g)
    mask = (torch.arange(T)[None, :] < lens[:, None]).int()

    def run(m, i):
        tap = torch.full((N * T, cfg.width), float("nan"), device=device)
        out = enc.logits(i, attention_mask=m.to(device), tap_after=cfg.layers - 1, tap=tap)
        torch.cuda.synchronize(device)
        return out.cpu(), tap.cpu().view(N, T, cfg.width)

    out0, tap0 = run(mask, ids)
    for keep in (0, N // 2, N - 1):
        for what in ("ones", "one-key", "other-ids"):
            m, i = mask.clone(), ids
            if what == "ones":
                m[:] = 1
            elif what == "one-key":
                m[:] = 0
                m[:, 0] = 1
            else:
                i = torch.randint(0, cfg.vocab, (N, T), generator=g, dtype=torch.int32).to(device)
                i[keep] = ids[keep]
            m[keep] = mask[keep]
            out, tap = run(m, i)
            assert _same(out[keep], out0[keep]) and _same(tap[keep], tap0[keep]), f"row {keep} changed ({what})"


# one T per launcher family: in-register kernels of 32 / 64 / 96 tokens, the streaming kernel with 64-query workgroups
# (T = 130: padding to 128-query workgroups would waste a block) and with 128-query workgroups (T = 250)
@pytest.mark.parametrize("T", [20, 50, 77, 130, 250])
@pytest.mark.parametrize("mode", ["full", "causal", "masked"])
def test_attention_sequence_does_not_depend_on_its_neighbours(L, device, T, mode):
    B, heads = 3, 2
    d = heads * 64
    g = torch.Generator().manual_seed(13 * T)
    PAD = 256                                                 # NaN rows after the last sequence, inside the buffer
    base = torch.full((B * T + PAD, 3 * d), float("nan"), dtype=torch.bfloat16)
    base[:B * T] = (torch.randn(B * T, 3 * d, generator=g) * 1.5).bfloat16()
    lens = torch.randint(1, T + 1, (B,), generator=g)
    mask = (torch.arange(T)[None, :] < lens[:, None]).int().to(device)

    def run(qkv):
        qd = qkv.to(device)
        o = torch.full((B * T + PAD, d), 7.0, dtype=torch.bfloat16, device=device)
        if mode == "masked":
            L.check(L.lib().mmr_debug_attention_masked(qd.data_ptr(), o.data_ptr(), B, T, heads, mask.data_ptr(), L.stream_ptr(device)))
        else:
            L.check(L.lib().mmr_debug_attention(qd.data_ptr(), o.data_ptr(), B, T, heads, int(mode == "causal"), L.stream_ptr(device)))
        torch.cuda.synchronize(device)
        o = o.cpu()
        assert torch.equal(o[B * T:].float(), torch.full((PAD, d), 7.0)), "stores past the last sequence"
        return o[:B * T].view(B, T, d)

    o0 = run(base)
    assert torch.isfinite(o0.float()).all()
    for keep in range(B):
        qkv = base.clone()
        for b in _others(B, keep):
            qkv[b * T:(b + 1) * T] = float("nan")
        o = run(qkv)
        assert _same(o[keep], o0[keep]), f"T={T} {mode}: sequence {keep} changed when its neighbours became NaN"


@pytest.mark.parametrize("T", [20, 50, 77])                   # the 32-, 64- and 96-token in-register kernels
@pytest.mark.parametrize("mode", ["full", "causal", "masked"])
def test_attention_kept_sequences_ignore_nan_pairs_sharing_their_workgroup(L, device, T, mode):
    """The persistent in-register kernel with several pairs per workgroup: 1 733 sequences x 4 heads = 6 932 pairs, five or
    more per workgroup whatever the resident-workgroup cap is (at most 1 280), pair p on workgroup p % grid.  Every
    sequence but a few kept ones is NaN, so the pair a kept pair's workgroup worked on before it (whose K / V sit in the
    other LDS image and whose Q sat in the prefetch registers) and the pair it prefetches while working on it are NaN.  The
    kept sequences' outputs must be the bits of the all-finite launch, and both the bits of a launch of that sequence
    alone (one pair per workgroup, nothing prefetched).

    Regression: the key-mask staging of the 32- and 96-token kernels used to copy whole 64-key slabs into a 32- / 96-entry
    mask image; the excess landed on the first K row of the other LDS buffer -- the pair being worked on -- so with more
    than one pair per workgroup key 0's scores depended on when the DMA landed (first seen here: T = 77 masked)."""
    B, heads = 1733, 4
    d = heads * 64
    g = torch.Generator().manual_seed(17 * T)
    PAD = 256                                                 # NaN rows after the last sequence, inside the buffer
    base = torch.full((B * T + PAD, 3 * d), float("nan"), dtype=torch.bfloat16)
    base[:B * T] = (torch.randn(B * T, 3 * d, generator=g) * 1.5).bfloat16()
    lens = torch.randint(1, T + 1, (B,), generator=g)
    mask = (torch.arange(T)[None, :] < lens[:, None]).int().to(device)
    keep = [0, 1, 5, 320, 321, 866, 1400, B - 2, B - 1]       # first / middle / last, alone and in adjacent pairs

    def launch(qd, o, m, nb):
        if mode == "masked":
            L.check(L.lib().mmr_debug_attention_masked(qd.data_ptr(), o.data_ptr(), nb, T, heads, m.data_ptr(), L.stream_ptr(device)))
        else:
            L.check(L.lib().mmr_debug_attention(qd.data_ptr(), o.data_ptr(), nb, T, heads, int(mode == "causal"), L.stream_ptr(device)))
        torch.cuda.synchronize(device)

    def run(qkv):
        qd = qkv.to(device)
        o = torch.full((B * T + PAD, d), 7.0, dtype=torch.bfloat16, device=device)
        launch(qd, o, mask, B)
        assert (o[B * T:] == 7.0).all(), "stores past the last sequence"
        return o[:B * T].view(B, T, d)[keep].cpu()

    o0 = run(base)
    assert torch.isfinite(o0.float()).all()
    base_d = base.to(device)
    for i, b in enumerate(keep):
        o1 = torch.zeros(T, d, dtype=torch.bfloat16, device=device)
        launch(base_d[b * T:(b + 1) * T], o1, mask[b:b + 1].contiguous(), 1)
        assert _same(o1, o0[i]), f"T={T} {mode}: sequence {b} differs between the {B}-sequence launch and a launch of its own"
    qkv = torch.full_like(base, float("nan"))
    for b in keep:
        qkv[b * T:(b + 1) * T] = base[b * T:(b + 1) * T]
    o = run(qkv)
    for i, b in enumerate(keep):
        assert _same(o[i], o0[i]), f"T={T} {mode}: sequence {b} changed when every other sequence became NaN"


# ------------------------------------------------------------------ call-order independence
@pytest.mark.parametrize("name,kind", [("ViT-B/32", "v"), ("ViT-L/14", "v"), ("ViT-B/32", "t")])
@FOLD
def test_tower_result_does_not_depend_on_the_previous_call(device, name, kind, fold):
    """Batch X after a larger call (whose rows beyond X's M stay in the workspace: "padding holds old data"; for the
    vision towers that call's pixels are NaN, so every row it leaves is NaN), after a smaller one, and on a fresh
    workspace."""
    tower = _tower(device, name, kind, fold)
    B = 5
    x = _input(tower, B, torch.float32, seed=80)
    tower._lanes.clear()                                       # fresh workspace
    feat0, tap0, _ = _forward(tower, x)
    assert torch.isfinite(feat0).all()
    big = _input(tower, 3 * B + 2, torch.float32, seed=81)
    if kind == "v":
        big = torch.full_like(big, float("nan"))
    for prev in (big, x[:2].clone()):
        _forward(tower, prev)
        feat, tap, st = _forward(tower, x)
        assert _same(feat, feat0) and _same(tap, tap0) and st == 0, f"result depends on a previous call of batch {prev.shape[0]}"


def test_bert_result_does_not_depend_on_the_previous_call(device):
    enc = mmr_amd.load_text_encoder("tiny-bert-test", device=device)
    cfg = enc.cfg
    g = torch.Generator().manual_seed(21)
    mk = lambda n, t: torch.randint(0, cfg.vocab, (n, t), generator=g, dtype=torch.int32).to(device)
    x = mk(5, 33)
    out0 = enc.logits(x).cpu()
    for prev in (mk(17, 64), mk(2, 7)):
        enc.logits(prev)
        assert _same(enc.logits(x).cpu(), out0), f"logits depend on a previous call of shape {tuple(prev.shape)}"
