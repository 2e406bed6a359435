"""TEST INFRASTRUCTURE ONLY -- fp64 stage references for the BERT text tower, one function per stage, with the device's
rounding points made explicit, and the fixtures and bounds that tests/test_bert_stages_gpu.py (device against reference)
and tests/test_bert_stage_controls_host.py (reference against a deliberately wrong reference) share.

The arithmetic restates transformers/models/bert/modeling_bert.py as oracle/bert_ref.py does; the rounding points are
those of mmr_bert_forward_masked (csrc/tower.hip), in its order:

   1  x = bf16(h)                      the block's GEMM operand (h itself stays fp32 for the residual add)
   2  qkv = bf16(x Wqkv^T + b)
   3  attention output, bf16
   4  h = LN1(attn Wo^T + b + h), fp32, and x = bf16(h)
   5  u = bf16(GELU(x W1^T + b))
   6  h = LN2(u W2^T + b + h), fp32
   7  xc = bf16(h)[:, 0]               gather_first_rows, a copy
   8  pooled = bf16(tanh(xc Wp^T + b))
   9  feat = pooled Wc^T + b, fp32
  10  finish: feat (/ |feat|) rounded to the output dtype

Every function takes ``mut=None`` or one name of MUTATIONS: a mistake planted on purpose, which the pin that owns the
stage has to notice (the host test shows that it does).  ``rounding=False`` drops every rounding point, which leaves
oracle/bert_ref.py's arithmetic in fp64.
"""
import math

import torch

MUTATIONS = ("pos_shift", "types_ignored", "types_swapped", "mask_off_by_one", "mask_ignored", "eps_1e-5", "quickgelu",
             "ln2_uses_ln1", "pool_token1", "pool_bias_dropped", "no_tanh", "cls_bias_dropped")
EMBED_MUTATIONS = ("pos_shift", "types_ignored", "types_swapped", "eps_1e-5")
BLOCK_MUTATIONS = ("mask_off_by_one", "mask_ignored", "quickgelu", "ln2_uses_ln1")
TAIL_MUTATIONS = ("pool_token1", "pool_bias_dropped", "no_tanh", "cls_bias_dropped")

U32 = 2.0 ** -24          # unit roundoff of fp32
U_OUT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _known(mut):
    if mut is not None and mut not in MUTATIONS:
        raise ValueError(f"unknown mutation {mut!r}")


def _bf16(x, rounding=True):
    """What the device does: the fp32 value rounded once to bf16 (nearest even)."""
    return x.float().bfloat16().double() if rounding else x


def _f32(x, rounding=True):
    return x.float().double() if rounding else x


def ln64(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.double() + b.double()


def _eps(cfg, mut):
    return 1e-5 if mut == "eps_1e-5" else cfg.ln_eps


# ------------------------------------------------------------------------------------------------ the three stages
def embed_pre(w, cfg, ids, types, mut=None):
    """(word + type) + position before the LayerNorm, fp64 [N,T,d]."""
    _known(mut)
    ids = ids.long()
    N, T = ids.shape
    types = torch.zeros_like(ids) if types is None else types.long()
    if mut == "types_ignored":
        types = torch.zeros_like(ids)
    elif mut == "types_swapped":
        types = 1 - types
    pos = torch.arange(T)
    if mut == "pos_shift":
        pos = (pos - 1).clamp(min=0)
    return (w["b.tok"].double()[ids] + w["b.type"].double()[types]) + w["b.pos"].double()[pos]


def embed(w, cfg, ids, types, mut=None, rounding=True):
    """The residual stream after the embedding LayerNorm (tap_after = -1), fp64 [N,T,d]."""
    h = ln64(embed_pre(w, cfg, ids, types, mut), w["b.ln_emb.w"], w["b.ln_emb.b"], _eps(cfg, mut))
    return _f32(h, rounding)


def block(w, cfg, i, h_in, mask, mut=None, rounding=True):
    """Block i applied to the residual stream h_in [N,T,d] (tap_after = i-1) -> the stream after it (tap_after = i).
    ``mask`` [N,T] (0 = padded key) or None.  A sequence needs at least one kept key."""
    _known(mut)
    r = rounding
    N, T, d = h_in.shape
    heads, dh = cfg.heads, d // cfg.heads
    p, eps = f"b.l{i}", _eps(cfg, mut)
    W = lambda n: w[f"{p}.{n}"].double()                                    # noqa: E731
    h = h_in.double()
    x = _bf16(h, r)                                                         # 1
    qkv = _bf16(x @ W("qkv.w").t() + W("qkv.b"), r)                         # 2
    q, k, v = (t.view(N, T, heads, dh).transpose(1, 2) for t in qkv.split(d, dim=-1))
    scores = (q @ k.transpose(-1, -2)) * dh ** -0.5
    if mask is not None and mut != "mask_ignored":
        keep = mask.bool().clone()
        if mut == "mask_off_by_one":                                        # the last kept key is dropped as well
            last = keep.long().cumsum(1).argmax(1)
            keep[torch.arange(N), last] = False
        # HF's additive mask: the most negative fp32 number on a padded key (a row left with no key attends evenly)
        bias = torch.zeros(N, 1, 1, T, dtype=torch.float64)
        bias.masked_fill_(~keep.view(N, 1, 1, T), torch.finfo(torch.float32).min)
        scores = scores + bias
    ctx = _bf16((torch.softmax(scores, dim=-1) @ v).transpose(1, 2).reshape(N, T, d), r)        # 3
    h = _f32(ln64(ctx @ W("out.w").t() + W("out.b") + h, W("ln1.w"), W("ln1.b"), eps), r)       # 4
    x = _bf16(h, r)
    pre = x @ W("fc1.w").t() + W("fc1.b")
    u = pre * torch.sigmoid(1.702 * pre) if mut == "quickgelu" else 0.5 * pre * (1 + torch.erf(pre / math.sqrt(2.0)))
    u = _bf16(u, r)                                                         # 5
    ln2 = "ln1" if mut == "ln2_uses_ln1" else "ln2"
    return _f32(ln64(u @ W("fc2.w").t() + W("fc2.b") + h, W(f"{ln2}.w"), W(f"{ln2}.b"), eps), r)   # 6


def _tail_parts(w, cfg, h_last, mut, rounding):
    _known(mut)
    tok = 1 if mut == "pool_token1" and h_last.shape[1] > 1 else 0
    xc = _bf16(h_last.double()[:, tok], rounding)                           # 7
    z = xc @ w["b.pool.w"].double().t()
    if mut != "pool_bias_dropped":
        z = z + w["b.pool.b"].double()
    pooled = _bf16(z if mut == "no_tanh" else torch.tanh(z), rounding)      # 8
    feat = pooled @ w["b.cls.w"].double().t()
    if mut != "cls_bias_dropped":
        feat = feat + w["b.cls.b"].double()
    return z, pooled, _f32(feat, rounding)                                  # 9


def tail(w, cfg, h_last, normalize, out_dtype, mut=None, rounding=True):
    """The logits from the residual stream after the last block, h_last [N,T,d] (tap_after = layers-1), fp64 [N,E]."""
    _, _, feat = _tail_parts(w, cfg, h_last, mut, rounding)
    if normalize:
        feat = feat / feat.norm(dim=-1, keepdim=True)
    return feat.to(out_dtype).double() if rounding else feat                # 10


def logits(w, cfg, ids, mask=None, types=None, mut=None, rounding=False):
    """The three stages composed: the whole forward."""
    h = embed(w, cfg, ids, types, mut, rounding)
    for i in range(cfg.layers):
        h = block(w, cfg, i, h, mask, mut, rounding)
    return tail(w, cfg, h, False, torch.float32, mut, rounding)


# ------------------------------------------------------------------------------------------------ derived bounds
def embed_bound(w, cfg, ids, types, ref):
    """Per element, in the form of the vision-embedding bound (test_encoder_stages_gpu.vision_embed_bound), which holds
    the same ln_row: an error of the pre-LayerNorm value reaches the output scaled by |gamma| / std(row), plus
    test_layernorm's floor for the fp32 statistics, 1e-5 max|ref|.  Where the vision kernel's pre-LN value comes out of
    a GEMM (3e-5 of its scale), this kernel's is two fp32 additions of exact operands, (tok + type) + pos: two roundings
    of at most 2^-24 of the larger magnitude each, 2^-23 max(|tok + type|, |pre|) <= 2^-23 (|tok| + |type| + |pos|)."""
    ids = ids.long()
    types = torch.zeros_like(ids) if types is None else types.long()
    mag = (w["b.tok"].double()[ids].abs() + w["b.type"].double()[types].abs()) + w["b.pos"].double()[:ids.shape[1]].abs()
    std = embed_pre(w, cfg, ids, types).std(dim=-1, unbiased=False, keepdim=True)
    return 2.0 ** -23 * mag * w["b.ln_emb.w"].double().abs() / std + 1e-5 * ref.abs().max().item()


def ln_x_bound(ref):
    """test_layernorm's bound for the bf16 output: one rounding (2^-8 relative) plus 1e-5 of the largest output."""
    return 2.0 ** -8 * ref.abs() + 1e-5 * ref.abs().max().item()


def ln_h_bound(h, w, ref, d, eps):
    """Per element, for the fp32 output of ln_row (csrc/vit_ops.hip) on rows that are not constant, u = 2^-24:
      mean   d/64 adds per lane, 6 adds across the wave, one divide: |dmean| <= (d/64 + 7) u mean|x|  =: m
      t      = x - mean: |dt| <= m + u |t|
      var    = sum t^2 / d; sum(t) = 0, so m enters at second order only; the squares, the d/64 + 6 adds and the divide
               give a relative (d/64 + 9) u, and m at most 2 m / sigma
      rstd   = rsqrt(var + eps): half of var's relative error plus the instruction's own (taken as 4 u)
      out    = t rstd gamma + beta: three more roundings
    |out - ref| <= |gamma| rstd m + |gamma t rstd| (m / sigma + (d/128 + 12) u) + u |ref|, with rstd <= 1 / sigma.
    Constant rows (sigma = 0) have no such bound; they are pinned exactly instead."""
    h, w = h.double(), w.double()
    mu = h.mean(-1, keepdim=True)
    sigma = (h - mu).std(dim=-1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(sigma ** 2 + eps)
    m = (d / 64 + 7) * U32 * h.abs().mean(-1, keepdim=True)
    n = (h - mu).abs() * rstd
    return w.abs() * (rstd * m + n * (m / sigma + (d / 128 + 12) * U32)) + U32 * ref.abs()


def tail_bound(w, cfg, h_last, normalize, out_dtype):
    """Per element, in the form of the CLIP tail bound (test_encoder_stages_gpu.tail_reference).  The gathered rows
    are a copy of bf16(h), the same on both sides.  z = xc Wp^T + b accumulates in fp32: 3e-5 max(1, max|z|)
    (test_gemm_epilogues), which tanh (slope <= 1) passes on at most unchanged, dz.  The device then rounds its tanh
    value to bf16, half an ulp <= 2^-8 |pooled|, and so does the reference (rounding point 8): the two pooled rows
    differ by at most dz + 2 * 2^-8 |pooled| per element, which the classifier spreads over its row:
      |feat - ref| <= (2^-8 |pooled| [device] + 2^-8 |pooled| [reference's half-ulp] + dz) @ |Wc|^T + 3e-5 max(1, max|ref|)
    the last term being the classifier's own fp32 accumulation.  Normalised as in tail_reference; the output dtype adds
    its half-ulp once for the device and once for the reference."""
    z, pooled, ref = _tail_parts(w, cfg, h_last, None, True)
    dz = 3e-5 * max(1.0, z.abs().max().item())
    bound = (2 * 2.0 ** -8 * pooled.abs() + dz) @ w["b.cls.w"].double().abs().t() + 3e-5 * max(1.0, ref.abs().max().item())
    if normalize:
        nrm = ref.norm(dim=-1, keepdim=True)
        rho = bound.norm(dim=-1, keepdim=True) / nrm
        ref = ref / nrm
        bound = bound / nrm + ref.abs() * (rho / (1 - rho) + 2.0 ** -22)
    return bound + 2 * U_OUT[out_dtype] * ref.abs()


# ------------------------------------------------------------------------------------------------ fixtures
WIDTHS = (128, 512, 768, 1024)                   # the four MMR_VPL_SWITCH cases
SHAPES = ((3, 1), (5, 33), (2, 64), (4, 97), (3, 130), (2, 160))
MAX_POSITIONS, VOCAB = 160, 1000


def stage_config(width):
    from mmr_amd.config import BertTextConfig
    return BertTextConfig(f"stage-bert-{width}", width=width, layers=2, heads=width // 64, mlp=4 * width,
                          max_positions=MAX_POSITIONS, vocab=VOCAB, embed_dim=128 if width == 128 else 768)


_WEIGHTS = {}


def stage_weights(width):
    """The seeded synthetic weights, changed by bf16-exact steps so that planted mistakes show:
      fc1.b  sixteenths in [-3, -1.5] for seven units of eight and in [1.5, 3] for the eighth (stock: 0.02 randn), so that
             the pre-activations span about [-3, 3].  With the stock bias every pre-activation sits within a few tenths
             of zero, where QuickGELU and erf-GELU agree to 1e-3; near +-2 they differ by 2e-2.  Most units sit on the
             negative side because GELU is small there and so is its bf16 rounding step: on the CPU the QuickGELU control
             stands 8.5x to 13x above the block's rounding floor this way, 3.8x to 5x with an even spread
      pool.b, cls.b  x 8: the stock 0.02 is smaller than what the tail's |.|-summed bound allows at width 1024
    The attention weights are left as they are."""
    if width not in _WEIGHTS:
        from mmr_amd import weights
        cfg = stage_config(width)
        w = dict(weights.make_bert_weights(cfg, seed=5))
        j = torch.arange(cfg.mlp)
        for i in range(cfg.layers):
            w[f"b.l{i}.fc1.b"] = ((((j * 37 + 11 * i) % 25) + 24) * torch.where(j % 8 == 0, 1, -1)).float() / 16.0
        w["b.pool.b"] = w["b.pool.b"] * 8.0
        w["b.cls.b"] = w["b.cls.b"] * 8.0
        for k, v in w.items():
            assert torch.equal(v, v.bfloat16().float()), k
        _WEIGHTS[width] = w
    return stage_config(width), _WEIGHTS[width]


def stage_batch(N, T, seed=0):
    """ids, mask, types [N,T] int32: very short sequences beside full ones (lengths T, 1, 17, T-1, 5, ...), pads are id 0,
    both token types inside every row that has two kept tokens; ids 0 and vocab-1 occur among the kept tokens."""
    g = torch.Generator().manual_seed(1000 * N + T + seed)
    lens = torch.tensor([min(max(v, 1), T) for v in (T, 1, 17, T - 1, 5)][:N])
    mask = (torch.arange(T)[None, :] < lens[:, None]).int()
    ids = torch.randint(1, VOCAB, (N, T), generator=g, dtype=torch.int32)
    ids[:, 0] = 101
    if T > 2:
        ids[0, 1], ids[0, T - 1] = 0, VOCAB - 1
    else:
        ids[0, 0], ids[N - 1, 0] = 0, VOCAB - 1
    ids = ids * mask
    types = ((torch.arange(T)[None, :] >= (lens[:, None] + 1) // 2).int()) * mask
    return ids, mask, types


def wrong_pool_rows(N, T):
    """Rows of the flat [N*T, d] stream that a first-row gather with a wrong stride or offset would take for sequence n."""
    n = torch.arange(N)
    return (("row n", n), ("row n*T + 1", n * T + 1), ("row n*T + T - 1", n * T + T - 1))


def frac_of_max(got, ref):
    """Largest error as a fraction of the largest |reference| entry."""
    return ((got.double() - ref.double()).abs().max() / ref.double().abs().max()).item()
