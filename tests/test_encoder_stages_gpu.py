"""Per-element parity of the encoder's glue kernels, through the stage taps of mmr_tower_forward.

  a. embed_text_kernel                        tap -1 of a text tower      exact
  b. im2col / fused patch gather + patch GEMM
     + embed_vision_kernel (LN_pre)           tap -1 of a vision tower    derived bound, tightened to ~3x measured
  c. pool_ln_kernel (EOT arg-max, LN_final)
     + projection GEMM + finish_kernel        feature vs the tapped h     derived bound

Every reference is fp64 on the CPU from the bf16-rounded operands the device consumes (the seeded weights are
bf16-representable already).  Towers here are one block deep where the blocks are not what is tested.
"""
import dataclasses

import numpy as np
import pytest
import torch

import mmr_amd
from mmr_amd import synth, weights
from mmr_amd.config import TowerConfig

pytestmark = pytest.mark.gpu


def _tower(cfg, w, device, fold=False):
    from mmr_amd.clip import _Tower
    return _Tower(cfg, w, device, fold_ln=fold)


def _tap(tower, inp, tap_after, out_dtype=torch.float32, normalize=False):
    cfg = tower.cfg
    tap = torch.full((inp.shape[0] * cfg.tokens, cfg.width), float("nan"), device=tower.device)
    feat = tower.forward(inp, out_dtype, normalize, tap_after, tap)
    torch.cuda.synchronize(tower.device)
    return tap.cpu().view(inp.shape[0], cfg.tokens, cfg.width), feat.cpu()


def _launch_counts(tower, inp):
    """(GEMM launches, row-wise launches) of one forward, from the library's launch profiler."""
    from mmr_amd import _lib
    _lib.prof_enable(True, 64)
    try:
        tower.forward(inp, torch.float32, False)
        torch.cuda.synchronize(tower.device)
        counts = _lib.prof_read()
    finally:
        _lib.prof_enable(False)
    assert counts["dropped"] == 0
    return counts["gemm"][1], counts["rowwise"][1]


def _ln64(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.double() + b.double()


# ------------------------------------------------------------------ a. text embedding
def _text_cfg(name):
    """The named model's text tower, one block deep (the embedding does not depend on the depth)."""
    return dataclasses.replace(mmr_amd.get_config(name).text, layers=1)


@pytest.mark.parametrize("name", ["tiny-test", "ViT-B/32", "ViT-L/14"])      # widths 128, 512, 768
def test_text_embedding_is_exact(device, name):
    cfg = _text_cfg(name)
    w = weights.make_text_weights(cfg, seed=3)
    tower = _tower(cfg, w, device)
    N, T, V = 3, cfg.tokens, cfg.vocab
    assert (N * T) % 4 != 0                                   # four rows per workgroup: the last one is ragged
    ids = synth.synth_token_ids(N, T, V, seed=8)
    ids[0, 3], ids[2, 76], ids[1, 0] = 0, 0, V - 1            # both ends of the table, and zeros that are not padding
    assert int(ids.min()) == 0 and int(ids.max()) == V - 1

    def expect(i):
        # exact: one fp32 add per element
        return w["t.tok"].bfloat16().float()[i.long()] + w["t.pos"][None, :T]

    got, _ = _tap(tower, ids.to(device), -1)
    assert torch.equal(got, expect(ids)), "tok[ids] + pos is not bit-exact"
    assert tower.status_word() == 0
    bad = ids.clone()
    bad[0, 5], bad[2, 40] = -3, V + 11                        # clamped to 0 and to V - 1, and reported
    clamped = ids.clone()
    clamped[0, 5], clamped[2, 40] = 0, V - 1
    got, _ = _tap(tower, bad.to(device), -1)
    assert torch.equal(got, expect(clamped)), "an out-of-range id did not read the clamped id's row"
    assert tower.status_word() == 1
    got, _ = _tap(tower, ids.to(device), -1)
    assert torch.equal(got, expect(ids)) and tower.status_word() == 0


# ------------------------------------------------------------------ b. vision embedding
def position_coded_images(B, S):
    """A pixel's value is a function of its own (image, channel, y, x): integers in [-254, 254] over 64, all
    bf16-representable.  Neighbouring pixels, rows and channels differ by whole steps, so a gather that swaps two kx runs,
    transposes ky / kx, takes another channel or another patch moves the patch sums by far more than the bound."""
    c = torch.arange(3).view(1, 3, 1, 1)
    y = torch.arange(S).view(1, 1, S, 1)
    x = torch.arange(S).view(1, 1, 1, S)
    b = torch.arange(B).view(B, 1, 1, 1)
    idx = (c * S + y) * S + x + 7919 * b
    px = ((idx % 509) - 254).float() / 64.0
    assert torch.equal(px, px.bfloat16().float())
    return px


def vision_embed_reference(w, cfg, px):
    """fp64 LN_pre(concat(cls, conv(px)) + pos) of bf16-rounded pixels -> (reference [B,T,d], pre-LN values [B,T,d])."""
    B, P, G, d = px.shape[0], cfg.patch, cfg.grid, cfg.width
    p = px.bfloat16().double().view(B, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B, G * G, 3 * P * P)
    pe = p @ w["v.patch_w"].double().reshape(d, -1).t()
    pre = torch.cat([w["v.cls"].double().expand(B, 1, d), pe], dim=1) + w["v.pos"].double()
    return _ln64(pre, w["v.ln_pre.w"], w["v.ln_pre.b"], cfg.ln_eps), pre


def vision_embed_bound(w, ref, pre):
    """Derived, per element: the patch GEMM's fp32 result is within 3e-5 * max(1, max |pre-LN|) (test_gemm_epilogues, fp32
    outputs, K <= 3072); LayerNorm scales a row's error by |gamma| / std(row); plus test_layernorm's floor for the fp32
    statistics, 1e-5 * max |ref|."""
    std = pre.std(dim=-1, unbiased=False, keepdim=True)
    return 3e-5 * max(1.0, pre.abs().max().item()) * w["v.ln_pre.w"].double().abs() / std + 1e-5 * ref.abs().max().item()


# measured (MI355X, 2026-10-16) against the fp64 reference above: the largest error over the 14 cases below is 1.96e-2 of
# the derived bound (patch 32, K = 3072: 1.8e-2 .. 2.0e-2 on all three routes; patch 16 / 14: 6.4e-3 .. 9.9e-3).  The guard
# is ~3x that measurement, as a fraction of vision_embed_bound that an element's error may reach.
VISION_EMBED_GUARD = 6e-2


def _images(kind, B, S, seed):
    return synth.synth_images(B, S, seed=seed) if kind == "noise" else position_coded_images(B, S)


def _vision_cfg(name):
    return dataclasses.replace(mmr_amd.get_config(name).vision, layers=1)


def _check_vision_embed(got, w, cfg, px, sample, what):
    ref, pre = vision_embed_reference(w, cfg, px[sample])
    excess = ((got[sample].double() - ref).abs() / vision_embed_bound(w, ref, pre)).max().item()
    print(f"MEASURED vision embed {what}: {excess:.3e} of the derived per-element bound")
    assert excess <= 1.0, f"{what}: error is {excess:.2f}x the derived bound"
    assert excess <= VISION_EMBED_GUARD, f"{what}: {excess:.2e} of the derived bound is above the regression guard {VISION_EMBED_GUARD:.1e}"


@pytest.mark.parametrize("kind", ["noise", "position"])
@pytest.mark.parametrize("B", [5, 256, 300])
def test_vision_embedding_patch32_three_routes(device, kind, B):
    """ViT-B/32: fp32 pixels go through im2col + the plain GEMM; bf16 pixels take the GEMM with the gather fused into its
    A-tile loads at 256 and 300 images (300: ragged, the padding rows re-read the last patch) and fall back to im2col at
    5.  The routes agree bit for bit at equal batch, and each is held to the fp64 reference.  That the bf16 pixels really
    took the fused route shows in the launch counts: the same GEMM launches and one row-wise launch (im2col) fewer."""
    cfg = _vision_cfg("ViT-B/32")
    w = weights.make_vision_weights(cfg, seed=1)
    tower = _tower(cfg, w, device)
    px = _images(kind, B, cfg.image_size, seed=40 + B).bfloat16()
    got16, f16 = _tap(tower, px.to(device), -1)
    got32, f32 = _tap(tower, px.float().to(device), -1)
    assert torch.isfinite(got16).all()
    assert torch.equal(got16, got32) and torch.equal(f16, f32), "bf16-pixel and fp32-pixel routes differ"     # exact
    (g16, r16), (g32, r32) = _launch_counts(tower, px.to(device)), _launch_counts(tower, px.float().to(device))
    assert g16 == g32 and r16 == r32 - (1 if B >= 256 else 0), f"B={B}: launches (gemm, row-wise) bf16 {g16, r16}, fp32 {g32, r32}"
    sample = list(range(B)) if B <= 8 else [0, 255, B - 1] if B > 256 else [0, B // 2, B - 1]
    _check_vision_embed(got16, w, cfg, px.float(), sample, f"ViT-B/32 {kind} B={B}")


@pytest.mark.parametrize("kind", ["noise", "position"])
@pytest.mark.parametrize("name,B", [("ViT-B/16", 5), ("ViT-L/14", 5), ("ViT-L/14", 48), ("ViT-L/14@336px", 3)])
def test_vision_embedding_other_patch_geometries(device, name, B, kind):
    """Patch 16 (vector im2col loads), patch 14 (scalar loads, K = 588 zero-padded to 640), 577 tokens; B = 48 at patch 14
    has 12 288 patch rows, which takes the 256-row GEMM tiles over the padded K."""
    cfg = _vision_cfg(name)
    w = weights.make_vision_weights(cfg, seed=1)
    tower = _tower(cfg, w, device)
    px = _images(kind, B, cfg.image_size, seed=50 + B).bfloat16()
    got16, _ = _tap(tower, px.to(device), -1)
    got32, _ = _tap(tower, px.float().to(device), -1)
    assert torch.equal(got16, got32), "bf16-pixel and fp32-pixel im2col differ"                               # exact
    sample = list(range(B)) if B <= 8 else [0, B // 2, B - 1]
    _check_vision_embed(got16, w, cfg, px.float(), sample, f"{name} {kind} B={B}")


# ------------------------------------------------------------------ c. the tail
def tail_reference(h_pick, ln_w, ln_b, proj, eps, normalize, bf16_out):
    """fp64 feature from the pooled rows h_pick [N,d] -> (ref, bound), per element, derived:
    the kernel rounds xc = LN_final(h) to bf16 once (2^-8 relative per element covers a whole ulp), the projection then
    accumulates in fp32 (3e-5 of the largest output, test_gemm_epilogues): |feat - ref| <= 2^-8 |xc| @ |proj|^T + 3e-5 max|ref|.
    Normalised: f/|f| - r/|r| = (f - r)/|r| - r (|f| - |r|)/(|f| |r|) and ||f| - |r|| <= |f - r|_2 <= |bound|_2, so the
    bound becomes bound/|r| + |r/|r|| * rho / (1 - rho) with rho = |bound|_2 / |r|, plus the fp32 rounding of the divide
    (2^-22 relative).  A bf16 output adds one more 2^-8 |ref|."""
    xc = _ln64(h_pick.double(), ln_w, ln_b, eps)
    ref = xc @ proj.double().t()
    bound = 2.0 ** -8 * (xc.abs() @ proj.double().abs().t()) + 3e-5 * ref.abs().max().item()
    if normalize:
        nrm = ref.norm(dim=-1, keepdim=True)
        rho = bound.norm(dim=-1, keepdim=True) / nrm
        ref = ref / nrm
        bound = bound / nrm + ref.abs() * (rho / (1 - rho) + 2.0 ** -22)
    if bf16_out:
        bound = bound + 2.0 ** -8 * ref.abs()
    return ref, bound


def eot_tie_ids(T, V, seed=0):
    """Seven rows of T = 77 ids (two passes of the kernel's 64-lane scan: lane = position % 64) and where numpy.argmax
    finds their largest id: at 0; 63; 64; 76; twice in one lane's stride (6 and 70: the first wins); twice in different
    lanes, the later lane holding the earlier position (70 and 10); everywhere (all ids equal).  For the tie rows the
    third column is the position a wrong tie rule would take."""
    assert T == 77
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V - 2, (7, T), generator=g, dtype=torch.int32)
    top = V - 1
    for row, where in enumerate([(0,), (63,), (64,), (76,), (6, 70), (70, 10)]):
        ids[row, list(where)] = top
    ids[6] = 500
    want = [0, 63, 64, 76, 6, 10, 0]
    other = [None, None, None, None, 70, 70, 76]
    assert list(np.argmax(ids.numpy(), axis=1)) == want          # numpy guarantees the first occurrence
    return ids, want, other


def _tail_cfgs(width, embed):
    common = dict(width=width, layers=1, heads=width // 64, mlp=4 * width, embed_dim=embed)
    return (TowerConfig("vision", tokens=17, image_size=64, patch=16, **common),
            TowerConfig("text", tokens=77, vocab=1024, **common))


TAIL = pytest.mark.parametrize("width,embed", [(128, 512), (512, 512), (768, 768), (1024, 768)])   # the four VPL instantiations
OUT = pytest.mark.parametrize("normalize,out_dtype", [(False, torch.float32), (True, torch.float32),
                                                      (False, torch.bfloat16), (True, torch.bfloat16)])


def _check_tail(feat, h_pick, w, pre, cfg, normalize, out_dtype, what):
    ref, bound = tail_reference(h_pick, w[f"{pre}.w"], w[f"{pre}.b"], w[f"{pre[0]}.proj"], cfg.ln_eps, normalize,
                                out_dtype == torch.bfloat16)
    assert feat.dtype == out_dtype
    excess = ((feat.double() - ref).abs() / bound).max(dim=-1).values
    print(f"MEASURED tail {what} normalize={normalize} {out_dtype}: {excess.max().item():.3f} of the derived bound")
    assert excess.max().item() <= 1.0, f"{what}: rows {torch.nonzero(excess > 1).flatten().tolist()} exceed the bound ({excess.max().item():.2f}x)"
    return ref, bound


@TAIL
@OUT
def test_vision_tail_from_the_tapped_residual_stream(device, width, embed, normalize, out_dtype):
    cfg, _ = _tail_cfgs(width, embed)
    w = weights.make_vision_weights(cfg, seed=2)
    tower = _tower(cfg, w, device)
    B = 130                                                   # neither a multiple of 4 nor of 128 (Bpad = 256)
    px = synth.synth_images(B, cfg.image_size, seed=6)
    h, feat = _tap(tower, px.to(device), cfg.layers - 1, out_dtype, normalize)
    assert torch.isfinite(h).all()
    _check_tail(feat, h[:, 0], w, "v.ln_post", cfg, normalize, out_dtype, f"vision d={width} E={embed}")


@TAIL
@OUT
def test_text_tail_and_eot_tie_rule(device, width, embed, normalize, out_dtype):
    _, cfg = _tail_cfgs(width, embed)
    w = weights.make_text_weights(cfg, seed=2)
    tower = _tower(cfg, w, device)
    ids7, want7, other7 = eot_tie_ids(cfg.tokens, cfg.vocab)
    reps = 19                                                 # 133 rows: neither a multiple of 4 nor of 128
    ids = ids7.repeat(reps, 1)
    ids[7:, 1] = torch.arange(2, 2 + len(ids) - 7, dtype=torch.int32)      # the copies are different prompts: position 1 is never a
    assert int(ids[7:, 1].max()) < 500                                     # pick and stays below every row's largest id
    want, other = want7 * reps, other7 * reps
    assert list(np.argmax(ids.numpy(), axis=1)) == want
    h, feat = _tap(tower, ids.to(device), cfg.layers - 1, out_dtype, normalize)
    assert torch.isfinite(h).all()
    rows = torch.arange(len(ids))
    ref, bound = _check_tail(feat, h[rows, want], w, "t.ln_final", cfg, normalize, out_dtype, f"text d={width} E={embed}")
    # the test cannot pass on the wrong pick: for every tie row the other candidate's reference is > 10 bounds away
    ties = [r for r in range(len(ids)) if other[r] is not None]
    ref_o, _ = tail_reference(h[ties, [other[r] for r in ties]], w["t.ln_final.w"], w["t.ln_final.b"], w["t.proj"], cfg.ln_eps,
                              normalize, out_dtype == torch.bfloat16)
    apart = ((ref_o - ref[ties]).abs() / bound[ties]).max(dim=-1).values
    assert apart.min().item() > 10.0, f"tie candidates only {apart.min().item():.1f} bounds apart"
