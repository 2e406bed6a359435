"""The three LayerNorm-folded GEMM epilogues (mmr_tower_cfg.fold_ln), one kernel at a time through mmr_debug_gemm_fold.

  epi 7 / 8 (EPI_LNFOLD[_GELU]_BF16): out = act(rstd * (x . W'^T - mean * colsum) + b'), (mean, rstd) from 16 partial
                                      (sum, sumsq) slots per row
  epi 9     (EPI_RESID_STATS_F32)   : h += A . W^T + b, plus x = bf16(h) and the new rows' partial slots

Every reference is computed on the CPU in fp64 from the bf16-rounded operands the device consumes.  Tolerances are
labelled exact / derived / measured where they are defined.

Which GEMM kernel serves a shape (128x128, 256x192 or 256x256 tiles) is the launcher's choice and cannot be seen from
the results, so the three widths are covered twice: by shapes that select each width under the launcher's policy on a
256-CU chip (`_tile` restates that policy; the assertion on it pins this restatement, not the launcher), and by
test_every_tile_width_forced, which runs this file in a child process per width with the launcher's MMR_GEMM_TILE
override (read once per process) on a shape every width accepts.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

NP = 16                 # LNFOLD_NP (csrc/mmr_common.h): partial-sum slots per row
EPS = 1e-5
EINVAL = -22


@pytest.fixture(scope="module")
def L(device):
    from mmr_amd import _lib
    return _lib


def _tile(M, N, cus=256):
    """The GEMM launcher's tile policy (csrc/gemm.hip, launch_gemm_aux) for the folded epilogues, which never take the
    32-column kernel: 256-row tiles need M % 256 == 0 and at least 128 tiles; of the two widths the cheaper by
    (rounds over the CUs) x (tile width) wins.  A restatement for choosing shapes: the launcher is not observed here."""
    def cost(bn):
        if M % 256 or N % bn:
            return -1
        tiles = (M // 256) * (N // bn)
        return -1 if tiles < 128 else (tiles + cus - 1) // cus * bn
    c256, c192 = cost(256), cost(192)
    tile = 256 if c256 > 0 else 128
    if c192 > 0 and (c256 < 0 or c192 < c256):
        tile = 192
    return tile


def _fold(L, device, epi, A, W, bias, out, colsum=None, stats_in=None, inv_d=0.0, stats_out=None, xout=None, M=None):
    """One launch; returns the C return code.  Every tensor is already on the device and stays referenced by the caller."""
    M = A.shape[0] if M is None else M
    N, K = W.shape
    p = lambda t: 0 if t is None else t.data_ptr()
    rc = L.lib().mmr_debug_gemm_fold(epi, A.data_ptr(), W.data_ptr(), M, N, K, bias.data_ptr(), out.data_ptr(), p(colsum),
                                     p(stats_in), inv_d, EPS, p(stats_out), p(xout), L.stream_ptr(device))
    torch.cuda.synchronize(device)
    return rc


# ------------------------------------------------------------------ EPI_RESID_STATS_F32
@pytest.mark.parametrize("M,N,K,tile", [(6400, 768, 768, 128),       # batch-128 out-proj: 12 slabs of 64 columns
                                        (12800, 768, 768, 192),      # 16 slabs of 48: the slot count's edge
                                        (12800, 1024, 1024, 256),    # 16 slabs of 64
                                        (3200, 768, 3072, 128),      # fc2 form: 48 K-tiles
                                        (12800, 768, 3072, 192)])    # fc2 at batch 256
def test_resid_stats_epilogue(L, device, M, N, K, tile):
    assert _tile(M, N) == tile, "the shape no longer selects the tile this case is here for"
    _check_resid_stats(L, device, M, N, K, tile)


def _check_resid_stats(L, device, M, N, K, tile):
    nslabs = N // (48 if tile == 192 else 64)
    g = torch.Generator().manual_seed(M + N + K + 9)
    # asymmetric, non-trivial operands, as in test_gemm_epilogues
    A = (torch.randn(M, K, generator=g) * 0.5).bfloat16()
    W = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    bias = torch.randn(N, generator=g) * 0.1
    h0 = torch.randn(M, N, generator=g)
    ref = h0.double() + A.double() @ W.double().t() + bias.double()
    PAD = 256                                                       # canary rows behind every output
    Ad = torch.full((M + PAD, K), float("nan"), dtype=torch.bfloat16)
    Ad[:M] = A
    Ad, Wd, bd = Ad.to(device), W.to(device), bias.to(device)
    out = torch.full((M + PAD, N), 7.0, device=device)
    out[:M] = h0.to(device)
    xout = torch.full((M + PAD, N), 7.0, dtype=torch.bfloat16, device=device)
    stats = torch.full((M + PAD, NP, 2), float("nan"), device=device)
    stats[M:] = 7.0
    L.check(_fold(L, device, 9, Ad, Wd, bd, out, stats_out=stats, xout=xout, M=M))
    got, gx, gs = out.cpu(), xout.cpu(), stats.cpu()
    assert torch.equal(got[M:], torch.full((PAD, N), 7.0)), "out: stores past the last row"
    assert torch.equal(gx[M:].float(), torch.full((PAD, N), 7.0)), "xout: stores past the last row"
    assert torch.equal(gs[M:], torch.full((PAD, NP, 2), 7.0)), "stats: stores past the last row"
    got, gx, gs = got[:M], gx[:M], gs[:M]
    # derived (test_gemm_epilogues): fp32 accumulation noise of the MFMA for K <= 3072, 3e-5 of the largest output
    scale = max(1.0, ref.abs().max().item())
    excess = ((got.double() - ref).abs() / (3e-5 * scale)).max().item()
    print(f"MEASURED resid_stats {M}x{N}x{K}: out error {excess * 3e-5:.2e} of max |ref| (bound 3e-5)")
    assert excess <= 1.0, f"out: error is {excess:.2f}x the bound"
    # exact: xout is the stored fp32 value rounded once
    assert torch.equal(gx, got.bfloat16()), "xout is not bf16(out)"
    # exact: a producer with `nslabs` column slabs zeroes every slot it does not fill (the buffer held NaN)
    assert torch.isfinite(gs).all(), "a partial slot was left unwritten"
    assert torch.equal(gs[:, nslabs:], torch.zeros(M, NP - nslabs, 2)), f"slots {nslabs}.. are not (0, 0)"
    # derived: N fp32 additions in any order are off by at most N * 2^-24 * sum |terms|
    g64 = got.double()
    tot = gs.double().sum(dim=1)
    for k, terms in ((0, g64), (1, g64 * g64)):
        bound = N * 2.0 ** -24 * terms.abs().sum(dim=1)
        excess = ((tot[:, k] - terms.sum(dim=1)).abs() / bound).max().item()
        assert excess <= 1.0, f"{'sumsq' if k else 'sum'} of the slots: {excess:.2f}x the fp32 summation bound"
    # ... and slot j holds slab j's share (same derivation, per slab)
    slab = g64.view(M, nslabs, N // nslabs)
    for k, terms in ((0, slab), (1, slab * slab)):
        bound = (N // nslabs) * 2.0 ** -24 * terms.abs().sum(dim=2) + 1e-30
        excess = ((gs[:, :nslabs, k].double() - terms.sum(dim=2)).abs() / bound).max().item()
        assert excess <= 1.0, f"slot layout: slab partial {k} is {excess:.2f}x its bound"


def test_resid_stats_refuses_more_slabs_than_slots(L, device):
    """N = 1280 is 20 slabs of 64 columns: more than the 16 slots of a row.  Refused, not run (the buffers are real and
    large enough anyway)."""
    M, N, K = 12800, 1280, 64
    assert _tile(M, N) == 256
    A = torch.zeros(M, K, dtype=torch.bfloat16, device=device)
    W = torch.zeros(N, K, dtype=torch.bfloat16, device=device)
    bias = torch.zeros(N, device=device)
    out = torch.full((M, N), 7.0, device=device)
    xout = torch.full((M + 256, N), 7.0, dtype=torch.bfloat16, device=device)
    stats = torch.full((M + 256, NP, 2), 7.0, device=device)
    rc = _fold(L, device, 9, A, W, bias, out, stats_out=stats, xout=xout)
    assert rc == EINVAL and b"partial slots" in L.lib().mmr_last_error()
    assert (out == 7.0).all() and (stats == 7.0).all() and (xout.float() == 7.0).all()
    # and the hook's own argument checks
    assert _fold(L, device, 6, A, W, bias, out, stats_out=stats, xout=xout) == EINVAL
    assert _fold(L, device, 9, A, W, bias, out) == EINVAL and b"stats_out" in L.lib().mmr_last_error()
    assert _fold(L, device, 7, A, W, bias, out) == EINVAL and b"row stats" in L.lib().mmr_last_error()


# ------------------------------------------------------------------ EPI_LNFOLD_BF16 / EPI_LNFOLD_GELU_BF16
FAMILIES = ("ordinary", "outlier", "large-mean", "constant")


def _rows(M, d, g):
    """Row r belongs to FAMILIES[r % 4]: ordinary rows as in test_layernorm; one channel 50x the rest (what
    test_outlier_channels_like_pretrained_residual_streams plants); mean 30x the standard deviation (where
    sumsq/d - mean^2 cancels in fp32); constant (variance 0; 1.5 is bf16-representable, so x == h there)."""
    h = torch.randn(M, d, generator=g) * 3 + 0.5
    h[1::4, 37] = 150.0
    h[2::4] = torch.randn(h[2::4].shape, generator=g) + 30.0
    h[3::4] = 1.5
    return h


def _quick_gelu(v):
    return v * torch.sigmoid(1.702 * v)


def lnfold_references(h, gamma, beta, W, b, epi, stats=None):
    """-> (x bf16, W' bf16, b', colsum, stats fp32 [M,2], ref1, ref2, bound1), all on the CPU.
    ref1: what the epilogue is to compute, fp64 rstd * (x @ W'^T - mean * colsum) + b' with mean / rstd from the GIVEN
          fp32 statistics; ref2: what it stands in for, fp64 LN(h) @ W^T + b.  QuickGELU on both for epi 8.
    bound1 (derived): the bf16 rounding of the result (half an ulp is at most 2^-8 relative, the bound test_gemm_epilogues
    uses), plus the GEMM test's fp32 accumulation bound (3e-5 of the largest magnitude the accumulator and the mean term
    can reach in the row) scaled by rstd and by the activation's slope (QuickGELU: at most 1.1)."""
    from mmr_amd.clip import fold_layernorm
    d = h.shape[1]
    x = h.bfloat16()
    Wf, bf, c = fold_layernorm(W, b, gamma, beta)
    h64 = h.double()
    if stats is None:
        stats = torch.stack([h64.sum(1), (h64 * h64).sum(1)], dim=1).float()
    s64 = stats.double()
    mean = s64[:, 0] / d
    rstd = 1.0 / torch.sqrt(torch.clamp(s64[:, 1] / d - mean * mean, min=0.0) + EPS)
    acc = x.double() @ Wf.double().t()
    ref1 = rstd[:, None] * (acc - mean[:, None] * c.double()[None, :]) + bf.double()[None, :]
    mu = h64.mean(1, keepdim=True)
    ln = (h64 - mu) / torch.sqrt(((h64 - mu) ** 2).mean(1, keepdim=True) + EPS) * gamma.double() + beta.double()
    ref2 = ln @ W.double().t() + b.double()
    mag = (x.double().abs() @ Wf.double().abs().t() + (mean[:, None] * c.double()[None, :]).abs()).max(dim=1).values
    slope = 1.0
    if epi == 8:
        ref1, ref2, slope = _quick_gelu(ref1), _quick_gelu(ref2), 1.1
    bound1 = 2.0 ** -8 * ref1.abs() + (slope * 3e-5 * rstd * mag)[:, None]
    return x, Wf, bf, c, stats, ref1, ref2, bound1


# measured (MI355X, 2026-10-16) against ref2 = fp64 LN(h) @ W^T + b (QuickGELU applied for epi 8): the largest
# |out - ref2| over a family's rows, in units of the largest |ref2| of those rows, over the 18 (shape, epilogue) cases below:
#   ordinary 4.1e-3, outlier 4.7e-3, constant 3.5e-3, large-mean 3.1e-2.  Each guard is ~3x its family's measurement.
# The large-mean rows pay the fold's documented accuracy price: x = bf16(h) carries an absolute error of
# 2^-9 |mean| per element where LN-then-round carries 2^-9 of a unit-variance value: 7x the ordinary rows' error here.
REF2_GUARD = {"ordinary": 1.2e-2, "outlier": 1.4e-2, "large-mean": 9e-2, "constant": 1e-2}


@pytest.mark.parametrize("M,d,N,tile", [(640, 512, 1536, 128), (5632, 512, 1536, 192), (4096, 512, 2048, 256),
                                        (3840, 768, 2304, 192), (6400, 768, 2304, 256), (3200, 768, 3072, 128),
                                        (2816, 1024, 3072, 192), (2048, 1024, 4096, 256), (1152, 1024, 4096, 128)])
@pytest.mark.parametrize("epi", [7, 8])
def test_lnfold_epilogues(L, device, M, d, N, tile, epi):
    assert _tile(M, N) == tile, "the shape no longer selects the tile this case is here for"
    _check_lnfold(L, device, M, d, N, epi)


def _check_lnfold(L, device, M, d, N, epi):
    g = torch.Generator().manual_seed(M + d + N + epi)
    h = _rows(M, d, g)
    gamma, beta = torch.randn(d, generator=g), torch.randn(d, generator=g)        # as in test_layernorm
    W = (torch.randn(N, d, generator=g) * 0.05).bfloat16().float()
    b = torch.randn(N, generator=g) * 0.1
    x, Wf, bf, c, stats, ref1, ref2, bound1 = lnfold_references(h, gamma, beta, W, b, epi)
    # a constant row normalises to beta, so what the epilogue is to compute there is b' itself (variance exactly 0).
    # bound1 says little about those rows: rstd = 1 / sqrt(eps) = 316 makes its accumulation term about a third of the
    # output's size, so it asserts "finite and near b'" there, and the measured REF2_GUARD below is what pins them.
    bact = _quick_gelu(bf.double()) if epi == 8 else bf.double()
    assert ((ref1[3::4] - bact).abs() <= 0.01 * bound1[3::4]).all()
    slots = torch.zeros(M, NP, 2)
    slots[:, 0] = stats                                              # as emit_fold_inputs writes them
    xd, Wd, bd, cd, sd = x.to(device), Wf.to(device), bf.to(device), c.to(device), slots.to(device)
    out = torch.full((M + 256, N), 7.0, dtype=torch.bfloat16, device=device)
    L.check(_fold(L, device, epi, xd, Wd, bd, out, colsum=cd, stats_in=sd, inv_d=1.0 / d, M=M))
    got = out.float().cpu()
    assert torch.equal(got[M:], torch.full((256, N), 7.0)), "stores past the last output row"
    got = got[:M].double()
    assert torch.isfinite(got).all()
    e1 = ((got - ref1).abs() / bound1)
    line = [f"MEASURED lnfold epi={epi} {M}x{N}x{d}:"]
    worst = {}
    for k, fam in enumerate(FAMILIES):
        r = slice(k, M, 4)
        worst[fam] = (got[r] - ref2[r]).abs().max().item() / ref2[r].abs().max().item()
        line.append(f"{fam}: ref1 {e1[r].max().item():.2f}x bound, ref2 {worst[fam]:.2e};")
    print(" ".join(line))
    for k, fam in enumerate(FAMILIES):
        ex = e1[k::4].max().item()
        assert ex <= 1.0, f"{fam} rows: error against the folded formula is {ex:.2f}x the derived bound"
    for fam in FAMILIES:
        assert worst[fam] <= REF2_GUARD[fam], f"{fam} rows: {worst[fam]:.2e} of max |LN(h) W^T + b| is above the guard {REF2_GUARD[fam]:.1e}"


@pytest.mark.parametrize("M", [512, 3840])       # the 128x128 kernel; a 256-row kernel (its own prologue, 512 threads)
def test_lnfold_consumer_does_not_depend_on_the_slot_layout(L, device, M):
    assert (_tile(M, 2304) == 128) == (M == 512)
    _check_slot_layout(L, device, M, 768, 2304)


def _check_slot_layout(L, device, M, d, N):
    """mmr_common.h: the consumer adds the 16 slots in a fixed order, so results do not depend on the tile width the
    producer ran with.  The same row statistics laid out as the embedding kernels write them (all in slot 0), over 12
    slots (64-column slabs of a 768-wide row) and over 16 (48-column slabs): the rows hold small integers, so every
    partial and every sum of partials is exact in fp32 in any order, and the three outputs must be bit-identical."""
    g = torch.Generator().manual_seed(5)
    h = torch.randint(-8, 9, (M, d), generator=g).float()                  # bf16-representable; |sum| <= 6144, sumsq <= 49152
    gamma, beta = torch.randn(d, generator=g), torch.randn(d, generator=g)
    W = (torch.randn(N, d, generator=g) * 0.05).bfloat16().float()
    b = torch.randn(N, generator=g) * 0.1
    x, Wf, bf, c, stats, ref1, _, bound1 = lnfold_references(h, gamma, beta, W, b, 7)
    layouts = []
    for nslabs in (1, 12, 16):
        part = h.view(M, nslabs, d // nslabs)
        slots = torch.zeros(M, NP, 2)
        slots[:, :nslabs, 0] = part.sum(2)
        slots[:, :nslabs, 1] = (part * part).sum(2)
        assert torch.equal(slots.sum(1), stats)
        layouts.append(slots)
    xd, Wd, bd, cd = x.to(device), Wf.to(device), bf.to(device), c.to(device)
    outs = []
    for slots in layouts:
        sd = slots.to(device)
        out = torch.zeros(M, N, dtype=torch.bfloat16, device=device)
        L.check(_fold(L, device, 7, xd, Wd, bd, out, colsum=cd, stats_in=sd, inv_d=1.0 / d))
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])      # exact
    assert ((outs[0].double() - ref1).abs() / bound1).max().item() <= 1.0       # derived, as in test_lnfold_epilogues


# ------------------------------------------------------------------ every tile width, forced
FORCED = (3840, 768, 2304)          # rows, width, columns: multiples of 256 rows and of 192 / 256 columns, so every width accepts it


@pytest.mark.parametrize("tile", [128, 192, 256])
def test_every_tile_width_forced(device, tile):
    """The checks above on one shape with the GEMM tile width forced (MMR_GEMM_TILE is read once per process, hence a
    child): epi 9 on 3840x768x768 -- 16 zero-padded slots of 48 columns at 192, 12 of 64 otherwise --, epi 7 / 8 and the
    slot-layout check on 3840x2304x768."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(tile)], env={**os.environ, "MMR_GEMM_TILE": str(tile)},
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and f"FORCED_TILE_OK {tile}" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from mmr_amd import _lib
    tile = int(sys.argv[1])
    assert os.environ.get("MMR_GEMM_TILE") == str(tile)
    dev = torch.device("cuda:0")
    M, d, N = FORCED
    _check_resid_stats(_lib, dev, M, d, d, tile)
    for epi in (7, 8):
        _check_lnfold(_lib, dev, M, d, N, epi)
    _check_slot_layout(_lib, dev, M, d, N)
    print(f"FORCED_TILE_OK {tile}")
