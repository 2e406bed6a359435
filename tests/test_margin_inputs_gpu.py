"""The quantities the certificates' margins are built from, measured directly: mmr_gallery_norm_bound (G) and
mmr_gallery_split_bf16 (hi, lo and R = max_row |g - hi|).

A margin is sound only if G and R are upper bounds, and tight only if they are not far above; both are pinned here
against margin_helpers.exact_norm2 (exact sums of squares) on squares, where the comparison is exact in fp64:
    G^2 >= exact   and   G <= sqrt(exact) * up * (1 + 2^-22)
with ``up`` the constant of the kernel's norm_upper_f32 call and 2^-22 for its two fp32 roundings.  One row carries the
maximum (every other row at most half of it), and it is planted wherever the measuring kernels' loops change trips: their
grid is 4096 workgroups of 4 rows, so rows from 16384 are a second stride pass and rows from 32768 a third; the 16-byte
chunk loop of a row takes a second trip for the elements from 512.  A kernel that skips a pass, a trip or a tail row
returns half the bound or less."""
import numpy as np
import pytest
import torch

import margin_helpers as M

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
ES = [8, 72, 128, 256, 512, 520, 768, 1024]
NS = [1, 5, 16385, 16387, 40001]
PASS = 16384                         # rows one stride pass of the 4096 x 4 grid covers
UP_G = float(np.float32(1.000001))   # rownorm_max_kernel
UP_R = float(np.float32(1.00001))    # split_resid_max_kernel


@pytest.fixture(scope="module")
def L(device):
    from mmr_amd import _lib
    return _lib


def _code(L, dtype):
    return {torch.float32: L.MMR_F32, torch.bfloat16: L.MMR_BF16, torch.float16: L.MMR_F16}[dtype]


def _norm_bound(L, gal, device):
    out = torch.full((1,), -1.0, dtype=torch.float32, device=device)
    N, E = gal.shape
    L.check(L.lib().mmr_gallery_norm_bound(gal.data_ptr(), _code(L, gal.dtype), N, E, out.data_ptr(), L.stream_ptr(device)))
    return float(out.item())


def _positions(N):
    """row 0, row N - 1, the last row of the first pass, the first row of the second and of the third pass, and the last
    row of the last full group of four (the last wave a workgroup runs whole)"""
    want = [0, N - 1, PASS - 1, PASS, 2 * PASS - 1, 2 * PASS, (N // 4) * 4 - 1]
    return sorted({r for r in want if 0 <= r < N})


def _masses(E):
    out = [("whole row", slice(0, E)), ("last 8", slice(E - 8, E))]
    if E >= 520:
        out.append(("[512, 520)", slice(512, 520)))
    return out


def _pin(got, exact, up, what):
    assert got * got >= exact, f"{what}: bound {got!r} is below the true maximum {np.sqrt(exact)!r}"
    assert got <= np.sqrt(exact) * up * (1 + 2.0 ** -22), f"{what}: bound {got!r} is above {np.sqrt(exact)!r} * up"


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_bound_is_the_maximum_wherever_it_sits(L, device, dtype, E):
    gen = torch.Generator().manual_seed(E)
    # elements in [1, 2): random mantissas of the dtype, every sum of squares different
    mass = (1 + torch.rand(E, generator=gen)).to(dtype)
    dgen = torch.Generator(device=device).manual_seed(E)
    for N in NS:
        # every other row at most half the planted one's norm in its smallest form (8 elements >= 1: norm >= 2.83)
        base = ((2 * torch.rand(N, E, device=device, generator=dgen) - 1) * (1.2 / E ** 0.5)).to(dtype)
        assert float(base.float().square().sum(1).max()) <= 1.41 ** 2
        for where, sl in _masses(E):
            row = torch.zeros(E, dtype=dtype)
            row[sl] = mass[sl]
            exact = float(M.exact_norm2(row[None, :])[0])
            assert exact >= 8.0
            for r in _positions(N):
                keep = base[r].clone()
                base[r] = row.to(device)
                got = _norm_bound(L, base, device)
                base[r] = keep
                _pin(got, exact, UP_G, f"{dtype} N={N} E={E} row {r} mass {where}")


def test_norm_bound_documented_cases_of_norm_upper_f32(L, device):
    for dtype in DTYPES:
        assert _norm_bound(L, torch.zeros(37, 72, dtype=dtype, device=device), device) == 0.0
    for dtype in (torch.bfloat16, torch.float32):
        # a norm too small for fp32 arithmetic is overstated, not rounded towards zero: exactly 2^-100
        tiny = torch.full((37, 72), 2.0 ** -120, dtype=dtype, device=device)
        tiny[::2] = -tiny[::2]
        assert _norm_bound(L, tiny, device) == 2.0 ** -100
        # a finite row whose sum of squares passes FLT_MAX
        big = torch.zeros(37, 72, dtype=dtype, device=device)
        big[35, 64:] = 2.0 ** 64                                     # 8 * 2^128
        assert _norm_bound(L, big, device) == float("inf")
        big[35, 65:] = 0                                             # 2^128 alone is past FLT_MAX too
        assert _norm_bound(L, big, device) == float("inf")
        big[35, 64] = 2.0 ** 63                                      # 2^126: finite
        _pin(_norm_bound(L, big, device), 2.0 ** 126, UP_G, "2^63")


def _split(L, g, device, want_resid=True):
    N, E = g.shape
    hi = torch.full((N, E), 0x7fc1, dtype=torch.int16, device=device).view(torch.bfloat16)
    lo = hi.clone()
    resid = torch.full((1,), -1.0, dtype=torch.float32, device=device)
    L.check(L.lib().mmr_gallery_split_bf16(g.data_ptr(), N, E, hi.data_ptr(), lo.data_ptr(),
                                           resid.data_ptr() if want_resid else None, L.stream_ptr(device)))
    return hi, lo, float(resid.item())


def _bits(x):
    return x.contiguous().view(torch.int16)


def _special_values():
    """fp32 bit patterns where a rounding to bf16 goes wrong first"""
    u = [0x00000000, 0x80000000,                                     # +-0
         0x00000001, 0x80000001, 0x00007fff, 0x00008000, 0x00008001, 0x00018000, 0x007fffff, 0x807fffff,   # subnormals
         0x00800000, 0x00ffffff,                                     # smallest normals
         0x3f7fffff, 0xbf7fffff, 0x3fffffff, 0x40ffc000,             # round up into the next binade
         0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,             # exact ties: to even (down, then up)
         0x3f808001, 0x3f807fff, 0x3f80ffff, 0x3f810000,             # either side of a tie
         0x7f7f0000, 0xff7f0000, 0x7f7f7fff, 0x7f7e8000, 0x7f7e8001, # the largest finite values that stay finite
         0x7f7f8000, 0x7f7fffff, 0xff7fffff]                         # ... and those that round to infinity
    return torch.tensor(np.array(u, dtype=np.uint32).view(np.int32)).view(torch.float32)


@pytest.mark.parametrize("E", [8, 72, 512, 768])
def test_split_is_its_definition_bit_for_bit(L, device, E):
    N = 33001
    assert (N * (E // 8)) % 256 != 0                                 # the last 256-thread block is partly empty
    gen = torch.Generator().manual_seed(100 + E)
    g = torch.randn(N, E, generator=gen) * torch.exp2(torch.randint(-20, 20, (N, 1), generator=gen).float())
    sp = _special_values()
    flat = g.view(-1)
    flat[:sp.numel()] = sp                                           # the first elements ...
    flat[-sp.numel():] = sp.flip(0)                                  # ... and the last, in the partly empty block
    mid = (N // 2) * E + 3
    flat[mid:mid + sp.numel()] = sp
    hi, lo, _ = _split(L, g.to(device), device, want_resid=False)
    want_hi = g.bfloat16()
    want_lo = (g - want_hi.float()).bfloat16()                       # -inf where a finite value's hi is +inf
    assert not bool(want_lo.isnan().any()) and bool(want_hi.isinf().any()) and bool(want_lo.isinf().any())
    assert torch.equal(_bits(hi.cpu()), _bits(want_hi)), "hi != bf16(x)"
    assert torch.equal(_bits(lo.cpu()), _bits(want_lo)), "lo != bf16(x - hi)"


@pytest.mark.parametrize("E", [8, 72, 512, 768])
def test_split_residual_bound_is_the_maximum_wherever_it_sits(L, device, E):
    N = 33001
    gen = torch.Generator().manual_seed(200 + E)
    # background: |x| < 2^-5, so a residual is at most 2^-14 per element: under 1.7e-3 per row
    base = ((2 * torch.rand(N, E, generator=gen) - 1) * 2.0 ** -5).to(device)
    # the longest row is bf16-exact (residual 0) and is never the row with the largest residual
    longest = N // 3
    base[longest] = 4.0
    # the planted row: v + 0.3 .. 0.49 ulp, v in [1, 2) bf16-exact: residuals 2.3e-3 .. 3.8e-3 per element, exact in fp32
    v = (1 + torch.rand(E, generator=gen)).bfloat16().float()
    full = v + (0.3 + 0.19 * torch.rand(E, generator=gen)) * 2.0 ** -7
    assert torch.equal(full.bfloat16().float(), v)
    for where, sl in _masses(E):
        row = torch.zeros(E)
        row[sl] = full[sl]
        exact = float(M.exact_norm2((row - row.bfloat16().float())[None, :])[0])
        assert exact >= 8 * (0.3 * 2.0 ** -7) ** 2 > 4 * E * 2.0 ** -28
        for r in _positions(N):
            assert r != longest
            keep = base[r].clone()
            base[r] = row.to(device)
            hi, lo, got = _split(L, base, device)
            base[r] = keep
            _pin(got, exact, UP_R, f"N={N} E={E} row {r} mass {where}")
            assert torch.equal(_bits(hi[r].cpu()), _bits(row.bfloat16()))
            assert torch.equal(_bits(lo[r].cpu()), _bits((row - row.bfloat16().float()).bfloat16()))
    assert _norm_bound(L, base, device) >= 4.0 * E ** 0.5
