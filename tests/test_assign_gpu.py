"""GPU parity: nearest-centroid assignment (cosine_assign / GalleryIndex.assign / mmr_cosine_assign) against the
brute-force fp64 oracle of tests/assign_helpers.py.  Labels are compared exactly, best64 bit for bit."""
import functools

import numpy as np
import pytest
import torch

import assign_helpers as A

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def S(device):
    from mmr_amd import search
    return search


@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


def _raw_assign(device, g, c, bias, amb_cap, fill=0xFF, mask_words=None, want_best=True):
    """mmr_cosine_assign through the C ABI with labels pre-filled with -7 and best64, counts and the workspace with `fill`
    bytes.  -> (labels int32 [N], best64 fp64 [N] or None, counts int64 [2]) device tensors"""
    from mmr_amd import _lib
    L = _lib.lib()
    N, E = g.shape
    K = c.shape[0]
    need = L.mmr_assign_workspace_bytes(N, E, K, amb_cap, _lib.dtype_code(g.dtype))
    assert need > 0
    ws = torch.full((need,), fill, dtype=torch.uint8, device=device)
    labels = torch.full((max(N, 1),), -7, dtype=torch.int32, device=device)
    best = torch.full((max(N, 1) * 8,), fill, dtype=torch.uint8, device=device).view(torch.float64) if want_best else None
    counts = torch.full((16,), fill, dtype=torch.uint8, device=device).view(torch.int64)
    bias_dev = None if bias is None else torch.from_numpy(np.ascontiguousarray(bias, dtype=np.float64)).to(device)
    _lib.check(L.mmr_cosine_assign(g.data_ptr(), c.data_ptr(), _lib.dtype_code(g.dtype), N, K, E, _lib.ptr(bias_dev), 0.0, None,
                                   _lib.ptr(mask_words), amb_cap, labels.data_ptr(), _lib.ptr(best), counts.data_ptr(),
                                   ws.data_ptr(), need, _lib.stream_ptr(device)))
    torch.cuda.synchronize(device)
    return labels[:N], (None if best is None else best[:N]), counts


def _assert_exact(labels, best, want_labels, want_best):
    got = labels.cpu().numpy()
    assert not (got == -7).any(), "an element of labels was not written"
    if not np.array_equal(got, want_labels):
        bad = np.flatnonzero(got != want_labels)
        raise AssertionError(f"{bad.size} labels differ from the oracle; first rows {bad[:8]}: got {got[bad[:8]]}, want {want_labels[bad[:8]]}")
    if best is not None:
        gb = best.cpu().numpy()
        assert np.array_equal(np.isnan(gb), want_labels < 0), "best64 is NaN exactly where the label is -1"
        ok = want_labels >= 0
        assert np.array_equal(gb[ok].view(np.int64), want_best[ok].view(np.int64)), "best64 bits differ"


@functools.lru_cache(maxsize=None)
def _parity_case(ref, E, K, N, dtype, euclid):
    """(gallery, centroids, bias or None, oracle labels, oracle best64), computed once"""
    g, c = A.parity_fixture(E, K, N, dtype)
    gf, cf = A.f32(g), A.f32(c)
    bias = A.euclid_bias(cf) if euclid else None
    labels, best, _ = A.oracle_assign(ref, gf, cf, bias)
    return g, c, bias, labels, best


# ------------------------------------------------------------------ 1. parity, all rows
@pytest.mark.parametrize("euclid", [False, True], ids=["nobias", "euclid"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("E,K,N", A.PARITY_SHAPES)
def test_parity(ref, device, E, K, N, dtype, euclid):
    g, c, bias, want_labels, want_best = _parity_case(ref, E, K, N, dtype, euclid)
    labels, best, counts = _raw_assign(device, g.to(device), c.to(device), bias, amb_cap=N)
    _assert_exact(labels, best, want_labels, want_best)
    done, amb = counts[:2].tolist()
    assert 0 <= done == amb <= N
    assert (want_labels >= 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_python_front_ends_agree_with_the_oracle(S, ref, device, dtype):
    E, K, N = 128, 300, 4099
    g, c, bias, want_labels, want_best = _parity_case(ref, E, K, N, dtype, True)
    gd = g.to(device)
    labels, best = S.cosine_assign(gd, c.to(device), torch.from_numpy(bias), return_score=True)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (N,) and best.dtype == torch.float64
    _assert_exact(labels, best, want_labels, want_best)
    index = S.GalleryIndex(gd)
    _assert_exact(index.assign(c, torch.from_numpy(bias).to(device)), None, want_labels, want_best)
    only = S.cosine_assign(gd, c.to(device), torch.from_numpy(bias))
    assert isinstance(only, torch.Tensor) and torch.equal(only, labels)


# ------------------------------------------------------------------ 2. the share of rows left to the exact recheck
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_few_rows_are_ambiguous(S, device, dtype):
    """A kernel that sent every row to the recheck would pass parity.  The margin leaves 0.2-1.3 % of these fixtures'
    rows undecided (test_assign_host computes it on the CPU); the per-wave maximum of the margins and the merge's outward
    roundings add a little."""
    for E, K, N in A.PARITY_SHAPES:
        if K == 1:
            continue
        g, c = A.parity_fixture(E, K, N, dtype)
        cf = A.f32(c)
        for bias in (None, torch.from_numpy(A.euclid_bias(cf))):
            _, (done, amb) = S.cosine_assign(g.to(device), c.to(device), bias, return_counts=True)
            print(f"E={E} K={K} N={N} {dtype} bias={'none' if bias is None else 'euclid'}: {amb} ambiguous rows of {N}")
            assert done == amb <= 0.03 * N, (E, K, N, amb)


# ------------------------------------------------------------------ 3. last-bit twins
TWINS = [(3, 10), (5, 40), (7, 260), (31, 32), (250, 299), (64, 255), (100, 256), (0, 288)]   # (a, b), a < b, K = 300 at
# E = 128 (256 centroids per pass, 32 per wave): same wave, other wave, other pass, neighbouring waves, ...


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_last_bit_twins(ref, device, dtype):
    """Centroid b copies centroid a (a < b); planted row i is centroid a_i itself, so a and b lead the row and tie."""
    E, K, N = 128, 300, 1000
    g, c = A.parity_fixture(E, K, N, dtype)
    g, c = g.clone(), c.clone()
    rows = [17 + 97 * i for i in range(len(TWINS))]
    for (a, b), r in zip(TWINS, rows):
        c[b] = c[a]
        g[r] = c[a]
    gf, cf = A.f32(g), A.f32(c)
    d = np.array([A.exact_score(ref, gf[r], cf[a], None) for (a, b), r in zip(TWINS, rows)])
    assert (d > 0.9).all()
    gd, cd = g.to(device), c.to(device)
    for case in ("equal", "up", "down"):
        bias = np.zeros(K, dtype=np.float64)
        for (a, b), di in zip(TWINS, d):
            if case != "equal":
                bias[b] = np.nextafter(di, np.inf if case == "up" else -np.inf) - di       # exact: one ulp of the score
                assert di + bias[b] == np.nextafter(di, np.inf if case == "up" else -np.inf)
        want_labels, want_best, _ = A.oracle_assign(ref, gf, cf, bias)
        labels, best, _ = _raw_assign(device, gd, cd, bias, amb_cap=N)
        got = labels.cpu().numpy()
        for (a, b), r in zip(TWINS, rows):
            assert got[r] == (b if case == "up" else a), (case, a, b, r, got[r])
        _assert_exact(labels, best, want_labels, want_best)


# ------------------------------------------------------------------ 4. the cap protocol
def test_cap_protocol(S, ref, device):
    E, K, N = 128, 20, 1000
    g, c = A.parity_fixture(E, K, N, torch.bfloat16)
    c2 = torch.cat([c, c]).contiguous()                      # every centroid twice: every row is ambiguous
    want_labels, want_best, _ = A.oracle_assign(ref, A.f32(g), A.f32(c2))
    assert (want_labels < K).all()                           # ties go to the lower copy
    gd, cd = g.to(device), c2.to(device)
    labels, _, counts = _raw_assign(device, gd, cd, None, amb_cap=16, want_best=False)
    done, amb = counts[:2].tolist()
    assert amb == N > 16 and done == 16                      # INCOMPLETE: the counter kept counting, the stores stopped
    got = labels.cpu().numpy()
    assert ((got == -1) | (got == want_labels)).all() and (got == -1).sum() == N - 16
    labels, best, (done, amb) = S.cosine_assign(gd, cd, return_score=True, amb_cap=16, return_counts=True)   # retries once
    assert done == amb == N
    _assert_exact(labels, best, want_labels, want_best)
    with pytest.raises(MemoryError):
        S.cosine_assign(gd, cd, amb_cap=16, max_ambiguous=100)


# ------------------------------------------------------------------ 5. masks and edges
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_row_mask_and_deleted_rows(S, ref, device, dtype):
    E, K, N = 128, 33, 1000
    g, c, _, want_labels, _ = _parity_case(ref, E, K, N, dtype, False)
    gd, cd = g.to(device), c.to(device)
    keep = torch.rand(N, generator=torch.Generator().manual_seed(1)) < 0.6
    keep[64:160] = False                                     # whole tiles without a live row
    want = np.where(keep.numpy(), want_labels, -1).astype(np.int32)
    _assert_exact(S.cosine_assign(gd, cd, row_mask=keep.to(device)), None, want, None)
    from mmr_amd import search
    words = search._pack_row_mask(keep.to(device), None, N)
    labels, best, _ = _raw_assign(device, gd, cd, None, amb_cap=N, mask_words=words)
    _assert_exact(labels, None, want, None)
    assert np.array_equal(np.isnan(best.cpu().numpy()), want < 0)
    index = S.GalleryIndex(gd)
    index.delete_rows(torch.nonzero(~keep).reshape(-1))
    _assert_exact(index.assign(cd), None, want, None)
    extra = torch.ones(N, dtype=torch.bool)
    extra[:500] = False                                      # a call's own mask is AND-ed with the deletions
    want = np.where((keep & extra).numpy(), want_labels, -1).astype(np.int32)
    _assert_exact(index.assign(cd, row_mask=extra.to(device)), None, want, None)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_non_finite_values_and_extreme_scales(S, ref, device, dtype):
    E, K, N = 128, 33, 1000
    g, c = A.parity_fixture(E, K, N, dtype)

    def check(g, c, bias=None):
        want_labels, want_best, _ = A.oracle_assign(ref, A.f32(g), A.f32(c), bias)
        labels, best, _ = _raw_assign(device, g.to(device), c.to(device), bias, amb_cap=N)
        _assert_exact(labels, best, want_labels, want_best)
        return want_labels

    # a NaN row gets -1, its neighbours their labels
    g1 = g.clone()
    g1[5, 3] = float("nan")
    g1[600] = float("nan")
    w = check(g1, c)
    assert w[5] == -1 and w[600] == -1 and (np.delete(w, [5, 600]) >= 0).all()
    # a NaN centroid never wins
    c1 = c.clone()
    c1[4, 100] = float("nan")
    w = check(g, c1)
    assert (w != 4).all() and (w >= 0).all()
    # an all-zero centroid set: every score ties at 0, the lowest centroid wins
    w = check(g, torch.zeros(5, E, dtype=dtype))
    assert (w == 0).all()
    # a centroid far out of scale: large (2^14 in fp16, 2^100 in bf16) and, in bf16, wild (2^128: |c| G past FLT_MAX)
    for e in ([14] if dtype == torch.float16 else [100, 128]):
        c2 = c.clone()
        c2[7] = (c[7].float() * 2.0 ** (e // 2) * 2.0 ** (e - e // 2)).to(dtype)
        assert torch.isfinite(c2[7].float()).all() and float(c2[7].float().abs().max()) > 2.0 ** (e - 4)
        w = check(g, c2)
        assert (w == 7).sum() > 100                          # it wins wherever its dot is positive
        check(g, c2, A.euclid_bias(A.f32(c2)))
    # +-inf entries are numbers
    g3 = g.clone()
    g3[10, 0] = float("inf")
    g3[11, 1] = float("-inf")
    g3[12, 2] = float("inf")
    g3[12, 3] = float("-inf")
    check(g3, c)
    c3 = c.clone()
    c3[2, 9] = float("inf")
    check(g, c3)


def test_an_fp32_gallery_is_refused(S, device):
    g = A.unit_rows(100, 128, 3).to(device)
    c = A.unit_rows(4, 128, 4).to(device)
    with pytest.raises(ValueError, match="fp32 galleries are not supported"):
        S.cosine_assign(g, c)
    with pytest.raises(ValueError, match="fp32 galleries are not supported"):
        S.GalleryIndex(g).assign(c)
    from mmr_amd import _lib
    L = _lib.lib()
    rc = L.mmr_cosine_assign(g.data_ptr(), c.data_ptr(), _lib.MMR_F32, 100, 4, 128, None, 0.0, None, None, 8, 256, None, 256, 256,
                             1 << 30, 0)
    assert rc == -95 and b"fp32 galleries are not supported" in L.mmr_last_error()
