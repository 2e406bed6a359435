"""GPU: k-means++ seeding (cluster.kmeans_plusplus / mmr_kmeanspp_seed) EQUALS the restatement of its definition in
tests/kmeanspp_helpers.py -- indices, potentials, shift and centers, through the Python call and through the raw C call --
and seeds kmeans, select_k and reference_vector_by_clustering.  test_kmeanspp_host holds the restatement itself."""
import functools
import math

import numpy as np
import pytest
import torch

import kmeanspp_helpers as H

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ["bf16", "fp16"]
METRICS = ["euclidean", "cosine"]


@pytest.fixture(scope="module")
def C(device):
    from mmr_amd import cluster
    return cluster


def _norm_bound(gd) -> float:
    from mmr_amd import search
    return float(search.gallery_norm_bound(gd))


def _raw_seed(device, gd, K, L, metric, variates, mask=None, nb=0.0, nb_dev=None, poison=0xFF):
    """mmr_kmeanspp_seed through the C ABI with every output and the workspace poisoned (`poison`: a byte, or "nan": fp64 NaN
    bit patterns).  -> (centers, indices int64, potentials, shift) on the host side of the comparison"""
    from mmr_amd import _lib, search
    lib = _lib.lib()
    N, E = gd.shape
    need = lib.mmr_kmeanspp_workspace_bytes(N, E, K, L)
    assert need > 0

    def poisoned(nbytes):
        n8 = (nbytes + 7) // 8 * 8
        if poison == "nan":
            return torch.full((n8 // 8,), float("nan"), dtype=torch.float64, device=device).view(torch.uint8)
        return torch.full((n8,), poison, dtype=torch.uint8, device=device)

    ws = poisoned(need)
    indices = poisoned(4 * K).view(torch.int32)
    potentials = poisoned(8 * K).view(torch.int64)
    shift = poisoned(8).view(torch.int32)
    centers = poisoned(2 * K * E).view(gd.dtype)
    var_dev = torch.from_numpy(np.ascontiguousarray(variates, dtype=np.int64)).to(device)
    words = None if mask is None else search._pack_row_mask(torch.from_numpy(mask).to(device), None, N)
    _lib.check(lib.mmr_kmeanspp_seed(gd.data_ptr(), _lib.dtype_code(gd.dtype), N, E, K, L, H.METRICS[metric], _lib.ptr(words),
                                     var_dev.data_ptr(), nb, _lib.ptr(nb_dev), indices.data_ptr(), potentials.data_ptr(),
                                     shift.data_ptr(), centers.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(device)))
    torch.cuda.synchronize(device)
    return centers[:K * E].view(K, E), indices[:K].to(torch.int64), potentials[:K], int(shift[0])


def _assert_equals(got, want: H.Restated, gallery, what=""):
    centers, indices, potentials, shift = got
    gi, gp = indices.cpu().numpy(), potentials.cpu().numpy()
    assert shift == want.shift, (what, shift, want.shift)
    assert np.array_equal(gi, want.indices), (what, gi, want.indices)
    assert np.array_equal(gp, want.potentials), (what, gp, want.potentials)
    assert torch.equal(centers.cpu().view(torch.int16), gallery[torch.from_numpy(want.indices)].view(torch.int16)), what


@functools.lru_cache(maxsize=None)
def _restated(case_key, G):
    case = _CASES[case_key]
    return H.restate(case.g32, case.K, case.L, case.variates, G, case.metric, case.mask)


_CASES = {}


def _case(case):
    _CASES.setdefault(case.name, case)
    return _CASES[case.name]


def _public(C, case, gd, device, **kw):
    mask = None if case.mask is None else torch.from_numpy(case.mask).to(device)
    return C.kmeans_plusplus(gd, case.K, metric=case.metric, row_mask=mask, variates=torch.from_numpy(case.variates),
                             n_local_trials=case.L, return_potentials=True, **kw)


# ------------------------------------------------------------------ 1. parity
# every shape x dtype x metric, without a mask and with parity_mask -- except (128, 1, 1), whose one row cannot be cleared
PARITY = [(E, K, N, dtype, metric, masked) for E, K, N in H.PARITY_SHAPES for dtype in DTYPES for metric in METRICS
          for masked in (False, True) if not (masked and N - 2 < K)]


@pytest.mark.parametrize("E,K,N,dtype,metric,masked", PARITY,
                         ids=[f"{E}-{K}-{N}-{DTYPE_IDS[DTYPES.index(d)]}-{m}-{'masked' if k else 'all'}" for E, K, N, d, m, k in PARITY])
def test_parity_with_the_restatement(C, device, E, K, N, dtype, metric, masked):
    case = _case(H.parity_case(E, K, N, dtype, metric, masked))
    gd = case.gallery.to(device)
    G = _norm_bound(gd)
    shift, dmax = H.scale_of(G, metric)
    assert shift == 37 - math.frexp(dmax)[1] + 1 == 37 - int(math.floor(math.log2(dmax)))
    want = _restated(case.name, G)
    _assert_equals(_public(C, case, gd, device), want, case.gallery, "kmeans_plusplus")
    _assert_equals(_raw_seed(device, gd, K, case.L, metric, case.variates, case.mask), want, case.gallery, "mmr_kmeanspp_seed")
    assert len(set(want.indices.tolist())) == K


def test_every_row_is_chosen_when_k_is_n(C, device):
    case = _case(H.parity_case(128, 31, 31, torch.bfloat16, "euclidean", False))
    gd = case.gallery.to(device)
    want = _restated(case.name, _norm_bound(gd))
    got = _public(C, case, gd, device)
    _assert_equals(got, want, case.gallery)
    assert sorted(got[1].tolist()) == list(range(31)) and int(got[2][-1]) == 0


# ------------------------------------------------------------------ 2. crafted targets
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_targets_on_the_sampling_blocks_edges(C, device, dtype):
    """b = 0 over leading zero weights, b = 2^53 - 1, and r one below / equal to the prefix sum at the end of the sampling's
    block 0, from the restatement's own prefix sums.  parity_mask clears the rows on both sides of that boundary, so this
    is the FIRST level's boundary with zero weights around it: the draws land on the last live row below the cleared run
    and on the first above it.  The boundary rows themselves are the next test's."""
    B = C.KMEANSPP_BLOCK_ROWS
    assert B == H.BLOCK_ROWS                     # the helpers place their rows by the header's constant
    case = H.crafted_case(dtype)
    gd = case.gallery.to(device)
    var, want = H.crafted_variates(case, _norm_bound(gd))
    assert want.indices[0] == B + 14 and (var[1:, 0] == 0).all() and (var[1:, 1] == 2 ** 53 - 1).all()
    _assert_equals(_raw_seed(device, gd, case.K, case.L, case.metric, var, case.mask), want, case.gallery)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_targets_on_the_last_row_of_a_block_and_the_first_of_the_next(C, device, dtype, metric):
    """An unmasked gallery of two blocks and a short third: the weights around both block boundaries are positive, and
    every trial draws exactly row B - 1, B, 2B - 1 or 2B -- the last thread of a block's scan and the first of the next.
    L = 1: one target a step, so each IS the step's seed.  L = 2: a boundary's two rows a step, one of them the seed, the
    other in the potential (the smaller of the two trials' sums)."""
    B = C.KMEANSPP_BLOCK_ROWS
    assert B == H.BLOCK_ROWS
    for L in (1, 2):
        case = H.edge_case(L, dtype, metric)
        gd = case.gallery.to(device)
        var, want = H.edge_variates(case, _norm_bound(gd))
        last = 2 * B + 187
        if L == 1:
            assert want.cands == [[last], [B - 1], [B], [2 * B - 1], [2 * B]]
            assert want.indices.tolist() == [last, B - 1, B, 2 * B - 1, 2 * B]
        else:
            assert want.cands == [[last], [B - 1, B], [2 * B - 1, 2 * B]]
            assert want.indices[1] in (B - 1, B) and want.indices[2] in (2 * B - 1, 2 * B)
        _assert_equals(_raw_seed(device, gd, case.K, L, metric, var), want, case.gallery, f"L={L}")


# ------------------------------------------------------------------ 3. more seeds than distinct rows
def test_duplicates_then_the_lowest_live_row(C, device):
    case = _case(H.duplicates_case())
    gd = case.gallery.to(device)
    want = _restated(case.name, _norm_bound(gd))
    assert sorted(i % 3 for i in want.indices[:3]) == [0, 1, 2] and want.indices[3:].tolist() == [0, 0]
    _assert_equals(_public(C, case, gd, device), want, case.gallery)
    # the lowest LIVE row: with rows 0 and 1 masked the tail repeats row 2
    mask = np.ones(12, dtype=bool)
    mask[:2] = False
    want = H.restate(case.g32, 5, 16, case.variates, _norm_bound(gd), "euclidean", mask)
    assert want.indices[3:].tolist() == [2, 2]
    _assert_equals(_raw_seed(device, gd, 5, 16, "euclidean", case.variates, mask), want, case.gallery)


def test_an_all_zero_gallery(C, device):
    g = torch.zeros(40, 128, dtype=torch.bfloat16)
    var = H.variates_of(4, 3, 9)
    mask = H.parity_mask(40)
    want = H.restate(g.float().numpy(), 4, 3, var, 0.0, "euclidean", mask)
    assert want.shift == 0 and want.potentials.tolist() == [0] * 4 and want.indices[1:].tolist() == [1, 1, 1]
    _assert_equals(_raw_seed(device, g.to(device), 4, 3, "euclidean", var, mask), want, g)


# ------------------------------------------------------------------ 4. scale
@pytest.mark.parametrize("metric", METRICS)
def test_unscaled_rows_and_a_loose_caller_bound(C, device, metric):
    """Rows of norm 5 to 30: shift is sized from G, so nothing saturates; a caller bound 8 times the true one gives the
    restatement's result for THAT bound"""
    base = H.planted(700, 256, 6, torch.float16)
    scale = torch.linspace(5.0, 30.0, 700)[torch.randperm(700, generator=torch.Generator().manual_seed(3))]
    g = (base.float() * scale[:, None]).to(torch.float16).contiguous()
    g32 = g.float().numpy()
    gd = g.to(device)
    G = _norm_bound(gd)
    assert 29.0 < G < 31.0
    var = H.variates_of(6, 3, 77)
    want = H.restate(g32, 6, 3, var, G, metric)
    assert want.potentials.max() < 700 * H.WMAX and int(want.closest.max()) < H.WMAX
    _assert_equals(_raw_seed(device, gd, 6, 3, metric, var), want, g)
    loose = float(np.float32(8.0 * G))
    want8 = H.restate(g32, 6, 3, var, loose, metric)
    assert want8.shift == want.shift - 6           # 64 times the Dmax, for either metric at G = 30
    _assert_equals(_raw_seed(device, gd, 6, 3, metric, var, nb=loose), want8, g)
    # max(caller's, device scalar): the larger wins whichever side it is on
    dev = torch.tensor([loose], dtype=torch.float32, device=device)
    _assert_equals(_raw_seed(device, gd, 6, 3, metric, var, nb=G, nb_dev=dev), want8, g)


# ------------------------------------------------------------------ 5. repeatability
def test_two_runs_agree_whatever_the_workspace_held(C, device):
    case = _case(H.parity_case(512, 17, 4099, torch.bfloat16, "euclidean", True))
    gd = case.gallery.to(device)
    runs = [_raw_seed(device, gd, case.K, case.L, case.metric, case.variates, case.mask, poison=p) for p in (0xFF, "nan", 0x00, 0xFF)]
    for r in runs[1:]:
        assert r[3] == runs[0][3]
        for a, b in zip(r[:3], runs[0][:3]):
            assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    _assert_equals(runs[1], _restated(case.name, _norm_bound(gd)), case.gallery)


# ------------------------------------------------------------------ 6. trials per step
@pytest.mark.parametrize("L", [1, 16])
def test_one_and_sixteen_trials(C, device, L):
    case = _case(H.parity_case(256, 8, 700, torch.float16, "cosine", True, L=L))
    gd = case.gallery.to(device)
    want = _restated(case.name, _norm_bound(gd))
    _assert_equals(_public(C, case, gd, device), want, case.gallery)


def test_the_default_trials_and_variates(C, device):
    K = 21                                        # 2 + int(ln 21) = 5
    g = H.planted(700, 128, K, torch.bfloat16)
    gd = g.to(device)
    got = C.kmeans_plusplus(gd, K, generator=torch.Generator().manual_seed(123), return_potentials=True)
    want = H.restate(g.float().numpy(), K, 5, H.variates_of(K, 5, 123), _norm_bound(gd))
    _assert_equals(got, want, g)
    centers, indices = C.kmeans_plusplus(gd, K, generator=torch.Generator().manual_seed(123))
    assert indices.dtype == torch.int64 and torch.equal(indices, got[1]) and torch.equal(centers, got[0])
    with pytest.raises(ValueError, match="live rows"):
        C.kmeans_plusplus(gd, K, row_mask=torch.arange(700, device=device) < K - 1)


# ------------------------------------------------------------------ 7. the public paths
def _same_run(a, b):
    return (torch.equal(a.centroids, b.centroids) and torch.equal(a.labels, b.labels) and a.n_iter == b.n_iter
            and a.inertia == b.inertia and a.converged == b.converged)


@pytest.mark.parametrize("metric", METRICS)
def test_kmeans_seeds_with_kmeans_plusplus(C, device, metric):
    g = H.planted(2051, 128, 6, torch.bfloat16).to(device)
    mask = torch.from_numpy(H.parity_mask(2051)).to(device)
    gen = lambda: torch.Generator().manual_seed(2024)
    a = C.kmeans(g, 6, init="k-means++", metric=metric, row_mask=mask, generator=gen(), max_iter=30)
    seeds = C.kmeans_plusplus(g, 6, metric=metric, row_mask=mask, generator=gen())[0]
    b = C.kmeans(g, 6, init=seeds, metric=metric, row_mask=mask, max_iter=30)
    assert _same_run(a, b) and int(a.sizes.sum()) == int(mask.sum())
    with pytest.raises(ValueError, match="init must be"):
        C.kmeans(g, 6, init="kmeans++")


def test_select_k_and_reference_vector_pass_it_through(C, device):
    g = H.planted(700, 128, 3, torch.float16).to(device)
    gen = torch.Generator().manual_seed(7)
    sel = C.select_k(g, (2, 3), init="k-means++", generator=gen, max_iter=30)
    gen2 = torch.Generator().manual_seed(7)
    for k in (2, 3):
        seeds = C.kmeans_plusplus(g, k, generator=gen2)[0]
        assert _same_run(sel.results[k], C.kmeans(g, k, init=seeds, max_iter=30))
    feats = H.planted(40, 128, 2, torch.float16).float().to(device)
    vec, idx = C.reference_vector_by_clustering(feats, 5, init="k-means++", generator=torch.Generator().manual_seed(9), return_indices=True)
    seeds = C.kmeans_plusplus(feats.to(torch.float16), 2, generator=torch.Generator().manual_seed(9))[0]
    vec2, idx2 = C.reference_vector_by_clustering(feats, 5, init=seeds, return_indices=True)
    assert torch.equal(vec, vec2) and torch.equal(idx, idx2)


def test_the_seeding_is_graph_capturable(C, device):
    """One C call, no host read: captured with the norm bound measured inside, replayed on other variates"""
    from mmr_amd import _lib
    case = _case(H.parity_case(256, 8, 700, torch.float16, "cosine", True, L=4))
    gd = case.gallery.to(device)
    G = _norm_bound(gd)
    K, L, N, E = case.K, case.L, 700, 256
    lib = _lib.lib()
    from mmr_amd import search
    words = search._pack_row_mask(torch.from_numpy(case.mask).to(device), None, N)
    ws = torch.empty(lib.mmr_kmeanspp_workspace_bytes(N, E, K, L), dtype=torch.uint8, device=device)
    var = torch.from_numpy(case.variates).to(device)
    indices = torch.zeros(K, dtype=torch.int32, device=device)
    potentials = torch.zeros(K, dtype=torch.int64, device=device)
    shift = torch.zeros(1, dtype=torch.int32, device=device)
    centers = torch.zeros(K, E, dtype=gd.dtype, device=device)

    def call():
        _lib.check(lib.mmr_kmeanspp_seed(gd.data_ptr(), _lib.dtype_code(gd.dtype), N, E, K, L, 1, words.data_ptr(), var.data_ptr(),
                                         0.0, None, indices.data_ptr(), potentials.data_ptr(), shift.data_ptr(), centers.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _lib.stream_ptr(device)))

    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        call()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream(device).wait_stream(side)
    other = H.variates_of(K, L, 555)
    for v in (other, case.variates):
        var.copy_(torch.from_numpy(v))
        for t in (indices, potentials, shift, centers):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize(device)
        want = H.restate(case.g32, K, L, v, G, "cosine", case.mask)
        _assert_equals((centers, indices.to(torch.int64), potentials, int(shift[0])), want, case.gallery)
