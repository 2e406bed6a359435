"""mmr_cosine_topk_split through the C ABI with every source of the gallery norm bound.

GalleryIndex always hands the split search a measured device bound; a C caller may give none, a device scalar, a host
number or both.  include/mmr.h promises the same idx / score / dot64 / status as mmr_cosine_topk_ex(..., MMR_F32, ...) in
every case.  The fixture makes all three tiers matter: un-normalised rows (norms 0.5 .. 3.5), queries whose 40 near
neighbours step down by 1e-4 (the bf16 tier cannot certify them, the three-product tier can), queries whose 40 near neighbours
step down by 1e-6 (closer than the bf16 scan's rounding: only the exhaustive tier is exact) and one query with 41 exact
duplicates.  Shapes include Q on both sides of the fp32 and bf16 plans' query chunk (64 / 128 at E = 768, 128 / 256 at
E = 512), where the two plans lay the shared workspace out differently."""
import numpy as np
import pytest
import torch

from mmr_amd import synth

pytestmark = pytest.mark.gpu

K = 10


def _ladder(gal, q, qis, step, first_row, seed):
    """For each query qi: 40 unit rows at cosine 0.9, 0.9 - step, ... to the query, in 40 different tiles.  The query is made
    bf16-exact (and unit up to bf16 rounding), so the bf16 tier's scores of the 40 rows carry no common offset, only the
    rows' own rounding: with step below that rounding their order is scrambled in both directions."""
    N, E = gal.shape
    stride = (N - 200) // 40
    w = synth.synth_unit_rows(40, E, seed=seed).double()
    c = 0.9 - step * torch.arange(40, dtype=torch.float64)
    for j, qi in enumerate(qis):
        u = (q[qi] / q[qi].norm()).bfloat16().double()
        q[qi] = u.float()
        u /= u.norm()
        wj = w - (w @ u).unsqueeze(1) * u
        wj /= wj.norm(dim=1, keepdim=True)
        rows = [first_row + 7 * j + stride * t for t in range(40)]
        gal[rows] = (c.unsqueeze(1) * u + (1 - c * c).sqrt().unsqueeze(1) * wj).float()


def _fixture(N, E, Q, seed):
    g = torch.Generator().manual_seed(seed)
    gal = synth.synth_unit_rows(N, E, seed=seed) * (0.5 + 3.0 * torch.rand(N, 1, generator=g))
    q = synth.synth_unit_rows(Q, E, seed=seed + 1)
    _ladder(gal, q, sorted({0, Q // 2, Q - 3}), 1e-4, 100, seed + 2)          # second tier
    _ladder(gal, q, [2, 4, Q // 4, Q - 1], 1e-6, 50, seed + 3)                # exhaustive tier (and the sensitivity guard)
    stride = (N - 200) // 40
    gal[[190 + stride * t for t in range(40)]] = gal[7].clone()               # 41 exact copies of row 7
    q[1] = gal[7].clone()
    return gal, q


def _split(L, lib, gd, st):
    N, E = gd.shape
    hi = torch.empty(N, E, dtype=torch.bfloat16, device=gd.device)
    lo = torch.empty_like(hi)
    resid = torch.empty(1, dtype=torch.float32, device=gd.device)
    lib.check(L.mmr_gallery_split_bf16(gd.data_ptr(), N, E, hi.data_ptr(), lo.data_ptr(), resid.data_ptr(), st))
    return hi, lo, resid


def _outputs(Q, device):
    return (torch.empty(Q, K, dtype=torch.int32, device=device), torch.empty(Q, K, dtype=torch.float32, device=device),
            torch.empty(Q, K, dtype=torch.float64, device=device), torch.empty(Q, dtype=torch.int32, device=device))


def _run(device, N, E, Q, seed, guard):
    from mmr_amd import _lib, search
    from oracle import search_ref
    L = _lib.lib()
    st = _lib.stream_ptr(device)
    gal, q = _fixture(N, E, Q, seed)
    gd, qd = gal.to(device), q.to(device)
    hi, lo, resid = _split(L, _lib, gd, st)
    ws = torch.empty(L.mmr_search_workspace_bytes(N, E, Q, K), dtype=torch.uint8, device=device)

    def split_call(host, dev, resid_ptr):
        idx, score, d64, status = _outputs(Q, device)
        _lib.check(L.mmr_cosine_topk_split(qd.data_ptr(), gd.data_ptr(), hi.data_ptr(), lo.data_ptr(), resid_ptr, Q, N, E, K,
                                           100.0, host, _lib.ptr(dev), idx.data_ptr(), score.data_ptr(), d64.data_ptr(),
                                           status.data_ptr(), ws.data_ptr(), ws.numel(), st))
        return [t.cpu() for t in (idx, score, d64, status)]

    # the header's promise: the unsplit fp32 search (no bound: measured in the call)
    idx, score, d64, status = _outputs(Q, device)
    _lib.check(L.mmr_cosine_topk_ex(qd.data_ptr(), gd.data_ptr(), _lib.MMR_F32, Q, N, E, K, 100.0, 0.0, None, idx.data_ptr(),
                                    score.data_ptr(), d64.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), st))
    want = [t.cpu() for t in (idx, score, d64, status)]
    oi, os_, od = search_ref.cosine_topk(q, gal, K, scale=100.0)
    assert np.array_equal(want[0].numpy(), oi) and np.array_equal(want[2].numpy(), od) and np.array_equal(want[1].numpy(), os_)
    assert int(want[3][1]) == 1 and int(want[3][2]) == 1            # duplicates and the 1e-6 ladder: exhaustive tier
    assert int(want[3][0]) == 0                                       # the 1e-4 ladder: certified by the second tier

    nb = search.gallery_norm_bound(gd)
    honest = float(nb.item())                                         # the measured bound itself: same margins, same status
    sources = {"none": (0.0, None), "none (negative)": (-1.0, None), "device": (0.0, nb), "host": (honest, None),
               "both": (honest, nb)}
    for name, (host, dev) in sources.items():
        got = split_call(host, dev, resid.data_ptr())
        for what, a, b in zip(("idx", "score", "dot64", "status"), got, want):
            assert torch.equal(a, b), (N, E, Q, name, what, (a != b).nonzero()[:8].tolist())

    if guard:
        # Sensitivity guard: the same fixture with a margin that is far too small (bound 1e-3 x the true max row norm, no
        # device bound, no residual bound) must give a WRONG answer for some query -- the 1e-6 ladders lie closer together
        # than the bf16 tier's rounding, so an unsound certificate passes a wrong top-k there.  Without this, a fixture easy
        # enough to be right under any bound would let the comparisons above pass whatever bound the kernels read.
        true_max = gal.norm(dim=1).max().item()
        got = split_call(1e-3 * true_max, None, None)
        assert not (np.array_equal(got[0].numpy(), oi) and np.array_equal(got[2].numpy(), od)), \
            "fixture too easy: an understated bound still gave the exact top-k"


@pytest.mark.parametrize("N,E,Q", [(50003, 768, 100), (100000, 512, 200)])
def test_split_topk_every_bound_source(device, N, E, Q):
    _run(device, N, E, Q, seed=11, guard=True)


@pytest.mark.parametrize("N,E,Q", [(50003, 768, 64), (50003, 768, 65), (50003, 768, 128), (50003, 768, 129),
                                   (100000, 512, 128), (100000, 512, 129), (100000, 512, 256), (100000, 512, 257)])
def test_split_topk_every_bound_source_around_query_chunks(device, N, E, Q):
    _run(device, N, E, Q, seed=13, guard=False)


@pytest.mark.slow
def test_split_topk_every_bound_source_1m(device):
    _run(device, 1_000_000, 512, 256, seed=17, guard=True)
