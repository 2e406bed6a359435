"""GPU: row-mask filtered search (the *_masked entry points, row_mask=, GalleryIndex.delete_rows / restore_rows / dedup).

The expected result is always the oracle run on the compacted gallery gallery[mask], ids mapped back to the original
rows: idx, score and dot64 bit for bit; for range search and the self-join the same pairs in the same order."""
import numpy as np
import pytest
import torch

from mmr_amd import synth
from search_helpers import assert_topk as _assert_topk, expect_topk as _expect_topk, oracle_join as _oracle_join, \
    oracle_range as _oracle_range, plan_tpt as _plan_tpt, to_np as _np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S(device):
    from mmr_amd import search
    return search


@pytest.fixture(scope="module")
def oracle():
    from oracle import search_ref
    return search_ref


@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


def _masks(N, k, dtype, seed):
    rng = np.random.default_rng(seed)
    tr, tpt = _plan_tpt(N, dtype)
    out = {"random50": rng.random(N) < 0.5, "sparse0.1%": rng.random(N) < 0.001}
    m = rng.random(N) < 0.7
    for t in range(0, (N + tr - 1) // tr, 3):          # every third tile dead
        m[t * tr:(t + 1) * tr] = False
    for task in range(1, (N + tr * tpt - 1) // (tr * tpt), 4):    # every fourth task dead
        m[task * tr * tpt:(task + 1) * tr * tpt] = False
    m[2048:2 * 2048] = False                           # 64 dead 32-row tiles in a row
    out["dead tiles and tasks"] = m
    few = np.zeros(N, bool)
    few[rng.choice(N, k - 3, replace=False)] = True
    out["fewer than k live"] = few
    few10 = np.zeros(N, bool)
    few10[rng.choice(N, 7, replace=False)] = True      # fewer than k = 10 live: the fast path's short result
    out["fewer than 10 live"] = few10
    out["all zeros"] = np.zeros(N, bool)
    return out


@pytest.mark.parametrize("E", [128, 256, 512, 768, 1024])
@pytest.mark.parametrize("dtype,presplit", [(torch.bfloat16, False), (torch.float32, False), (torch.float32, True)])
def test_masked_topk_matrix(S, oracle, device, E, dtype, presplit):
    N = 12007
    g = synth.synth_unit_rows(N, E, seed=E).to(dtype)
    qall = synth.synth_unit_rows(300, E, seed=E + 1).to(dtype)
    gd = g.to(device)
    idx_ = S.GalleryIndex(gd, presplit=presplit)
    for name, mask in _masks(N, 40, dtype, seed=E).items():
        md = torch.from_numpy(mask).to(device)
        for Q, k in (((300, 10),) if name == "random50" else ()) + ((37, 40), (1, 10)):
            q = qall[:Q]
            want = _expect_topk(oracle, q, g, mask, k)
            got = idx_.search(q.to(device), k, return_dot64=True, row_mask=md)
            _assert_topk(got, want)
            if not presplit and Q == 37:
                got2 = S.cosine_topk(q.to(device), gd, k, return_dot64=True, row_mask=md)
                _assert_topk(got2, want)
            if name == "all zeros":
                assert (got[1] == -1).all() and torch.isinf(got[0]).all()


@pytest.mark.parametrize("dtype,presplit", [(torch.bfloat16, False), (torch.float32, False), (torch.float32, True)])
def test_all_ones_mask_is_the_unmasked_call_including_status(S, device, dtype, presplit):
    N, E = 20011, 512
    g = synth.synth_unit_rows(N, E, seed=3).to(dtype).to(device)
    q = synth.synth_unit_rows(300, E, seed=4).to(dtype).to(device)
    q[5] = g[77]                                       # some queries certify, some may not
    idx_ = S.GalleryIndex(g, presplit=presplit)
    a = idx_.search(q, 10, return_dot64=True, return_status=True)
    b = idx_.search(q, 10, return_dot64=True, return_status=True, row_mask=torch.ones(N, dtype=torch.bool, device=device))
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def _words(mask_np, garbage=False):
    """host packing: bit r & 31 of word r >> 5"""
    N = mask_np.size
    nw = (N + 31) // 32
    bits = np.zeros(nw * 32, np.uint64)
    bits[:N] = mask_np
    if garbage:
        bits[N:] = 1                                   # bits at or past N must be ignored
    w = (bits.reshape(nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return torch.from_numpy(w.view(np.int32).copy())


def test_row_mask_pack_matches_host_packing(S, device):
    for N in (1, 31, 32, 33, 50003):
        keep = torch.rand(N, device=device) < 0.5
        and_np = np.random.default_rng(N).random(N) < 0.5
        andw = _words(and_np, garbage=True).to(device)
        got = S._pack_row_mask(keep, andw, N)
        want = _words(keep.cpu().numpy() & and_np)
        assert torch.equal(got.cpu(), want), N
        assert torch.equal(S._pack_row_mask(keep, None, N).cpu(), _words(keep.cpu().numpy())), N


def _topk_c(L, lib, device, q, g, k, words, split=None, status=True):
    Q, E = q.shape
    N = g.shape[0]
    ws = torch.empty(L.mmr_search_workspace_bytes(N, E, Q, k), dtype=torch.uint8, device=device)
    idx = torch.empty(Q, k, dtype=torch.int32, device=device)
    sc = torch.empty(Q, k, dtype=torch.float32, device=device)
    d = torch.empty(Q, k, dtype=torch.float64, device=device)
    st = torch.empty(Q, dtype=torch.int32, device=device)
    s = lib.stream_ptr(device)
    outs = (idx.data_ptr(), sc.data_ptr(), d.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(), s)
    if split is not None:
        lib.check(L.mmr_cosine_topk_split_masked(q.data_ptr(), g.data_ptr(), split[0].data_ptr(), split[1].data_ptr(),
                                                 split[2].data_ptr(), Q, N, E, k, 1.0, 0.0, None, lib.ptr(words), *outs))
    else:
        lib.check(L.mmr_cosine_topk_masked(q.data_ptr(), g.data_ptr(), lib.dtype_code(g.dtype), Q, N, E, k, 1.0, 0.0, None,
                                           lib.ptr(words), *outs))
    return sc, idx.to(torch.int64), d, st


def test_c_abi_garbage_bits_past_n_and_null_mask(S, oracle, device):
    from mmr_amd import _lib as lib
    L = lib.lib()
    N, E, Q, k = 10001, 256, 37, 10                    # 10001 = 312 * 32 + 17: a ragged last word
    g = synth.synth_unit_rows(N, E, seed=8).bfloat16()
    q = synth.synth_unit_rows(Q, E, seed=9).bfloat16()
    mask = np.random.default_rng(1).random(N) < 0.5
    gd, qd = g.to(device), q.to(device)
    got = _topk_c(L, lib, device, qd, gd, k, _words(mask, garbage=True).to(device))
    _assert_topk(got, _expect_topk(oracle, q, g, mask, k))
    # NULL mask: bit-identical to mmr_cosine_topk_ex, status included
    a = _topk_c(L, lib, device, qd, gd, k, None)
    b = S.cosine_topk(qd, gd, k, return_dot64=True, return_status=True)
    for x, y in zip(a, (b[0], b[1], b[2], b[3])):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
    # fp32 split form, NULL mask against mmr_cosine_topk_split through an index without deletions
    gf, qf = g.float().to(device), q.float().to(device)
    ix = S.GalleryIndex(gf, presplit=True)
    a = _topk_c(L, lib, device, qf, gf, k, None, split=ix._split)
    b = ix.search(qf, k, return_dot64=True, return_status=True)
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def test_masked_rows_never_win_and_the_exhaustive_path_applies_the_mask(S, oracle, device):
    """Planted best matches are masked: the query's own copy, and the 60 near-identical rows of
    test_uncertified_queries_fall_back_to_exact (a crowd the certificate cannot separate: those queries take the exhaustive
    path, status 1, which must apply the mask too)."""
    N, E, k = 8192, 512, 10
    gb = synth.synth_unit_rows(N, E, seed=21).bfloat16()
    base = gb[5].clone()
    torch.manual_seed(0)
    crowd = torch.randperm(N)[:60].tolist()
    for j, r in enumerate(crowd):
        v = base.clone()
        v.view(torch.int16)[j] += (j % 5) - 2          # a few bf16 ulps on one component: dot moves by ~1e-5
        gb[r] = v
    qb = synth.synth_unit_rows(8, E, seed=22).bfloat16()
    qb[0] = base
    gb[500] = qb[1]                                    # exact copy of query 1
    mask = np.ones(N, bool)
    mask[crowd[::2]] = False                           # half the crowd masked: 30 live near-ties remain
    mask[[5, 500]] = False
    gd = gb.to(device)
    md = torch.from_numpy(mask).to(device)
    got = S.cosine_topk(qb.to(device), gd, k, return_dot64=True, return_status=True, row_mask=md)
    _assert_topk(got, _expect_topk(oracle, qb, gb, mask, k))
    dead = set(np.flatnonzero(~mask).tolist())
    assert not dead & set(got[1].cpu().numpy().ravel().tolist())
    assert int(got[3][0]) == 1, "the crowded query should take the exhaustive path"
    # k > 26: every query goes exhaustive
    got = S.cosine_topk(qb.to(device), gd, 40, return_dot64=True, row_mask=md)
    _assert_topk(got, _expect_topk(oracle, qb, gb, mask, 40))


def _ladder(gal, q, qis, step, first_row, seed):
    """For each query qi: 40 unit rows at cosine 0.9, 0.9 - step, ... to the (bf16-exact) query, in 40 different tiles
    (test_search_split_abi_gpu.py's construction): step 1e-4 needs the three-product tier, 1e-6 the exhaustive one."""
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


def test_fp32_split_index_tiers_under_a_mask(S, oracle, device):
    """Queries that need tier 2 (the three-product scan) and tier 3 (exhaustive) of the pre-split fp32 index, with a
    mask that removes half of each ladder."""
    N, E, Q, k = 20000, 256, 8, 10
    g = synth.synth_unit_rows(N, E, seed=31)
    q = synth.synth_unit_rows(Q, E, seed=32)
    _ladder(g, q, [0, 3], 1e-4, 100, 33)
    _ladder(g, q, [2, 5], 1e-6, 50, 34)
    mask = np.random.default_rng(5).random(N) < 0.5
    stride = (N - 200) // 40
    for first, qis in ((100, [0, 3]), (50, [2, 5])):
        for j in range(len(qis)):
            for t in range(40):      # 35 of each ladder's 40 rows stay live: more than the bf16 tier's 32 candidate tiles
                mask[first + 7 * j + stride * t] = t % 8 != 0
    gd = g.to(device)
    ix = S.GalleryIndex(gd, presplit=True)
    md = torch.from_numpy(mask).to(device)
    got = ix.search(q.to(device), k, return_dot64=True, return_status=True, row_mask=md)
    _assert_topk(got, _expect_topk(oracle, q, g, mask, k))
    st = got[3].cpu().numpy()
    assert st[2] == 1 and st[5] == 1, st                # the 1e-6 ladders: exhaustive tier
    plain = ix.search(q.to(device), k, return_dot64=True)
    assert not torch.equal(plain[1], got[1])


# ------------------------------------------------------------------ range search and self-join
def _planted(N, E, seed):
    g = synth.synth_unit_rows(N, E, seed=seed)
    for grp in range(12):
        base = g[grp * 331]
        for j in range(1, 6):
            r = base + synth.synth_unit_rows(1, E, seed=seed * 100 + grp * 10 + j)[0] * 0.03
            g[grp * 331 + j * 37] = r / r.norm()
    return g


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("E", [128, 768])
def test_masked_range_and_self_join_vs_oracle(S, ref, device, dtype, E):
    N, tau = 4099, 0.9
    g = _planted(N, E, seed=E).to(dtype)
    q = torch.cat([g[:300:7], synth.synth_unit_rows(5, E, seed=2).to(dtype)])
    mask = np.random.default_rng(E).random(N) < 0.6
    gn, qn = _np(g), _np(q)
    gd = g.to(device)
    md = torch.from_numpy(mask).to(device)
    off, idx, score, d64 = S.cosine_range(q.to(device), gd, tau, return_dot64=True, row_mask=md)
    wq, wr, wd = _oracle_range(ref, qn, gn, tau, mask)
    gq = np.repeat(np.arange(q.shape[0]), np.diff(off.cpu().numpy()))
    assert np.array_equal(gq, wq) and np.array_equal(idx.cpu().numpy(), wr)
    assert np.array_equal(d64.cpu().numpy().view(np.int64), wd.view(np.int64))
    a, b, sc, d = S.gallery_self_join(gd, tau, row_mask=md)
    wa, wb, wd = _oracle_join(ref, gn, tau, mask)
    assert wa.size > 0
    assert np.array_equal(a.cpu().numpy(), wa) and np.array_equal(b.cpu().numpy(), wb)
    assert np.array_equal(d.cpu().numpy().view(np.int64), wd.view(np.int64))
    # through an index with deletions, and its pre-split fp32 form
    ix = S.GalleryIndex(gd)
    ix.delete_rows(torch.from_numpy(np.flatnonzero(~mask)))
    a2, b2, _, d2 = ix.near_duplicates(tau)
    assert torch.equal(a2, a) and torch.equal(b2, b) and torch.equal(d2.view(torch.int64), d.view(torch.int64))
    off2, idx2, _, d642 = ix.range_search(q.to(device), tau, return_dot64=True)
    assert torch.equal(off2, off) and torch.equal(idx2, idx) and torch.equal(d642.view(torch.int64), d64.view(torch.int64))


def test_masked_calls_ignore_workspace_contents(S, device):
    """Workspace poison (0x00 vs 0xFF) does not change masked top-k, range search or self-join outputs."""
    from mmr_amd import _lib as lib
    L = lib.lib()
    N, E, Q, K = 4001, 512, 37, 10
    g = _planted(N, E, seed=5).bfloat16().to(device)
    q = g[:Q].clone()
    mask = torch.from_numpy(np.random.default_rng(2).random(N) < 0.5).to(device)
    words = S._pack_row_mask(mask, None, N)
    s = lib.stream_ptr(device)

    def topk(fill):
        ws = torch.full((L.mmr_search_workspace_bytes(N, E, Q, K),), fill, dtype=torch.uint8, device=device)
        o = [torch.full((Q, K), -7, dtype=t, device=device) for t in (torch.int32, torch.float32, torch.float64)]
        st = torch.full((Q,), -7, dtype=torch.int32, device=device)
        lib.check(L.mmr_cosine_topk_masked(q.data_ptr(), g.data_ptr(), 1, Q, N, E, K, 1.0, 0.0, None, words.data_ptr(),
                                           o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), st.data_ptr(), ws.data_ptr(),
                                           ws.numel(), s))
        return o + [st]

    def rng_(fill, join):
        cap = 4096
        ws = torch.full((L.mmr_range_workspace_bytes(N, E, 0 if join else Q, cap, 1, 0),), fill, dtype=torch.uint8,
                        device=device)
        o = [torch.full((cap,), -7, dtype=t, device=device) for t in (torch.int32, torch.int32, torch.float32, torch.float64)]
        cnt = torch.zeros(2, dtype=torch.int64, device=device)
        tail = (words.data_ptr(), cap, cap, *[x.data_ptr() for x in o], cnt.data_ptr(), ws.data_ptr(), ws.numel(), s)
        if join:
            lib.check(L.mmr_gallery_self_join_masked(g.data_ptr(), None, 1, N, E, 0.9, 1.0, 0.0, None, None, *tail))
        else:
            lib.check(L.mmr_cosine_range_masked(q.data_ptr(), g.data_ptr(), None, 1, Q, N, E, 0.9, 1.0, 0.0, None, None, *tail))
        return o + [cnt]

    for fn in (topk, lambda f: rng_(f, False), lambda f: rng_(f, True)):
        a, b = fn(0x00), fn(0xFF)
        torch.cuda.synchronize(device)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ------------------------------------------------------------------ index lifecycle
def test_index_delete_restore_graph_and_dedup(S, oracle, device):
    N, E, k = 9001, 512, 10
    g = _planted(N, E, seed=77).bfloat16()
    q = synth.synth_unit_rows(40, E, seed=78).bfloat16()
    q[:12] = g[[grp * 331 for grp in range(12)]]
    gd, qd = g.to(device), q.to(device)
    ix = S.GalleryIndex(gd)
    fresh = ix.search(qd, k, return_dot64=True, return_status=True)
    rng = np.random.default_rng(9)
    dead = rng.choice(N, 3000, replace=False)
    ix.delete_rows(torch.from_numpy(dead))
    mask = np.ones(N, bool)
    mask[dead] = False
    assert torch.equal(ix.live_mask.cpu(), torch.from_numpy(mask))
    got = ix.search(qd, k, return_dot64=True)
    _assert_topk(got, _expect_topk(oracle, q, g, mask, k))
    # a fresh index over the compacted gallery, ids mapped back
    rows = torch.from_numpy(np.flatnonzero(mask)).to(device)
    c = S.GalleryIndex(gd[rows]).search(qd, k, return_dot64=True)
    assert torch.equal(torch.where(c[1] >= 0, rows[c[1].clamp(min=0)], c[1]), got[1])
    assert torch.equal(c[2].view(torch.int64), got[2].view(torch.int64))
    # restore everything: bit-identical to an index that never deleted, status included
    ix.restore_rows(torch.from_numpy(dead))
    back = ix.search(qd, k, return_dot64=True, return_status=True)
    for x, y in zip(fresh, back):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
    # graph captured after a first deletion sees a second one
    ix.delete_rows([5])
    s = torch.cuda.Stream(device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        ix.search(qd, k, return_dot64=True)            # warm-up: workspace allocated outside the capture
    torch.cuda.current_stream(device).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gs, gi, gd64 = ix.search(qd, k, return_dot64=True)
    ix.delete_rows(torch.from_numpy(dead))
    graph.replay()
    torch.cuda.synchronize(device)
    mask[5] = False
    _assert_topk((gs, gi, gd64), _expect_topk(oracle, q, g, mask, k))
    # dedup over the live rows == keep_first over the unmasked pairs of the live rows
    from mmr_amd import dedup
    ix2 = S.GalleryIndex(gd)
    i, j, _, _ = ix2.near_duplicates(0.9)
    keep, dup = dedup.keep_first(N, i, j)
    dropped, partner = ix2.dedup(0.9)
    assert np.array_equal(dropped.cpu().numpy(), np.flatnonzero(~keep))
    assert np.array_equal(partner.cpu().numpy(), dup[~keep])
    assert dropped.numel() >= 12
    assert ix2.near_duplicates(0.9)[0].numel() == 0
    res = ix2.search(qd, k)[1].cpu().numpy().ravel()
    assert not set(dropped.cpu().numpy().tolist()) & set(res.tolist())


@pytest.mark.slow
def test_full_size_masked_topk(S, oracle, device):
    N, E, Q, k = 1_000_000, 512, 256, 10
    g = synth.synth_unit_rows(N, E, seed=101).bfloat16()
    q = synth.synth_unit_rows(Q, E, seed=102).bfloat16()
    mask = np.random.default_rng(3).random(N) < 0.5
    gd = g.to(device)
    ix = S.GalleryIndex(gd)
    ix.delete_rows(torch.from_numpy(np.flatnonzero(~mask)))
    score, idx, d64, status = ix.search(q.to(device), k, return_dot64=True, return_status=True)
    sample = [0, 1, 77, 128, 255]
    want = _expect_topk(oracle, q[sample], g, mask, k)
    _assert_topk((score[sample], idx[sample], d64[sample]), want)
    idx_np = idx.cpu().numpy()
    assert mask[idx_np].all(), "a masked row was returned"
    d = d64.cpu().numpy()
    assert np.all(np.diff(d, axis=1) <= 0)             # descending
    assert (status.cpu().numpy() == 0).mean() > 0.9    # the fast path certifies almost every query
