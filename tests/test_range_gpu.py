"""GPU parity: threshold (range) search and gallery self-join vs a brute-force fp64 oracle.

Oracle: numpy fp64 products find every pair within 1e-6 of the threshold or above it; oracle/search_ref.c's
mmr_ref_dot64 then makes the exact decision on those pairs and gives the exact bits."""
import ctypes

import numpy as np
import pytest
import torch

from mmr_amd import synth

pytestmark = pytest.mark.gpu

F32P = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def S(device):
    from mmr_amd import search
    return search


@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


def _f32(x: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(x.detach().float().cpu().numpy())


def _dot64(ref, a: np.ndarray, b: np.ndarray) -> float:
    return ref.mmr_ref_dot64(a.ctypes.data_as(F32P), b.ctypes.data_as(F32P), a.shape[0])


def _oracle_range(ref, q: np.ndarray, g: np.ndarray, tau: float):
    """-> (qids, rows, dot64) sorted by (q, row)"""
    s = q.astype(np.float64) @ g.astype(np.float64).T
    qs, rs = np.nonzero(s >= tau - 1e-6)
    d = np.array([_dot64(ref, q[a], g[b]) for a, b in zip(qs, rs)], dtype=np.float64)
    keep = d >= tau
    return qs[keep].astype(np.int64), rs[keep].astype(np.int64), d[keep]


def _oracle_join(ref, g: np.ndarray, tau: float, block: int = 1024):
    g64 = g.astype(np.float64)
    ii, jj = [], []
    for s0 in range(0, g.shape[0], block):
        s = g64[s0:s0 + block] @ g64.T
        a, b = np.nonzero(s >= tau - 1e-6)
        a = a + s0
        up = b > a
        ii.append(a[up])
        jj.append(b[up])
    ii, jj = np.concatenate(ii), np.concatenate(jj)
    o = np.lexsort((jj, ii))
    ii, jj = ii[o], jj[o]
    d = np.array([_dot64(ref, g[a], g[b]) for a, b in zip(ii, jj)], dtype=np.float64)
    keep = d >= tau
    return ii[keep].astype(np.int64), jj[keep].astype(np.int64), d[keep]


def _assert_same(got_a, got_b, got_score, got_d, want_a, want_b, want_d, scale):
    got_a, got_b = got_a.cpu().numpy().astype(np.int64), got_b.cpu().numpy().astype(np.int64)
    got_d, got_score = got_d.cpu().numpy(), got_score.cpu().numpy()
    assert got_a.shape == want_a.shape, (got_a.shape, want_a.shape)
    assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)
    assert np.array_equal(got_d.view(np.int64), want_d.view(np.int64)), "dot64 bits differ from the oracle"
    assert np.array_equal(got_score, (want_d * scale).astype(np.float32))


def _check_range_result(res, Q, want, scale):
    offsets, idx, score, d64 = res
    offsets = offsets.cpu().numpy()
    assert offsets.shape == (Q + 1,) and offsets[0] == 0 and np.all(np.diff(offsets) >= 0)
    qids = torch.from_numpy(np.repeat(np.arange(Q), np.diff(offsets)))
    _assert_same(qids, idx, score, d64, *want, scale)


@pytest.mark.parametrize("N", [1000, 10007])
@pytest.mark.parametrize("Q", [1, 7, 300])
@pytest.mark.parametrize("E", [128, 512, 768])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_cosine_range_vs_oracle(S, ref, device, N, Q, E, dtype):
    gal = synth.synth_unit_rows(N, E, seed=N + E).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=7 * Q + E).to(dtype)
    gf, qf = _f32(gal), _f32(q)
    s = qf.astype(np.float64) @ gf.astype(np.float64).T
    taus = [float(s.max()) + 0.01,                                                  # empty
            float(np.quantile(s, 1 - min(0.5, 20.0 / s.size))),                     # sparse
            float(np.quantile(s, 1 - min(0.5, 20000.0 / s.size)))]                  # dense
    gd, qd = gal.to(device), q.to(device)
    for tau in taus:
        want = _oracle_range(ref, qf, gf, tau)
        res = S.cosine_range(qd, gd, tau, scale=100.0, return_dot64=True)
        _check_range_result(res, Q, want, 100.0)
    if Q == 1:                                   # a 1-D query: flat (idx, scores, dot64)
        idx, score, d64 = S.cosine_range(qd[0], gd, taus[1], return_dot64=True)
        want = _oracle_range(ref, qf, gf, taus[1])
        _assert_same(torch.zeros_like(idx), idx, score, d64, *want, 1.0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_unnormalised_rows_margin_from_measured_bound(S, ref, device, dtype):
    rng = np.random.default_rng(5)
    N, Q, E = 10007, 7, 512
    gal = synth.synth_unit_rows(N, E, seed=41) * torch.from_numpy(rng.uniform(5, 30, (N, 1)).astype(np.float32))
    q = synth.synth_unit_rows(Q, E, seed=42) * torch.from_numpy(rng.uniform(5, 30, (Q, 1)).astype(np.float32))
    gal, q = gal.to(dtype), q.to(dtype)
    gf, qf = _f32(gal), _f32(q)
    s = qf.astype(np.float64) @ gf.astype(np.float64).T
    for quant in (1 - 30.0 / s.size, 0.99):
        tau = float(np.quantile(s, quant))
        want = _oracle_range(ref, qf, gf, tau)
        _check_range_result(S.cosine_range(q.to(device), gal.to(device), tau, return_dot64=True), Q, want, 1.0)
        # an understated caller bound cannot shrink the margin below the measured one (GalleryIndex takes the max)
        idx = S.GalleryIndex(gal.to(device), norm_bound=1.0)
        _check_range_result(idx.range_search(q.to(device), tau, return_dot64=True), Q, want, 1.0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_threshold_boundary_is_inclusive(S, ref, device, dtype):
    N, E = 4000, 512
    gal = synth.synth_unit_rows(N, E, seed=3).to(dtype)
    q = synth.synth_unit_rows(3, E, seed=4).to(dtype)
    gf, qf = _f32(gal), _f32(q)
    r = 1234
    d = _dot64(ref, qf[1], gf[r])
    gd, qd = gal.to(device), q.to(device)
    for tau, inside in ((d, True), (float(np.nextafter(d, np.inf)), False)):
        want = _oracle_range(ref, qf, gf, tau)
        res = S.cosine_range(qd, gd, tau, return_dot64=True)
        _check_range_result(res, 3, want, 1.0)
        offsets, idx = res[0].cpu().numpy(), res[1].cpu().numpy()
        assert (r in idx[offsets[1]:offsets[2]].tolist()) == inside


def _planted_gallery(N, E, seed):
    """Unit rows with planted near-duplicates: exact copies inside one 32-row tile, across tiles and across 256-row
    query blocks, noisy copies, and a chain a~b, b~c with a !~ c at threshold 0.9."""
    g = synth.synth_unit_rows(N, E, seed=seed).numpy()
    rng = np.random.default_rng(seed)
    g[9] = g[3]                          # same tile
    g[70] = g[40]                        # across tiles
    g[N - 5] = g[100]                    # across query blocks
    g[N // 2 + 1] = g[N // 2]            # (and the copy right after a block boundary's row)
    for a, b in ((200, 801), (333, N - 100), (N - 300, N - 299)):
        x = g[a] + 0.1 * rng.standard_normal(E).astype(np.float32) / np.sqrt(E)
        g[b] = x / np.linalg.norm(x)
    a = g[500].astype(np.float64)
    u = rng.standard_normal(E)
    u -= u.dot(a) * a
    u /= np.linalg.norm(u)
    c = 0.7 * a + np.sqrt(1 - 0.49) * u                    # cos(a, c) = 0.7
    b = (a + c) / np.linalg.norm(a + c)                    # cos(a, b) = cos(b, c) = 0.92
    g[600], g[N - 700] = b.astype(np.float32), c.astype(np.float32)
    return torch.from_numpy(g)


@pytest.mark.parametrize("N,E", [(2048, 512), (20000, 512), (2048, 768)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_self_join_vs_oracle(S, ref, device, N, E, dtype):
    from mmr_amd import dedup

    gal = _planted_gallery(N, E, seed=N + E).to(dtype)
    gf = _f32(gal)
    gd = gal.to(device)
    tau = 0.9
    want = _oracle_join(ref, gf, tau)
    assert len(want[0]) >= 8
    i, j, score, d64 = S.gallery_self_join(gd, tau, scale=100.0)
    _assert_same(i, j, score, d64, *want, 100.0)
    ii, jj = i.cpu().numpy(), j.cpu().numpy()
    assert np.all(ii < jj)
    pairs = set(zip(ii.tolist(), jj.tolist()))
    assert (500, 600) in pairs and (600, N - 700) in pairs and (500, N - 700) not in pairs     # the chain
    i2, j2, d2 = dedup.near_duplicate_pairs(gd, tau)
    assert torch.equal(i, i2) and torch.equal(j, j2) and torch.equal(d64, d2)


def test_self_join_dense(S, ref, device):
    N, E = 2048, 128
    gal = synth.synth_unit_rows(N, E, seed=77).bfloat16()
    gf = _f32(gal)
    tau = 0.2
    want = _oracle_join(ref, gf, tau)
    assert len(want[0]) > 5000
    i, j, score, d64 = S.gallery_self_join(gal.to(device), tau)
    _assert_same(i, j, score, d64, *want, 1.0)


def test_fp32_index_equals_per_call_and_refresh(S, ref, device):
    N, E = 5000, 512
    gal = _planted_gallery(N, E, seed=9).to(device)
    q = synth.synth_unit_rows(16, E, seed=10).to(device)
    q[3] = gal[40]
    index = S.GalleryIndex(gal)
    assert index._split is not None                     # pre-split: range search scans the hi half
    for tau in (0.9, 0.12):
        a = index.range_search(q, tau, return_dot64=True)
        b = S.cosine_range(q, gal, tau, return_dot64=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    a = index.near_duplicates(0.9)
    b = S.gallery_self_join(gal, 0.9)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # rows change: a new duplicate and a row 20x longer than any before
    rows = torch.tensor([11, 4000], device=device)
    vals = torch.stack([gal[2000], gal[7] * 20.0])
    index.update_rows(rows, vals)
    g2 = index.gallery.clone()
    want = _oracle_join(ref, _f32(g2), 0.9)
    a = index.near_duplicates(0.9)
    _assert_same(a[0], a[1], a[2], a[3], *want, 1.0)
    assert (11, 2000) in set(zip(a[0].tolist(), a[1].tolist()))
    b = S.gallery_self_join(g2, 0.9)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ra = index.range_search(q, 0.9, return_dot64=True)
    rb = S.cosine_range(q, g2, 0.9, return_dot64=True)
    assert all(torch.equal(x, y) for x, y in zip(ra, rb))


def test_capacity_retry_and_c_overflow_rule(S, ref, device):
    from mmr_amd import _lib

    N, E, Q = 3000, 256, 5
    gal = synth.synth_unit_rows(N, E, seed=21).bfloat16().to(device)
    q = synth.synth_unit_rows(Q, E, seed=22).bfloat16().to(device)
    tau = 0.1
    full = S.cosine_range(q, gal, tau, return_dot64=True)
    total = int(full[0][-1])
    assert total > 100
    small = S.cosine_range(q, gal, tau, return_dot64=True, cap=3, cand_cap=5)
    assert all(torch.equal(x, y) for x, y in zip(full, small))
    with pytest.raises(MemoryError):
        S.cosine_range(q, gal, tau, cand_cap=5, max_pairs=50)
    ji, jj, js, jd = S.gallery_self_join(gal, tau)
    ji2, jj2, js2, jd2 = S.gallery_self_join(gal, tau, cap=1, cand_cap=7)
    assert torch.equal(ji, ji2) and torch.equal(jj, jj2) and torch.equal(jd, jd2)

    # the C call: counts report what is needed; with a large enough candidate list it writes exactly the first cap pairs
    L = _lib.lib()
    flat_q = torch.repeat_interleave(torch.arange(Q, device=device), torch.diff(full[0]))

    def call(cap, cand_cap):
        ws = torch.empty(L.mmr_range_workspace_bytes(N, E, Q, cand_cap, _lib.MMR_BF16, 0), dtype=torch.uint8, device=device)
        oq = torch.full((cap + 4,), -7, dtype=torch.int32, device=device)
        orow = torch.full((cap + 4,), -7, dtype=torch.int32, device=device)
        osc = torch.zeros(cap + 4, dtype=torch.float32, device=device)
        od = torch.zeros(cap + 4, dtype=torch.float64, device=device)
        counts = torch.zeros(2, dtype=torch.int64, device=device)
        _lib.check(L.mmr_cosine_range(q.data_ptr(), gal.data_ptr(), None, _lib.MMR_BF16, Q, N, E, tau, 1.0, 0.0, None, None,
                                      cap, cand_cap, oq.data_ptr(), orow.data_ptr(), osc.data_ptr(), od.data_ptr(),
                                      counts.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(device)))
        return counts.tolist(), oq, orow, od

    (m, c), oq, orow, od = call(7, 1 << 16)
    assert m == total and c >= m
    assert torch.equal(oq[:7].long(), flat_q[:7]) and torch.equal(orow[:7].long(), full[1][:7])
    assert torch.equal(od[:7], full[3][:7])
    assert bool((oq[7:] == -7).all()) and bool((orow[7:] == -7).all())       # nothing written past cap
    (m2, c2), *_ = call(7, 10)
    assert c2 == c and c2 > 10                                                # the counter keeps counting past cand_cap


def test_determinism(S, device):
    gal = _planted_gallery(20000, 512, seed=31).bfloat16().to(device)
    q = synth.synth_unit_rows(300, 512, seed=32).bfloat16().to(device)
    a = S.cosine_range(q, gal, 0.1, return_dot64=True)
    b = S.cosine_range(q, gal, 0.1, return_dot64=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a = S.gallery_self_join(gal, 0.15)
    b = S.gallery_self_join(gal, 0.15)
    assert a[0].numel() > 1000
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.slow
def test_self_join_1m_planted(S, ref, device):
    N, E, P = 1_000_000, 512, 1000
    torch.manual_seed(0)
    g = torch.randn(N, E, device=device)
    g = g / g.norm(dim=-1, keepdim=True)
    rng = np.random.default_rng(1)
    picks = rng.choice(N, 2 * P, replace=False)
    src, dst = picks[:P], picks[P:]
    noise = torch.randn(P, E, device=device) * (0.05 / np.sqrt(E))
    srcs = torch.from_numpy(src).to(device)
    dsts = torch.from_numpy(dst).to(device)
    cp = g[srcs] + torch.where(torch.arange(P, device=device)[:, None] % 2 == 0, torch.zeros_like(noise), noise)
    g[dsts] = cp / cp.norm(dim=-1, keepdim=True)
    gb = g.bfloat16().contiguous()
    del g
    i, j, score, d64 = S.gallery_self_join(gb, 0.9)
    want = sorted((min(a, b), max(a, b)) for a, b in zip(src.tolist(), dst.tolist()))
    got = list(zip(i.tolist(), j.tolist()))
    assert got == want
    rows = _f32(gb[torch.from_numpy(np.array([x for p in want for x in p])).to(device)])
    wd = np.array([_dot64(ref, rows[2 * k], rows[2 * k + 1]) for k in range(P)])
    assert np.array_equal(d64.cpu().numpy().view(np.int64), wd.view(np.int64))
