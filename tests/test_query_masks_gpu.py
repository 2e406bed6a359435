"""GPU: a row mask per query (``row_masks=``; mmr_cosine_topk_deep_qmasked, mmr_row_masks_pack).

The contract: row q of the result equals, bit for bit, the existing single-mask call for query q alone with
``row_mask = row_masks[q] (& row_mask)``.  Expected values come from two independent sources and are compared bit for bit
(idx, score, dot64):
  - oracle/search_ref.c per query over the compacted gallery gallery[mask_q], ids mapped back (search_helpers.expect_topk);
  - the existing single-mask GPU call, once per query.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from mmr_amd import synth
from search_helpers import expect_topk, to_np

pytestmark = pytest.mark.gpu

FORMS = ("bf16", "fp16", "f32-presplit", "f32-frontend")


@pytest.fixture(scope="module")
def S(device):
    from mmr_amd import search
    return search


@pytest.fixture(scope="module")
def oracle():
    from oracle import search_ref
    return search_ref


def _dtype(form):
    return {"bf16": torch.bfloat16, "fp16": torch.float16}.get(form, torch.float32)


def _pack_host(keep):
    """bool [Q, N] -> int32 words [Q, ceil(N/32)] (numpy): bit r & 31 of word r >> 5"""
    Q, N = keep.shape
    W = max((N + 31) // 32, 1)
    pad = np.zeros((Q, W * 32), np.uint8)
    pad[:, :N] = keep
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint32).reshape(Q, W).view(np.int32)


def _oracle_per_query(oracle, q, g, masks, k, scale=1.0):
    """the C oracle over gallery[masks[i]] for every query i, ids mapped back -> (idx, score, dot64) [Q, k]"""
    qn, gn = to_np(q), to_np(g)

    def one(i):      # search_helpers.expect_topk on arrays converted once
        rows = np.flatnonzero(masks[i])
        if rows.size == 0:
            return np.full((1, k), -1, np.int64), np.full((1, k), -np.inf, np.float32), np.full((1, k), -np.inf, np.float64)
        oi, os_, od = oracle.cosine_topk(qn[i:i + 1], gn[rows], k, scale=scale)
        return np.where(oi >= 0, rows[np.clip(oi, 0, None)], -1), os_, od
    with ThreadPoolExecutor(8) as ex:
        parts = list(ex.map(one, range(q.shape[0])))
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


def _same(got, want, what):
    score, idx, d64 = got[:3]
    wi, ws, wd = want
    gi = idx.cpu().numpy()
    bad = np.flatnonzero((gi != wi).any(1))
    assert bad.size == 0, f"{what}: indices differ for queries {bad[:8].tolist()} (of {bad.size})"
    assert np.array_equal(d64.cpu().numpy().view(np.int64), np.ascontiguousarray(wd).view(np.int64)), f"{what}: dot64 bits differ"
    assert np.array_equal(score.cpu().numpy().view(np.int32), np.ascontiguousarray(ws).view(np.int32)), f"{what}: score bits differ"


def _t2np(got):
    """(score, idx, dot64) tensors -> the (idx, score, dot64) numpy triple _same takes as `want`"""
    return got[1].cpu().numpy(), got[0].cpu().numpy(), got[2].cpu().numpy()


class _Run:
    """One gallery on the device in one of FORMS: the per-query call and the single-mask call it must reproduce."""

    def __init__(self, S, device, form, g):
        self.S, self.device, self.form = S, device, form
        self.gd = g.to(device)
        self.ix = S.GalleryIndex(self.gd, presplit=True) if form == "f32-presplit" else None

    def qmasked(self, q, k, row_masks, scale=1.0, row_mask=None):
        if self.ix is not None:
            return self.ix.search_deep(q.to(self.device), k, scale, return_dot64=True, row_mask=row_mask, row_masks=row_masks)
        return self.S.cosine_topk_deep(q.to(self.device), self.gd, k, scale, return_dot64=True, row_mask=row_mask, row_masks=row_masks)

    def single(self, q, k, mask, scale=1.0):
        rm = torch.from_numpy(mask).to(self.device)
        if self.ix is not None:
            return self.ix.search_deep(q.to(self.device), k, scale, return_dot64=True, row_mask=rm)
        return self.S.cosine_topk_deep(q.to(self.device), self.gd, k, scale, return_dot64=True, row_mask=rm)

    def loop(self, q, k, masks, scale=1.0):
        parts = [_t2np(self.single(q[i:i + 1], k, masks[i], scale)) for i in range(q.shape[0])]
        return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


def _family_masks(oracle, q, g, k, seed):
    """Query i gets mask family i mod 8 -> (bool [Q, N], int32 words [Q, W]; family 7's words carry garbage past N)."""
    Q, N = q.shape[0], g.shape[0]
    rng = np.random.default_rng(seed)
    keep = np.ones((Q, N), bool)
    ones = np.flatnonzero(np.arange(Q) % 8 == 5)
    top1 = {}
    if ones.size:        # family 6 flips the top-1 row of its all-ones predecessor
        t = expect_topk(oracle, q[torch.from_numpy(ones)], g, np.ones(N, bool), 1)[0][:, 0]
        top1 = dict(zip(ones.tolist(), t.tolist()))
    for i in range(Q):
        f = i % 8
        if f == 0 or f == 7:
            keep[i] = rng.random(N) < 0.5
        elif f == 1:
            keep[i] = rng.random(N) < 0.001
        elif f == 2:     # dead 32-row tiles and dead 64-row tasks (two tiles per task at this N), the rest 70 % live
            m = rng.random(N) < 0.7
            m &= np.repeat(rng.random((N + 31) // 32) < 0.7, 32)[:N]
            m &= np.repeat(rng.random((N + 63) // 64) < 0.7, 64)[:N]
            keep[i] = m
        elif f == 3:     # fewer than k live
            keep[i] = False
            keep[i, rng.choice(N, max(k - 3, 1), replace=False)] = True
        elif f == 4:
            keep[i] = False
        elif f == 6:     # the previous query's mask (all ones) with that query's best row flipped
            keep[i] = keep[i - 1]
            keep[i, top1[i - 1]] = ~keep[i, top1[i - 1]]
    words = _pack_host(keep).copy()
    tail = N % 32
    if tail:
        garbage = rng.integers(0, 1 << 32, Q, dtype=np.uint64).astype(np.uint32) & np.uint32((0xffffffff << tail) & 0xffffffff)
        sel = np.arange(Q) % 8 == 7
        words.view(np.uint32)[sel, -1] |= garbage[sel]
    return keep, words


# =================================================================== A. top-k / deep matrix
@pytest.mark.parametrize("Qk", ["Q37k40", "twopass-k10"])
@pytest.mark.parametrize("E", [128, 256, 512, 768])
@pytest.mark.parametrize("form", FORMS)
def test_matrix_vs_oracle_and_single_mask_loop(S, oracle, device, form, E, Qk):
    N = 12007                                   # ragged last tile, 376 tiles, two tiles per task
    qmax = 256 if E <= 512 else 128
    Q, k = (37, 40) if Qk == "Q37k40" else (qmax + 44, 10)
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=7 + E).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=8 + E).to(dtype)
    keep, words = _family_masks(oracle, q, g, k, seed=E + Q)
    run = _Run(S, device, form, g)
    got = run.qmasked(q, k, S.DecisionMasks(torch.from_numpy(words).to(device), N))
    assert got[1].dtype == torch.int64 and tuple(got[1].shape) == (Q, k)
    _same(got, _oracle_per_query(oracle, q, g, keep, k), f"{form} E={E} {Qk} vs oracle")
    _same(got, run.loop(q, k, keep), f"{form} E={E} {Qk} vs the loop of single-mask calls")
    empty = torch.arange(4, Q, 8, device=device)
    assert (got[1][empty] == -1).all() and torch.isinf(got[0][empty]).all() and torch.isinf(got[2][empty]).all()


# =================================================================== B. tiles per task
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("padded", [False, True])
def test_many_tiles_per_task(S, oracle, device, k, padded):
    """13 tiles per task; `padded`: stride = W + 3 with the pad words poisoned (never read)"""
    N, E, Q = 100003, 512, 64
    g = synth.synth_unit_rows(N, E, seed=61).bfloat16()
    q = synth.synth_unit_rows(Q, E, seed=62).bfloat16()
    rng = np.random.default_rng(63)
    keep = rng.random((Q, N)) < 0.03            # sparse masks keep the per-query oracle cheap; every tile still holds live rows
    keep[5] = True
    keep[6] = False
    words = _pack_host(keep)
    W = words.shape[1]
    if padded:
        buf = np.full((Q, W + 3), -1, np.int32)
        buf[:, :W] = words
        wt = torch.from_numpy(buf).to(device)[:, :W]          # a view: rows W + 3 words apart
        assert wt.stride(0) == W + 3
    else:
        wt = torch.from_numpy(words).to(device)
    run = _Run(S, device, "bf16", g)
    got = run.qmasked(q, k, S.DecisionMasks(wt, N))
    _same(got, _oracle_per_query(oracle, q, g, keep, k), "vs oracle")
    sub = [0, 5, 6, 31, 32, 63]
    _same(tuple(t[sub] for t in got), run.loop(q[sub], k, keep[sub]), "vs the loop of single-mask calls")


def test_task_cut_to_the_lds_cap(S, oracle, device):
    """E = 768 with 128 resident queries leaves room for 31 tiles' words beside the ring; this gallery plans 32 per task"""
    N, E, Q, k = 254001, 768, 128, 10
    g = synth.synth_unit_rows(N, E, seed=71).half()
    q = synth.synth_unit_rows(Q, E, seed=72).half()
    rng = np.random.default_rng(73)
    keep = rng.random((Q, N)) < 0.01
    keep[:, -17:] = True                         # the ragged last tile is live for everybody
    run = _Run(S, device, "fp16", g)
    got = run.qmasked(q, k, torch.from_numpy(keep).to(device))
    _same(got, _oracle_per_query(oracle, q, g, keep, k), "vs oracle")
    sub = [0, 1, 63, 64, 127]
    _same(tuple(t[sub] for t in got), run.loop(q[sub], k, keep[sub]), "vs the loop of single-mask calls")


# =================================================================== C. all ones, identical rows
@pytest.mark.parametrize("form", FORMS)
def test_all_ones_and_identical_rows(S, device, form):
    N, E, Q, k = 12007, 512, 37, 40
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=81).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=82).to(dtype)
    run = _Run(S, device, form, g)
    qd = q.to(device)
    plain = (run.ix.search_deep(qd, k, return_dot64=True) if run.ix is not None else S.cosine_topk_deep(qd, run.gd, k, return_dot64=True))
    got = run.qmasked(q, k, torch.ones(Q, N, dtype=torch.bool, device=device))
    for a, b in zip(got, plain):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    m = torch.from_numpy(np.random.default_rng(83).random(N) < 0.5).to(device)
    shared = run.single(q, k, m.cpu().numpy())
    got = run.qmasked(q, k, m.unsqueeze(0).expand(Q, N).contiguous())
    for a, b in zip(got, shared):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # the same split between the two keywords: row_masks & row_mask
    half = torch.from_numpy(np.random.default_rng(84).random((Q, N)) < 0.7).to(device)
    both = run.qmasked(q, k, half, row_mask=m)
    anded = run.qmasked(q, k, half & m)
    for a, b in zip(both, anded):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# =================================================================== D. k
def test_k_1_64_65_1000_and_cosine_topk_route(S, oracle, device):
    N, E, Q = 12007, 512, 37
    g = synth.synth_unit_rows(N, E, seed=91).bfloat16()
    q = synth.synth_unit_rows(Q, E, seed=92).bfloat16()
    keep = np.random.default_rng(93).random((Q, N)) < 0.5
    keep[3] = False
    keep[3, :50] = True                          # fewer live rows than k = 64
    gd, qd, kd = g.to(device), q.to(device), torch.from_numpy(keep).to(device)
    want = _oracle_per_query(oracle, q, g, keep, 1000)
    for k in (1, 64, 65, 1000):
        got = S.cosine_topk_deep(qd, gd, k, return_dot64=True, row_masks=kd)
        _same(got, tuple(np.ascontiguousarray(w[:, :k]) for w in want), f"k={k}")
    for k in (1, 64):
        got = S.cosine_topk(qd, gd, k, return_dot64=True, row_masks=kd)
        assert got[1].dtype == torch.int64
        parts = [_t2np(S.cosine_topk(qd[i:i + 1], gd, k, return_dot64=True, row_mask=kd[i])) for i in range(Q)]
        _same(got, tuple(np.concatenate([p[j] for p in parts]) for j in range(3)), f"cosine_topk k={k}")
    with pytest.raises(ValueError):
        S.cosine_topk(qd, gd, 10, return_status=True, row_masks=kd)
    ix = S.GalleryIndex(gd)
    a = ix.search(qd, 10, return_dot64=True, row_masks=kd)
    _same(a, tuple(np.ascontiguousarray(w[:, :10]) for w in want), "GalleryIndex.search")


# =================================================================== E. non-finite
@pytest.mark.parametrize("form", ["bf16", "f32-frontend"])
def test_non_finite_rows_and_a_nan_query(S, oracle, device, form):
    N, E, Q, k = 4001, 256, 8, 20
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=101).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=102).to(dtype)
    g[100, 7] = float("nan")                     # its dot is NaN for every query: absent whether a mask keeps it or not
    g[2000, 3] = float("inf")                    # +-inf dots: rank first / last where live
    q[4, 0] = float("nan")                       # a NaN query between two ordinary ones: an empty result
    keep = np.random.default_rng(103).random((Q, N)) < 0.5
    keep[0::2, 100] = keep[0::2, 2000] = True
    keep[1::2, 100] = keep[1::2, 2000] = False
    run = _Run(S, device, form, g)
    got = run.qmasked(q, k, torch.from_numpy(keep).to(device))
    _same(got, _oracle_per_query(oracle, q, g, keep, k), "vs oracle")
    _same(got, run.loop(q, k, keep), "vs the loop of single-mask calls")
    idx = got[1].cpu().numpy()
    assert not (idx == 100).any() and (idx[4] == -1).all()
    assert not (idx[1::2] == 2000).any()         # the Inf row is dead for the odd queries (live: first or last, by its sign)


# =================================================================== F. cascade
@pytest.mark.parametrize("form", ["bf16", "f32-presplit"])
def test_cascade_decide_then_rank(S, device, form):
    """rank with tower B among the rows tower A's thresholds accepted; then the same with deleted rows and a shared row_mask"""
    N, E, Q, k = 12007, 512, 12, 20
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=111).to(dtype).to(device)
    a = synth.synth_unit_rows(Q, E, seed=112).to(dtype).to(device)
    b = synth.synth_unit_rows(Q, E, seed=113).to(dtype).to(device)
    ix = S.GalleryIndex(g, presplit=form == "f32-presplit")
    thr = [0.0, 0.02, 0.05, 0.08, -0.05, 0.1, 0.5, -1.0, 0.03, 0.04, 0.06, 0.01]      # some accept a few rows, one none, one all
    extra = torch.from_numpy(np.random.default_rng(114).random(N) < 0.6).to(device)
    for stage in ("fresh", "deleted"):
        if stage == "deleted":
            ix.delete_rows(torch.arange(0, N, 3))
        rm = extra if stage == "deleted" else None
        m = ix.decide(a, thr)
        got = ix.search_deep(b, k, return_dot64=True, row_masks=m, row_mask=rm)
        for i in range(Q):
            mi = m.row_mask(i) if rm is None else m.row_mask(i) & rm
            one = ix.search_deep(b[i:i + 1], k, return_dot64=True, row_mask=mi)
            for x, y in zip(got, one):
                assert torch.equal(x[i:i + 1].view(torch.uint8), y.view(torch.uint8)), (stage, i)
        live = m.num_set().cpu().numpy()
        assert live.min() == 0 and live.max() > k


# =================================================================== G. the C ABI
def _c_qdeep(device, q, g, k, words, stride, shared, cap, fill=None, out=None, split=None):
    from mmr_amd import _lib
    L = _lib.lib()
    Q, E = q.shape
    N = g.shape[0]
    code = _lib.dtype_code(g.dtype)
    hi, lo, resid = split if split is not None else (None, None, None)
    need = L.mmr_deep_topk_qmasked_workspace_bytes(N, E, Q, k, cap, cap, code, int(hi is not None))
    assert need > 0
    if out is None:
        ws = torch.empty(need, dtype=torch.uint8, device=device) if fill is None else torch.full((need,), fill, dtype=torch.uint8, device=device)
        out = (torch.full((Q, k), -7.0, dtype=torch.float32, device=device), torch.full((Q, k), -7, dtype=torch.int64, device=device),
               torch.full((Q, k), -7.0, dtype=torch.float64, device=device), torch.zeros(2, dtype=torch.int64, device=device), ws)
    score, idx, d64, counts, ws = out
    _lib.check(L.mmr_cosine_topk_deep_qmasked(q.data_ptr(), g.data_ptr(), _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(resid), code, Q, N, E,
                                              k, 1.0, 0.0, None, words.data_ptr(), stride, _lib.ptr(shared), cap, cap,
                                              idx.data_ptr(), score.data_ptr(), d64.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                              ws.numel(), _lib.stream_ptr(device)))
    return out


def test_c_abi_with_a_poisoned_workspace(S, oracle, device):
    N, E, Q, k = 4001, 512, 37, 10
    g = synth.synth_unit_rows(N, E, seed=121).bfloat16()
    q = synth.synth_unit_rows(Q, E, seed=122).bfloat16()
    rng = np.random.default_rng(123)
    keep = rng.random((Q, N)) < 0.5
    shared = rng.random(N) < 0.8
    gd, qd = g.to(device), q.to(device)
    words = torch.from_numpy(_pack_host(keep)).to(device)
    sw = torch.from_numpy(_pack_host(shared[None])[0]).to(device)
    want = _oracle_per_query(oracle, q, g, keep & shared, k)
    outs = []
    for fill in (0x00, 0xFF):
        o = _c_qdeep(device, qd, gd, k, words, words.shape[1], sw, 1 << 14, fill=fill)
        torch.cuda.synchronize(device)
        assert int(o[3][0]) <= 1 << 14 and int(o[3][1]) <= 1 << 14
        _same(o, want, f"workspace filled with {fill:#x}")
        outs.append(o)
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("N", [1, 31, 32, 33, 50003])
def test_row_masks_pack_vs_host(device, N):
    from mmr_amd import _lib
    L = _lib.lib()
    Q = 5
    rng = np.random.default_rng(N)
    keep = rng.random((Q, N)) < 0.5
    andm = rng.random(N) < 0.7
    W = (N + 31) // 32
    kd = torch.from_numpy(keep).to(device)
    ad = torch.from_numpy(_pack_host(andm[None])[0]).to(device)
    for stride, am in ((W, None), (W + 2, ad)):
        out = torch.full((Q, stride), 0x5a5a5a5a, dtype=torch.int32, device=device)
        _lib.check(L.mmr_row_masks_pack(kd.data_ptr(), _lib.ptr(am), Q, N, stride, out.data_ptr(), _lib.stream_ptr(device)))
        want = np.zeros((Q, stride), np.int32)
        want[:, :W] = _pack_host(keep if am is None else keep & andm)
        assert np.array_equal(out.cpu().numpy(), want), (N, stride)


# =================================================================== H. graph capture
def test_c_call_is_graph_capturable(S, oracle, device):
    N, E, Q, k = 20011, 512, 16, 100
    g = synth.synth_unit_rows(N, E, seed=131).bfloat16()
    qs = [synth.synth_unit_rows(Q, E, seed=132 + i).bfloat16() for i in range(2)]
    keeps = [np.random.default_rng(140 + i).random((Q, N)) < 0.5 for i in range(2)]
    gd = g.to(device)
    W = (N + 31) // 32
    cap = 8 * Q * k
    eager = []
    for q, kp in zip(qs, keeps):
        e = _c_qdeep(device, q.to(device), gd, k, torch.from_numpy(_pack_host(kp)).to(device), W, None, cap)
        torch.cuda.synchronize(device)
        assert e[3][0].item() <= cap and e[3][1].item() <= cap
        eager.append([t.clone() for t in e[:4]])
    static_q = qs[0].to(device).clone()
    static_w = torch.from_numpy(_pack_host(keeps[0])).to(device)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        out = _c_qdeep(device, static_q, gd, k, static_w, W, None, cap)          # warm, outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _c_qdeep(device, static_q, gd, k, static_w, W, None, cap, out=out)
    torch.cuda.current_stream(device).wait_stream(side)
    for i in (1, 0):
        static_q.copy_(qs[i].to(device))
        static_w.copy_(torch.from_numpy(_pack_host(keeps[i])).to(device))
        graph.replay()
        torch.cuda.synchronize(device)
        for a, b in zip(out[:4], eager[i]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), i
        _same(out, _oracle_per_query(oracle, qs[i], g, keeps[i], k), f"replay {i}")


# =================================================================== I. the labelled threshold sweep
@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


def _six_class_gallery(N, E, seed, dtype):
    """sweep_helpers.labelled_gallery's recipe with 6 classes -> (gallery, labels int32 [N], centres [6, E])"""
    centres = synth.synth_unit_rows(6, E, seed=seed)
    labels = torch.from_numpy(np.random.default_rng(seed + 1).integers(0, 6, N).astype(np.int32))
    g = 0.12 * centres[labels.long()] + synth.synth_unit_rows(N, E, seed=seed + 2)
    return (g / g.norm(dim=-1, keepdim=True)).to(dtype), labels, centres


def _raw_sweep_qm(device, q, g, labels, targets, thr, words, stride, shared, cand_cap, fill):
    from mmr_amd import _lib
    L = _lib.lib()
    Q, E = q.shape
    N = g.shape[0]
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    T = thr.shape[0]
    need = L.mmr_sweep_workspace_bytes(N, E, Q, T, cand_cap, _lib.dtype_code(g.dtype), 0)
    assert need > 0
    ws = torch.full((need,), fill, dtype=torch.uint8, device=device)
    outs = [torch.full((n,), fill, dtype=torch.uint8, device=device).view(torch.int64) for n in (Q * 2 * T * 8, Q * 2 * 8, 16)]
    _lib.check(L.mmr_threshold_sweep_qmasked(q.data_ptr(), g.data_ptr(), None, _lib.dtype_code(g.dtype), Q, N, E, labels.data_ptr(),
                                             targets.data_ptr(), thr.ctypes.data, T, 0.0, None, None, words.data_ptr(), stride,
                                             _lib.ptr(shared), cand_cap, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                             ws.data_ptr(), need, _lib.stream_ptr(device)))
    torch.cuda.synchronize(device)
    return outs[0].view(Q, 2, T), outs[1].view(Q, 2), outs[2]


SWEEP_CASES = {"E512-bf16-T200": (512, torch.bfloat16, 37, 200), "E768-fp16-T200": (768, torch.float16, 37, 200),
               "E512-fp32-T50": (512, torch.float32, 13, 50), "E512-bf16-T1001": (512, torch.bfloat16, 37, 1001)}


@pytest.mark.parametrize("kind", ["leave-out", "random"])
@pytest.mark.parametrize("case", list(SWEEP_CASES))
def test_sweep_vs_oracle_and_single_mask_loop(S, ref, device, case, kind):
    import sweep_helpers as H
    E, dtype, Q, T = SWEEP_CASES[case]
    N = 12007
    gal, labels, centres = _six_class_gallery(N, E, seed=E + T, dtype=dtype)
    q = synth.synth_unit_rows(Q, E, seed=E + T + 5)
    q[:6] = centres
    q = q.to(dtype)
    targets = torch.arange(Q, dtype=torch.int32) % 6
    rng = np.random.default_rng(Q + T)
    if kind == "leave-out":      # every query leaves 10 rows of its own class (its "shots") out of its gallery
        lab = labels.numpy()
        shots = np.stack([rng.choice(np.flatnonzero(lab == int(targets[i])), 10, replace=False) for i in range(Q)])
        masks = S.leave_out_masks(Q, N, np.repeat(np.arange(Q), 10), shots.reshape(-1), device)
        keep = np.ones((Q, N), bool)
        keep[np.repeat(np.arange(Q), 10), shots.reshape(-1)] = False
    else:
        keep = rng.random((Q, N)) < 0.5
        keep[2] = False                          # an empty gallery for one query
        masks = torch.from_numpy(keep).to(device)
    thr = np.linspace(-0.15, 0.45, T)
    gd, qd, ld, td = gal.to(device), q.to(device), labels.to(device), targets.to(device)
    res = S.threshold_sweep(qd, gd, ld, td, thr, row_masks=masks)
    gf, qf = H.f32(gal), H.f32(q)
    ge = np.zeros((Q, 2, T), np.int64)
    total = np.zeros((Q, 2), np.int64)
    for i in range(Q):
        a, b, _ = H.oracle_sweep(ref, qf[i:i + 1], gf, labels.numpy(), targets.numpy()[i:i + 1], thr, mask=keep[i])
        ge[i], total[i] = a[0], b[0]
    H.check_sweep(res, ge, total)
    assert int(res.pos[2]) + int(res.neg[2]) == (0 if kind == "random" else N - 10)
    ix = S.GalleryIndex(gd)
    for i in list(range(0, Q, 5)) + [2]:         # the existing single-mask call, query by query
        one = ix.threshold_sweep(qd[i:i + 1], ld, td[i:i + 1], thr, row_mask=torch.from_numpy(keep[i]).to(device))
        assert torch.equal(one.tp[0], res.tp[i]) and torch.equal(one.fp[0], res.fp[i]), i
        assert int(one.pos[0]) == int(res.pos[i]) and int(one.neg[0]) == int(res.neg[i]), i
    again = ix.threshold_sweep(qd, ld, td, thr, row_masks=masks)       # the index form: same counts
    assert torch.equal(again.tp, res.tp) and torch.equal(again.fp, res.fp)


def test_sweep_c_abi_with_a_poisoned_workspace(S, ref, device):
    import sweep_helpers as H
    N, E, Q, T = 4001, 512, 37, 25
    gal, labels, centres = _six_class_gallery(N, E, seed=151, dtype=torch.bfloat16)
    q = synth.synth_unit_rows(Q, E, seed=152)
    q[:6] = centres
    q = q.bfloat16()
    targets = torch.arange(Q, dtype=torch.int32) % 6
    rng = np.random.default_rng(153)
    keep = rng.random((Q, N)) < 0.5
    shared = rng.random(N) < 0.8
    thr = np.arange(-0.2, 1.0001, 0.05)
    words = torch.from_numpy(_pack_host(keep)).to(device)
    sw = torch.from_numpy(_pack_host(shared[None])[0]).to(device)
    gf, qf = H.f32(gal), H.f32(q)
    ge = np.zeros((Q, 2, T), np.int64)
    total = np.zeros((Q, 2), np.int64)
    for i in range(Q):
        a, b, _ = H.oracle_sweep(ref, qf[i:i + 1], gf, labels.numpy(), targets.numpy()[i:i + 1], thr, mask=keep[i] & shared)
        ge[i], total[i] = a[0], b[0]
    outs = []
    for fill in (0x00, 0xFF):
        o = _raw_sweep_qm(device, q.to(device), gal.to(device), labels.to(device), targets.to(device), thr, words, words.shape[1], sw,
                          1 << 17, fill)
        assert 0 < int(o[2][0]) == int(o[2][1]) <= 1 << 17
        assert np.array_equal(o[0].cpu().numpy(), ge) and np.array_equal(o[1].cpu().numpy(), total), hex(fill)
        outs.append(o)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# =================================================================== J. the example
def test_few_shot_sweep_example(device):
    """examples/few_shot_sweep_synthetic.py checks in-script that the one call equals the loop of single-mask calls"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "few_shot_sweep_synthetic.py")
    spec = importlib.util.spec_from_file_location("few_shot_sweep_synthetic", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    report = mod.main(["--rows", "20000"])
    assert len(report) == 24 and [r[0] for r in report[::6]] == [1, 5, 10, 20]
    f1 = np.array([r[3] for r in report]).reshape(4, 6)
    assert np.isfinite(f1).all() and f1[3].mean() > f1[0].mean()      # a mean of 20 shots is a better class vector than one shot
