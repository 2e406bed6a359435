"""Workspace contents must not leak into results: every C-ABI search call run twice on the same inputs, once with its
workspace filled with 0x00 bytes and once with 0xFF (NaN as fp32, -1 as integers), gives bit-identical outputs.

Callers allocate workspaces with torch.empty, so a region read before the call writes it would otherwise go unnoticed.
The output buffers are filled alike in both runs (entries a call legitimately leaves alone compare equal)."""
import pytest
import torch

from mmr_amd import synth

pytestmark = pytest.mark.gpu

N, E, Q, K = 4001, 512, 37, 10
TAU, CAP, CAND_CAP = 0.5, 1000, 4096
SWEEP_T, SWEEP_CAND_CAP = 25, 1 << 17       # grid -0.2 .. 1.0 in steps of 0.05: it crosses the bulk near 0 and the planted rows
DEEP_K = 100
DEEP_CAP = 1 << 15                          # tile and survivor capacity: k nears the 126 tiles, so ~200 survivors per query


@pytest.fixture(scope="module")
def data(device):
    gal = synth.synth_unit_rows(N, E, seed=31)
    q = synth.synth_unit_rows(Q, E, seed=32)
    base = gal[5].clone()
    noise = synth.synth_unit_rows(12, E, seed=33) * 0.05
    near = base + noise
    gal[list(range(100, 4000, 330))] = near / near.norm(dim=1, keepdim=True)   # 12 near duplicates of row 5: 13 matches, 78 pairs
    q[0] = base
    return gal.to(device), q.to(device)


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu()


def _topk(L, lib, device, qd, gd, dtype, split):
    nq, n = qd.shape[0], gd.shape[0]
    ws_bytes = L.mmr_search_workspace_bytes(n, E, nq, K)
    st = lib.stream_ptr(device)
    if split:
        hi = torch.empty(n, E, dtype=torch.bfloat16, device=device)
        lo = torch.empty_like(hi)
        resid = torch.empty(1, dtype=torch.float32, device=device)
        lib.check(L.mmr_gallery_split_bf16(gd.data_ptr(), n, E, hi.data_ptr(), lo.data_ptr(), resid.data_ptr(), st))

    def run(fill):
        ws = torch.full((ws_bytes,), fill, dtype=torch.uint8, device=device)
        idx = torch.full((nq, K), -7, dtype=torch.int32, device=device)
        score = torch.full((nq, K), -7.0, dtype=torch.float32, device=device)
        d64 = torch.full((nq, K), -7.0, dtype=torch.float64, device=device)
        status = torch.full((nq,), -7, dtype=torch.int32, device=device)
        if split:
            lib.check(L.mmr_cosine_topk_split(qd.data_ptr(), gd.data_ptr(), hi.data_ptr(), lo.data_ptr(), resid.data_ptr(), nq,
                                              n, E, K, 100.0, 0.0, None, idx.data_ptr(), score.data_ptr(), d64.data_ptr(),
                                              status.data_ptr(), ws.data_ptr(), ws_bytes, st))
        else:
            q_, g_ = qd.to(dtype), gd.to(dtype)
            lib.check(L.mmr_cosine_topk_ex(q_.data_ptr(), g_.data_ptr(), lib.dtype_code(dtype), nq, n, E, K, 100.0, 0.0, None,
                                           idx.data_ptr(), score.data_ptr(), d64.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                           ws_bytes, st))
        torch.cuda.synchronize(device)
        return idx, score, d64, status
    return run


def _range(L, lib, device, qd, gd, dtype, self_join, hi_given):
    n = gd.shape[0]
    nq = 0 if self_join else qd.shape[0]
    g_ = gd.to(dtype)
    q_ = qd.to(dtype)
    st = lib.stream_ptr(device)
    hi = None
    if hi_given:
        hi = torch.empty(n, E, dtype=torch.bfloat16, device=device)
        lo = torch.empty_like(hi)
        lib.check(L.mmr_gallery_split_bf16(g_.data_ptr(), n, E, hi.data_ptr(), lo.data_ptr(), None, st))
    ws_bytes = L.mmr_range_workspace_bytes(n, E, nq, CAND_CAP, lib.dtype_code(dtype), int(hi_given))

    def run(fill):
        ws = torch.full((ws_bytes,), fill, dtype=torch.uint8, device=device)
        oa = torch.full((CAP,), -7, dtype=torch.int32, device=device)
        ob = torch.full((CAP,), -7, dtype=torch.int32, device=device)
        sc = torch.full((CAP,), -7.0, dtype=torch.float32, device=device)
        d64 = torch.full((CAP,), -7.0, dtype=torch.float64, device=device)
        counts = torch.full((2,), -7, dtype=torch.int64, device=device)
        common = (TAU, 100.0, 0.0, None, None, CAP, CAND_CAP, oa.data_ptr(), ob.data_ptr(), sc.data_ptr(), d64.data_ptr(),
                  counts.data_ptr(), ws.data_ptr(), ws_bytes, st)
        if self_join:
            lib.check(L.mmr_gallery_self_join(g_.data_ptr(), lib.ptr(hi), lib.dtype_code(dtype), n, E, *common))
        else:
            lib.check(L.mmr_cosine_range(q_.data_ptr(), g_.data_ptr(), lib.ptr(hi), lib.dtype_code(dtype), nq, n, E, *common))
        torch.cuda.synchronize(device)
        assert 0 < int(counts[0]) <= int(counts[1]) <= CAND_CAP
        return oa, ob, sc, d64, counts
    return run


def _split(L, lib, device, g_, with_resid):
    n = g_.shape[0]
    hi = torch.empty(n, E, dtype=torch.bfloat16, device=device)
    lo = torch.empty_like(hi)
    resid = torch.empty(1, dtype=torch.float32, device=device) if with_resid else None
    lib.check(L.mmr_gallery_split_bf16(g_.data_ptr(), n, E, hi.data_ptr(), lo.data_ptr(), lib.ptr(resid), lib.stream_ptr(device)))
    return hi, lo, resid


def _sweep(L, lib, device, qd, gd, dtype, hi_given):
    nq, n = qd.shape[0], gd.shape[0]
    q_, g_ = qd.to(dtype), gd.to(dtype)
    st = lib.stream_ptr(device)
    hi = _split(L, lib, device, g_, False)[0] if hi_given else None      # no residual bound: the margin falls back to 2^-8 G
    labels = (torch.arange(n, dtype=torch.int32) % 3).to(device)
    targets = (torch.arange(nq, dtype=torch.int32) % 3).to(device)
    thr = torch.linspace(-0.2, 1.0, SWEEP_T, dtype=torch.float64)            # host array
    ws_bytes = L.mmr_sweep_workspace_bytes(n, E, nq, SWEEP_T, SWEEP_CAND_CAP, lib.dtype_code(dtype), int(hi_given))

    def run(fill):
        ws = torch.full((ws_bytes,), fill, dtype=torch.uint8, device=device)
        ge = torch.full((nq, 2, SWEEP_T), -7, dtype=torch.int64, device=device)
        total = torch.full((nq, 2), -7, dtype=torch.int64, device=device)
        counts = torch.full((2,), -7, dtype=torch.int64, device=device)
        lib.check(L.mmr_threshold_sweep(q_.data_ptr(), g_.data_ptr(), lib.ptr(hi), lib.dtype_code(dtype), nq, n, E,
                                        labels.data_ptr(), targets.data_ptr(), thr.data_ptr(), SWEEP_T, 0.0, None, None, None,
                                        SWEEP_CAND_CAP, ge.data_ptr(), total.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                        ws_bytes, st))
        torch.cuda.synchronize(device)
        assert 0 <= int(counts[0]) == int(counts[1]) <= SWEEP_CAND_CAP           # no overflow: every candidate was rechecked
        assert int(total.sum()) == nq * n
        return ge, total, counts
    return run


def _deep(L, lib, device, qd, gd, dtype, hi_given):
    nq, n = qd.shape[0], gd.shape[0]
    q_, g_ = qd.to(dtype), gd.to(dtype)
    st = lib.stream_ptr(device)
    hi, lo, resid = _split(L, lib, device, g_, True) if hi_given else (None, None, None)
    ws_bytes = L.mmr_deep_topk_workspace_bytes(n, E, nq, DEEP_K, DEEP_CAP, DEEP_CAP, lib.dtype_code(dtype), int(hi_given))

    def run(fill):
        ws = torch.full((ws_bytes,), fill, dtype=torch.uint8, device=device)
        idx = torch.full((nq, DEEP_K), -7, dtype=torch.int64, device=device)
        score = torch.full((nq, DEEP_K), -7.0, dtype=torch.float32, device=device)
        d64 = torch.full((nq, DEEP_K), -7.0, dtype=torch.float64, device=device)
        counts = torch.full((2,), -7, dtype=torch.int64, device=device)
        lib.check(L.mmr_cosine_topk_deep(q_.data_ptr(), g_.data_ptr(), lib.ptr(hi), lib.ptr(lo), lib.ptr(resid),
                                         lib.dtype_code(dtype), nq, n, E, DEEP_K, 100.0, 0.0, None, None, DEEP_CAP, DEEP_CAP,
                                         idx.data_ptr(), score.data_ptr(), d64.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                         ws_bytes, st))
        torch.cuda.synchronize(device)
        assert 0 < int(counts[0]) <= DEEP_CAP and nq * DEEP_K <= int(counts[1]) <= DEEP_CAP
        return idx, score, d64, counts
    return run


CASES = {
    "topk_ex bf16": lambda L, lib, dev, q, g: _topk(L, lib, dev, q, g, torch.bfloat16, False),
    "topk_ex fp32": lambda L, lib, dev, q, g: _topk(L, lib, dev, q, g, torch.float32, False),
    "topk_split": lambda L, lib, dev, q, g: _topk(L, lib, dev, q, g, torch.float32, True),
    "range fp32, split in the call": lambda L, lib, dev, q, g: _range(L, lib, dev, q, g, torch.float32, False, False),
    "range fp32, hi given, no residual bound": lambda L, lib, dev, q, g: _range(L, lib, dev, q, g, torch.float32, False, True),
    "self_join bf16": lambda L, lib, dev, q, g: _range(L, lib, dev, q, g, torch.bfloat16, True, False),
    "self_join fp32": lambda L, lib, dev, q, g: _range(L, lib, dev, q, g, torch.float32, True, False),
    "sweep bf16": lambda L, lib, dev, q, g: _sweep(L, lib, dev, q, g, torch.bfloat16, False),
    "sweep fp16": lambda L, lib, dev, q, g: _sweep(L, lib, dev, q, g, torch.float16, False),
    "sweep fp32, split in the call": lambda L, lib, dev, q, g: _sweep(L, lib, dev, q, g, torch.float32, False),
    "sweep fp32, hi given, no residual bound": lambda L, lib, dev, q, g: _sweep(L, lib, dev, q, g, torch.float32, True),
    "deep bf16": lambda L, lib, dev, q, g: _deep(L, lib, dev, q, g, torch.bfloat16, False),
    "deep fp32 unsplit": lambda L, lib, dev, q, g: _deep(L, lib, dev, q, g, torch.float32, False),
    "deep fp32, hi given": lambda L, lib, dev, q, g: _deep(L, lib, dev, q, g, torch.float32, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_outputs_do_not_depend_on_workspace_contents(device, data, case):
    from mmr_amd import _lib
    gd, qd = data
    run = CASES[case](_lib.lib(), _lib, device, qd, gd)
    zero, ones = run(0x00), run(0xFF)
    for i, (a, b) in enumerate(zip(zero, ones)):
        assert torch.equal(_bits(a), _bits(b)), (case, "output", i)
