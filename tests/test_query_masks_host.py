"""CPU: the per-query-mask calls' host side -- exported symbols, argument checks that return before any launch, the Python
front end's ValueErrors and the mask builders' packing.  No GPU: pointers given to the C calls are never dereferenced
(the checks return first, as in test_row_mask_isa.py) and the Python checks see meta / CPU tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

NEW = ("mmr_cosine_topk_deep_qmasked", "mmr_deep_topk_qmasked_workspace_bytes", "mmr_threshold_sweep_qmasked", "mmr_row_masks_pack")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def test_new_symbols_are_exported_and_declared(lib):
    L = lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.HEADER.functions, name
    assert L.mmr_version() == 1


def _deep(L, row_masks=16, stride=4, row_mask=None, dtype=1, E=512, k=10, hi=None, N=100, ws=16, ws_bytes=1 << 30):
    return L.mmr_cosine_topk_deep_qmasked(16, 16, hi, None, None, dtype, 4, N, E, k, 1.0, 1.0, None, row_masks, stride, row_mask, 8, 8,
                                          16, 16, None, 16, ws, ws_bytes, 0)


def _sweep(L, row_masks=16, stride=4, row_mask=None, E=512, N=100):
    thr = (ctypes.c_double * 2)(0.1, 0.2)
    return L.mmr_threshold_sweep_qmasked(16, 16, None, 1, 4, N, E, 16, 16, thr, 2, 1.0, None, None, row_masks, stride, row_mask, 8, 16,
                                         16, 16, 16, 1 << 30, 0)


@pytest.mark.parametrize("call", [_deep, _sweep], ids=["deep", "sweep"])
def test_c_abi_checks_the_masks_before_any_launch(lib, call):
    L = lib.lib()
    assert call(L, row_masks=18) == -22 and b"row_masks" in L.mmr_last_error()          # misaligned
    assert call(L, row_masks=None) == -22 and b"row_masks" in L.mmr_last_error()        # missing
    assert call(L, stride=3) == -22 and b"mask_stride" in L.mmr_last_error()            # ceil(100 / 32) = 4 words
    assert call(L, stride=-1) == -22 and b"mask_stride" in L.mmr_last_error()
    assert call(L, row_mask=18) == -22 and b"row_mask" in L.mmr_last_error()            # the shared mask's alignment
    assert call(L, E=1024) == -95                                                       # no MFMA scan at E = 1024
    assert call(L, E=100) == -95


def test_c_abi_deep_specifics(lib):
    L = lib.lib()
    assert _deep(L, dtype=0) == -22 and b"gallery_hi" in L.mmr_last_error()             # fp32 needs the split
    assert _deep(L, k=0) == -22 and _deep(L, k=4097) == -22
    assert _deep(L, ws=None) == -22
    assert _deep(L, ws_bytes=16) == -28                                                 # MMR_ENOSPC: every check passed, no launch yet
    assert L.mmr_deep_topk_qmasked_workspace_bytes(1000, 512, 4, 10, 8, 8, 0, 0) == 0   # fp32 without a split: refused
    assert L.mmr_deep_topk_qmasked_workspace_bytes(1000, 1024, 4, 10, 8, 8, 1, 0) == 0
    for dt, split in ((1, 0), (2, 0), (0, 1)):
        assert L.mmr_deep_topk_qmasked_workspace_bytes(1000, 512, 4, 10, 8, 8, dt, split) > 0
    # more queries leave room for fewer tiles' mask words per task: the per-query plan needs more task maxima, never fewer
    args = (4_000_000, 768, 128, 10, 64, 64, 1, 0)
    assert L.mmr_deep_topk_qmasked_workspace_bytes(*args) > L.mmr_deep_topk_workspace_bytes(*args) > 0


def test_c_abi_row_masks_pack_checks(lib):
    L = lib.lib()
    assert L.mmr_row_masks_pack(16, None, 5, 100, 3, 16, 0) == -22 and b"stride" in L.mmr_last_error()
    assert L.mmr_row_masks_pack(16, None, 5, 100, 4, 18, 0) == -22
    assert L.mmr_row_masks_pack(16, 2, 5, 100, 4, 16, 0) == -22
    assert L.mmr_row_masks_pack(16, None, 5, 100, 4, None, 0) == -22
    assert L.mmr_row_masks_pack(16, None, -1, 100, 4, 16, 0) == -22
    assert L.mmr_row_masks_pack(None, None, 0, 100, 4, None, 0) == 0                    # Q == 0: nothing to do


def test_python_checks_raise_before_any_launch(lib):
    """Wrong shape, dtype, device or Q of row_masks: ValueError on the host.  The gallery is a meta tensor, so nothing could
    be launched even if a check were missing."""
    from mmr_amd import search

    dev = torch.device("cuda:0")
    Q, N, E = 3, 100, 512
    ok = torch.ones(Q, N, dtype=torch.bool, device="meta")
    bad = [torch.ones(Q, N - 1, dtype=torch.bool), torch.ones(Q + 1, N, dtype=torch.bool), torch.ones(N, dtype=torch.bool),
           torch.ones(Q, N, dtype=torch.uint8), ok, [[True] * N] * Q,
           search.DecisionMasks(torch.zeros(Q + 1, 4, dtype=torch.int32), N), search.DecisionMasks(torch.zeros(Q, 4, dtype=torch.int32), N + 64),
           search.DecisionMasks(torch.zeros(Q, 3, dtype=torch.int32), N), search.DecisionMasks(torch.zeros(Q, 4, dtype=torch.int64), N),
           search.DecisionMasks(torch.zeros(Q, 4, dtype=torch.int32), N)]          # right shape, wrong device (CPU)
    for m in bad:
        with pytest.raises(ValueError):
            search._check_row_masks(m, Q, N, E, dev)
    search._check_row_masks(None, Q, N, E, dev)
    search._check_row_masks(ok, Q, N, E, torch.device("meta"))
    search._check_row_masks(search.DecisionMasks(torch.zeros(Q, 4, dtype=torch.int32), N), Q, N, E, torch.device("cpu"))
    with pytest.raises(ValueError, match="status"):
        search._check_row_masks(ok, Q, N, E, torch.device("meta"), return_status=True)
    with pytest.raises(ValueError, match="1024"):
        search._check_row_masks(torch.ones(Q, N, dtype=torch.bool, device="meta"), Q, N, 1024, torch.device("meta"))
    # through the public calls: a meta gallery reaches the checks and nothing else
    g = torch.empty(N, E, dtype=torch.bfloat16, device="meta")
    q = torch.empty(Q, E, dtype=torch.bfloat16, device="meta")
    for m in (torch.ones(Q, N + 1, dtype=torch.bool, device="meta"), torch.ones(Q, N, dtype=torch.bool)):
        with pytest.raises(ValueError, match="row_masks"):
            search.cosine_topk_deep(q, g, 10, row_masks=m)
        with pytest.raises(ValueError, match="row_masks"):
            search.cosine_topk(q, g, 10, row_masks=m)
    with pytest.raises(ValueError, match="status"):
        search.cosine_topk(q, g, 10, return_status=True, row_masks=ok)
    with pytest.raises(ValueError, match="row_mask has shape"):                       # the 1-D keyword still refuses 2-D tensors
        search._check_row_mask(ok, N, torch.device("meta"))


def _pack_np(keep):
    Q, N = keep.shape
    W = max((N + 31) // 32, 1)
    pad = np.zeros((Q, W * 32), np.uint8)
    pad[:, :N] = keep
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint32).reshape(Q, W).view(np.int32)


@pytest.mark.parametrize("N", [1, 31, 32, 33, 1000])
def test_from_bool_and_leave_out_masks_pack_like_numpy(N):
    from mmr_amd import search

    rng = np.random.default_rng(N)
    keep = rng.random((5, N)) < 0.5
    keep[0] = True                                   # bit 31 set: the int32 words go negative
    m = search.DecisionMasks.from_bool(torch.from_numpy(keep))
    assert m.num_rows == N and m.words.dtype == torch.int32
    assert np.array_equal(m.words.numpy(), _pack_np(keep))
    assert np.array_equal(m.to_bool().numpy(), keep)
    n = min(7, N)
    qi, ri = rng.integers(0, 5, n), rng.integers(0, N, n)
    lo = search.leave_out_masks(5, N, qi, ri)
    want = np.ones((5, N), bool)
    want[qi, ri] = False
    assert np.array_equal(lo.words.numpy(), _pack_np(want))
    with pytest.raises(ValueError):
        search.leave_out_masks(5, N, [5], [0])
    with pytest.raises(ValueError):
        search.leave_out_masks(5, N, [0], [N])
    with pytest.raises(ValueError):
        search.leave_out_masks(5, N, [0, 1], [0])
    with pytest.raises(ValueError):
        search.DecisionMasks.from_bool(torch.ones(5, N, dtype=torch.uint8))
