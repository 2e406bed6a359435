"""CPU: the deep top-k's C ABI and Python argument checks (mmr_cosine_topk_deep, cosine_topk_deep, GalleryIndex.search_deep).

Every C call below returns on the host before any launch, so the library is exercised without a GPU."""
import os

import pytest
import torch

import mmr_amd
from mmr_amd import _lib as lib

BF16, F32 = 1, 0


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(lib.LIB_PATH):
        pytest.fail(f"{lib.LIB_PATH} missing: run __graft_entry__.build() first")
    return lib.lib()


def _deep(L, q=16, g=16, dtype=BF16, Q=4, N=100, E=512, k=10, scale=1.0, bound=1.0, tile_cap=64, surv_cap=64, idx=16, score=16,
          counts=16, ws=16, ws_bytes=1 << 30):
    return L.mmr_cosine_topk_deep(q, g, 0, 0, 0, dtype, Q, N, E, k, scale, bound, 0, 0, tile_cap, surv_cap, idx, score, 0, counts,
                                  ws, ws_bytes, 0)


def test_header_declares_and_library_exports_the_deep_calls(L):
    assert lib.HEADER.constants["MMR_DEEP_K_MAX"] == 4096
    for name in ("mmr_deep_topk_workspace_bytes", "mmr_cosine_topk_deep"):
        assert name in lib.HEADER.functions, name
        assert hasattr(L, name), name
    assert "cosine_topk_deep" in mmr_amd.__all__
    assert callable(mmr_amd.cosine_topk_deep) and callable(mmr_amd.GalleryIndex.search_deep)
    from mmr_amd import search
    assert search.DEEP_K_MAX == 4096


def test_deep_argument_validation_happens_before_any_launch(L):
    assert _deep(L, k=0) == -22 and b"k=0" in L.mmr_last_error()
    assert _deep(L, k=4097) == -22 and b"k=4097" in L.mmr_last_error()
    assert _deep(L, k=4096, ws_bytes=8) == -28                      # k = 4096 itself is accepted: it gets as far as the workspace
    assert _deep(L, E=100) == -95 and b"E=100" in L.mmr_last_error()
    assert _deep(L, E=1024) == -95 and b"E=1024" in L.mmr_last_error()
    assert _deep(L, scale=0.0) == -22 and b"scale" in L.mmr_last_error()
    assert _deep(L, scale=-1.0) == -22 and b"scale" in L.mmr_last_error()
    assert _deep(L, scale=float("inf")) == -22 and b"scale" in L.mmr_last_error()
    assert _deep(L, dtype=7) == -22 and b"dtype" in L.mmr_last_error()
    assert _deep(L, bound=float("nan")) == -22 and b"gallery_norm_bound" in L.mmr_last_error()
    assert _deep(L, ws=0) == -22 and b"workspace" in L.mmr_last_error()
    assert _deep(L, ws_bytes=8) == -28 and b"workspace" in L.mmr_last_error()
    assert _deep(L, tile_cap=0) == -22 and b"tile_cap" in L.mmr_last_error()
    assert _deep(L, surv_cap=0) == -22 and b"surv_cap" in L.mmr_last_error()
    assert _deep(L, q=0) == -22 and b"null" in L.mmr_last_error()
    assert _deep(L, counts=0) == -22 and b"null" in L.mmr_last_error()
    assert _deep(L, q=8) == -22 and b"aligned" in L.mmr_last_error()
    assert _deep(L, N=1 << 31) == -22 and b"int32" in L.mmr_last_error()
    assert _deep(L, Q=-1) == -22
    # Q == 0: nothing to do, whatever the pointers
    assert _deep(L, Q=0, q=0, g=0, idx=0, score=0, counts=0, ws=0, ws_bytes=0) == 0
    # the old calls keep their limit
    assert L.mmr_cosine_topk(16, 16, 1, 4, 100, 512, 65, 1.0, 1.0, 16, 16, 0, 0, 16, 1 << 30, 0) == -22
    assert b"k=65" in L.mmr_last_error()


def test_deep_workspace_size(L):
    W = L.mmr_deep_topk_workspace_bytes
    base = W(1_000_000, 512, 16, 1000, 40_000, 40_000, BF16, 0)
    assert base > 0
    assert W(1_000_000, 512, 16, 1000, 80_000, 40_000, BF16, 0) >= base + 8 * 40_000        # 8 bytes per listed pair
    assert W(1_000_000, 512, 16, 1000, 40_000, 80_000, BF16, 0) >= base + 32 * 40_000       # 32 bytes per survivor
    # the bucket maxima: one float per (tile, query of a pass) -- 16-row tiles for an unsplit fp32 gallery
    assert base >= 4 * 31250 * 32
    assert W(1_000_000, 512, 16, 1000, 40_000, 40_000, F32, 0) >= base + 4 * 31250 * 32
    # a split fp32 index holds the bf16 copy of the queries
    assert W(1_000_000, 512, 16, 1000, 40_000, 40_000, F32, 1) >= base + 16 * 512 * 2
    assert base < 64e6
    for bad in ((-1, 512, 16, 10, 1, 1, BF16, 0), (100, 1024, 16, 10, 1, 1, BF16, 0), (100, 512, 16, 0, 1, 1, BF16, 0),
                (100, 512, 16, 4097, 1, 1, BF16, 0), (100, 512, 16, 10, 0, 1, BF16, 0), (100, 512, 16, 10, 1, 0, BF16, 0),
                (100, 512, 16, 10, 1, 1, 7, 0)):
        assert W(*bad) == 0, bad


def test_python_checks_run_before_the_device_is_touched():
    from mmr_amd import search
    g = torch.zeros(40, 128)
    q = torch.zeros(3, 128)
    with pytest.raises(ValueError, match="query dim"):
        search.cosine_topk_deep(torch.zeros(3, 256), g, 10)
    for k in (0, -1, 4097, 2.5):
        with pytest.raises(ValueError, match="outside"):
            search.cosine_topk_deep(q, g, k)
    with pytest.raises(ValueError, match="row_mask"):
        search.cosine_topk_deep(q, g, 10, row_mask=torch.ones(39, dtype=torch.bool))
    with pytest.raises(ValueError, match="row_mask"):
        search.cosine_topk_deep(q, g, 10, row_mask=torch.ones(40, dtype=torch.int32))
    with pytest.raises(ValueError, match="row_mask"):
        search.cosine_topk_deep(q, g, 10, row_mask=[True] * 40)
    with pytest.raises(ValueError, match="1-D or 2-D"):
        search.cosine_topk_deep(torch.zeros(1, 3, 128), g, 10)
    # valid arguments get as far as the device check: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        search.cosine_topk_deep(q, g, 100)
    # the old call still refuses k = 65 in the library, not in Python: its signature and docstring only gained a pointer
    assert "cosine_topk_deep" in search.cosine_topk.__doc__ and "search_deep" in search.GalleryIndex.search.__doc__
