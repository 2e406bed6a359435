"""CPU: the fp16 dtype at the host boundary -- the dtype code, the workspace plans and the argument checks, no launch.

An fp16 gallery has the bf16 gallery's layout, so every plan for dtype 2 (MMR_F16) equals the plan for dtype 1."""
import os

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def test_dtype_code_of_float16(lib):
    assert lib.dtype_code(torch.float32) == 0 and lib.dtype_code(torch.bfloat16) == 1
    assert lib.dtype_code(torch.float16) == 2
    with pytest.raises(TypeError):
        lib.dtype_code(torch.float64)


@pytest.mark.parametrize("E", [128, 256, 512, 768])
def test_fp16_workspace_plans_equal_the_bf16_plans(lib, E):
    L = lib.lib()
    N, Q = 100003, 37
    for hi_given in (0, 1):
        a, b = L.mmr_range_workspace_bytes(N, E, Q, 1 << 16, 2, hi_given), L.mmr_range_workspace_bytes(N, E, Q, 1 << 16, 1, hi_given)
        assert a == b and a > 0
        a, b = L.mmr_sweep_workspace_bytes(N, E, Q, 200, 1 << 16, 2, hi_given), L.mmr_sweep_workspace_bytes(N, E, Q, 200, 1 << 16, 1, hi_given)
        assert a == b and a > 0
        a = L.mmr_deep_topk_workspace_bytes(N, E, Q, 1000, 1 << 16, 1 << 16, 2, hi_given)
        b = L.mmr_deep_topk_workspace_bytes(N, E, Q, 1000, 1 << 16, 1 << 16, 1, hi_given)
        assert a == b and a > 0
    # the fp32 plans differ (query copies, 16-row tiles): dtype 2 did not fall into the fp32 branch
    assert L.mmr_sweep_workspace_bytes(N, E, Q, 200, 1 << 16, 2, 1) != L.mmr_sweep_workspace_bytes(N, E, Q, 200, 1 << 16, 0, 1)


def test_dtype_3_is_still_rejected(lib):
    L = lib.lib()
    assert L.mmr_range_workspace_bytes(1000, 512, 4, 1 << 16, 3, 0) == 0
    assert L.mmr_sweep_workspace_bytes(1000, 512, 4, 200, 1 << 16, 3, 0) == 0
    assert L.mmr_deep_topk_workspace_bytes(1000, 512, 4, 100, 1 << 16, 1 << 16, 3, 0) == 0
    # pointers are never dereferenced: the dtype check returns first
    rc = L.mmr_cosine_topk_masked(16, 16, 3, 4, 100, 512, 10, 1.0, 1.0, None, 16, 16, 16, 0, 0, 16, 1 << 30, 0)
    assert rc == -22 and b"dtype" in L.mmr_last_error()
    rc = L.mmr_cosine_range_masked(16, 16, None, 3, 4, 100, 512, 0.5, 1.0, 1.0, None, None, 16, 8, 8, 16, 16, 16, 16, 16, 16,
                                   1 << 30, 0)
    assert rc == -22 and b"dtype" in L.mmr_last_error()
    rc = L.mmr_gallery_norm_bound(16, 3, 100, 512, 16, 0)
    assert rc == -22 and b"dtype" in L.mmr_last_error()
    rc = L.mmr_l2norm_rows(16, 3, 4, 512, 0)
    assert rc == -22 and b"dtype" in L.mmr_last_error()
    # dtype 2 passes the dtype check and fails on the next one (a misaligned mask), before any launch
    rc = L.mmr_cosine_topk_masked(16, 16, 2, 4, 100, 512, 10, 1.0, 1.0, None, 18, 16, 16, 0, 0, 16, 1 << 30, 0)
    assert rc == -22 and b"row_mask" in L.mmr_last_error()


def test_version_is_unchanged(lib):
    assert lib.lib().mmr_version() == 1


def test_model_wrappers_take_float16_as_an_output_dtype():
    """CLIP._set_dtype / BertTextEncoder._set_dtype accept float16 (the methods touch no device state)."""
    from mmr_amd.bert import BertTextEncoder
    from mmr_amd.clip import CLIP

    for cls in (CLIP, BertTextEncoder):
        m = cls.__new__(cls)
        m._dtype = torch.float32
        assert cls.half(m) is m and m.dtype == torch.float16
        assert cls.to(m, torch.bfloat16) is m and m.dtype == torch.bfloat16
        assert cls.to(m, dtype=torch.float16).dtype == torch.float16
        assert cls.float(m).dtype == torch.float32
        with pytest.raises(TypeError):
            cls._set_dtype(m, torch.float64)
