"""CPU: host-side parts of the pooled-row last block -- the workspace plan and the switch -- and the ISA of its attention
kernels (no spills, compiler-counted waits only)."""
import ctypes
import os
import subprocess
import sys

import pytest

import mmr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def _tower(L, cfg, fold=False):
    """A tower handle over a blob that is never read (no launch happens in these tests)."""
    from mmr_amd.clip import _tower_cfg_struct
    c = _tower_cfg_struct(cfg, fold)
    h = ctypes.c_void_p()
    assert L.mmr_tower_create(ctypes.byref(c), 256, 1 << 40, ctypes.byref(h)) == 0
    return h


def test_workspace_plan_adds_the_compact_buffers_only_past_the_gate(lib):
    L = lib.lib()
    cfg = mmr_amd.get_config("ViT-B/32").vision                     # T = 50, d = 768, mlp = 3072
    t = _tower(L, cfg)
    ws = lambda b: L.mmr_tower_workspace_bytes(t, b)
    # 40 images pad to 2 048 token rows (the full path's plan); 41 images to 2 176, with the same 2 048 patch rows.
    # Per padded token row h (4d) + x (2d) + wide (2 mlp); the compact buffers are picks + xg, qc, oc (bf16 d) +
    # hc (fp32 d) + mc (bf16 mlp) for 128 pooled rows
    per_row = 4 * 768 + 2 * 768 + 2 * 3072
    compact = 128 * (4 + 3 * 2 * 768 + 4 * 768 + 2 * 3072)
    grown = ws(41) - ws(40)
    assert grown >= 128 * per_row + compact
    assert grown < 128 * (per_row + 4 * 768) + compact + 16 * 256   # + patch rows, alignment
    # the folded-LayerNorm mode keeps its plan: growth there has no compact part
    tf = _tower(L, cfg, fold=True)
    wf = lambda b: L.mmr_tower_workspace_bytes(tf, b)
    assert wf(41) - wf(40) < grown - compact + 128 * (2 * 768 + 16 * 8) + 16 * 256
    # the switch changes no size: it may be flipped after the workspace was allocated
    assert L.mmr_tower_set_full_last_block(t, 1) == 0 and ws(41) - ws(40) == grown
    assert L.mmr_tower_set_full_last_block(t, 0) == 0
    assert L.mmr_tower_set_full_last_block(None, 1) == -22 and b"null tower" in L.mmr_last_error()
    L.mmr_tower_destroy(t)
    L.mmr_tower_destroy(tf)


def test_environment_variable_sets_the_initial_value_without_changing_sizes():
    """MMR_FULL_LAST_BLOCK=1 is read when a tower is created; a child process so this one's environment stays as it is."""
    code = ("import ctypes, mmr_amd\n"
            "from mmr_amd import _lib\n"
            "from mmr_amd.clip import _tower_cfg_struct\n"
            "L = _lib.lib()\n"
            "c = _tower_cfg_struct(mmr_amd.get_config('ViT-B/32').vision, False)\n"
            "h = ctypes.c_void_p()\n"
            "assert L.mmr_tower_create(ctypes.byref(c), 256, 1 << 40, ctypes.byref(h)) == 0\n"
            "print(L.mmr_tower_workspace_bytes(h, 256))\n")
    sizes = []
    for val in ("0", "1"):
        env = dict(os.environ, MMR_FULL_LAST_BLOCK=val, PYTHONPATH=ROOT)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
        assert out.returncode == 0, out.stderr
        sizes.append(int(out.stdout.split()[-1]))
    assert sizes[0] == sizes[1] > 0


def test_pooled_attention_kernels_isa():
    """attn_pool_kernel / attn_pool_stream_kernel: no scratch, four 8-byte output stores per wave, and no hand-counted
    vmcnt wait (their loads are plain C++, so the compiler's counters cover them)."""
    from test_host_logic import _kernel_isa
    v = _kernel_isa("attention.hip")
    short = {k: ins for k, ins in v.items() if "attn_pool_kernel" in k}
    stream = {k: ins for k, ins in v.items() if "attn_pool_stream_kernel" in k}
    assert len(short) == 6 and len(stream) == 2                      # NT in {2,4,6} x {plain, causal}; {plain, causal}
    for name, ins in {**short, **stream}.items():
        stores = [i for i in ins if i.startswith("global_store")]
        assert len(stores) == 4 and all(s == "global_store_dwordx2" for s in stores), (name, stores)
        assert not any(i.startswith("scratch_") for i in ins), name
        assert not any("lds" in i for i in ins if i.startswith("global_load")), name      # no LDS-DMA: nothing to count by hand
        assert any(i.startswith("ds_read_b64_tr_b16") for i in ins), name
    gather = [k for k in _kernel_isa("vit_ops.hip") if "pick_gather_kernel" in k]
    assert len(gather) == 4                                          # widths 128, 512, 768, 1024
