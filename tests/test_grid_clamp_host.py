"""Host: the mmr_debug_grid_cap hook itself and the launch-site table of tests/test_grid_clamp_gpu.py against the sources.

No device is needed: the hook is host state (two atomics in csrc/api_common.cpp) and the table is data."""
import collections
import ctypes
import glob
import os
import re

import pytest

import test_grid_clamp_gpu as G

import mmr_amd

CSRC = os.path.join(os.path.dirname(os.path.abspath(mmr_amd.__file__)), "csrc")


@pytest.fixture(scope="module")
def L():
    from mmr_amd import _lib
    return _lib


def test_negative_cap_is_einval_and_changes_nothing(L):
    lib = L.lib()
    assert lib.mmr_debug_grid_cap(0) >= 0
    assert lib.mmr_debug_grid_cap(3) == 0
    assert lib.mmr_debug_grid_cap(-1) == L.HEADER.constants["MMR_EINVAL"] == -22
    assert b"mmr_debug_grid_cap" in lib.mmr_last_error()
    assert lib.mmr_debug_grid_cap(-(1 << 40)) == -22
    # still 3, still no launch counted: the next valid call reports 0, and so does the one after the restore
    assert lib.mmr_debug_grid_cap(0) == 0
    assert lib.mmr_debug_grid_cap(0) == 0


def test_set_then_restore_counts_nothing_when_nothing_ran(L):
    lib = L.lib()
    for cap in (1, 3, 1 << 40):
        assert lib.mmr_debug_grid_cap(cap) == 0
        assert lib.mmr_debug_grid_cap(0) == 0


def test_binding_is_generated_with_the_documented_signature(L):
    restype, argtypes, names = L.HEADER.functions["mmr_debug_grid_cap"]
    assert restype is ctypes.c_int64 and argtypes == [ctypes.c_int64] and names == ["cap"]
    f = L.lib().mmr_debug_grid_cap
    assert f.restype is ctypes.c_int64 and list(f.argtypes) == [ctypes.c_int64]


def test_context_manager_restores_on_error_and_refuses_nesting(L, monkeypatch):
    """grid_cap() without a device: torch.cuda.synchronize is not reached when the body raises"""
    with pytest.raises(RuntimeError, match="body"):
        with G.grid_cap(3):
            raise RuntimeError("body")
    assert G._SET[0] == 0 and L.lib().mmr_debug_grid_cap(0) == 0
    monkeypatch.setattr(G.torch.cuda, "synchronize", lambda *a: None)
    with G.grid_cap(1) as g:
        with pytest.raises(AssertionError, match="nested"):
            with G.grid_cap(3):
                pass
    assert g.clamped == 0 and G._SET[0] == 0


def _calls_in(text, name):
    """Every `name(...)` in the text with its balanced argument list, as written"""
    out = []
    for m in re.finditer(r"\b" + name + r"\(", text):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        out.append(" ".join(text[m.start():i].split()))
    return out


def test_table_rows_are_the_call_sites_of_the_sources():
    """A plain source grep for the two identifiers: a launch added without a row in the table fails here."""
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(files) > 20
    found = collections.Counter()
    for path in files:
        with open(path) as f:
            text = f.read()
        for name in ("grid_1d", "grid_cap"):
            for expr in _calls_in(text, name):
                found[(os.path.basename(path), expr)] += 1
    table = collections.Counter((s.file, s.expr) for s in G.SITES)
    assert found == table, {"in the sources only": found - table, "in the table only": table - found}
    for s in G.SITES:
        with open(os.path.join(CSRC, s.file)) as f:
            text = f.read()
        assert re.search(r"\b" + s.kernel + r"\b", text), (s.file, s.kernel)
        assert s.per_block >= 1 and s.cap >= 1 and s.call in G.CALLS


def test_the_hand_written_clamps_are_on_the_hook():
    by_file = collections.defaultdict(list)
    for s in G.SITES:
        by_file[s.file].append(s.kernel)
    assert "hash_join_kernel" in by_file["hash_join.hip"]
    assert {"jpeg_idct_kernel", "jpeg_color_kernel"} <= set(by_file["jpeg.hip"])
    assert "decision_counts_kernel" in by_file["decide.hip"]
    assert "im2col_kernel" in by_file["vit_ops.hip"]
    assert "tip_grid_cache_kernel" in by_file["tip_grid.hip"]
    assert "deep_list_kernel" in by_file["deep_topk.hip"]


def test_every_call_counts_at_least_its_sites():
    """CALLS[call] is no smaller than the number of table rows that name the call: each of those launches at least once"""
    rows = collections.Counter(s.call for s in G.SITES)
    for call, n in rows.items():
        # range_split_hi runs for fp32 galleries only: the fp32 cases ask for one launch more than CALLS
        assert G.CALLS[call] >= n - (1 if call == "mmr_cosine_range" else 0), (call, n)
    assert all(n >= 1 for n in G.CALLS.values())


def test_the_shapes_bind_a_cap_of_three():
    """The arithmetic of condition 3, without a device: ceil(items / per_block) > 3 at the shapes the GPU tests use"""
    b = G.blocks
    assert b(1003, 4) == 251 and b(G.N_ROWS, 256) == 17 and b(G.N_ROWS, 16) == 257 and b(G.N_ROWS, 4) == 1025
    assert b(G.RANGE_CAP, 256) == 5 and b(G.RANGE_CAP, 16) == 69 and b(G.HASH_CAP, 256) == 5
    assert b(1200, 256) == 5 and b(7 * 300, 256) == 9 and b(300 * 300, 256) == 352
    assert b(b(G.DEEP_N, 32), 64) == 25 and b(b(G.DEEP_N, 32), 8) == 196
    assert all(x % 3 for x in (251, 17, 257, 1025, 5, 352, 25, 196)), "three divides none of them: the last pass is ragged"
