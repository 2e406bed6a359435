"""CPU: the perceptual-hash join kernels, checked without a GPU, in the manner of test_fp16_scan_isa.py.

hash_join.hip is compiled with `hipcc -S` for gfx950.  Every hash_* kernel must run without scratch (private segment 0)
and without SGPR or VGPR spills; hash_join_kernel exists for H = 1..4 x W in (1, 4) x (self, cross); its population
counts are v_bcnt_u32_b32, its wave-uniform rows arrive by scalar loads inside the row loop, and nothing in it is
inline assembly.

The hot loop's VALU count, read from the H = 3, W = 1 self-join (2 rows x 4 columns = 8 pairs a step): per pair and
64-bit word 2 v_xor_b32 + 2 v_bcnt_u32_b32 + 1 v_add3_u32 (the two half-word counts plus minus-the-threshold), per pair
one v_min3_i32 over the three kinds, and per step 4 more min and one v_cmp: 133 VALU instructions for 8 pairs, 16.6 a
pair, 5.5 a pair-word ("hash join", holds the same figures).  test_hot_loop_valu_count pins them.
"""
import collections
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-modal-retrieval-system-image-search-and-data-governance_amd", "csrc")
JOIN = "_ZN3mmr16hash_join_kernelI"


def _parse(text):
    """-> ({kernel: [line, ...]} = instructions, labels and `;;#ASM` marks, {kernel: (private segment bytes, sgpr spills,
    vgpr spills)})"""
    kernels, cur = {}, None
    for ln in text.splitlines():
        t = ln.strip()
        if ln and not ln[0].isspace() and t.startswith("_Z") and ":" in t:
            cur = t.split(":")[0]
            kernels[cur] = []
        elif t.startswith(".Lfunc_end"):
            cur = None
        elif cur and t and (t.startswith((".LBB", ";;#ASM")) or not t.startswith((";", "."))):
            kernels[cur].append(t)
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)\n\s+\.sgpr_count:\s+\d+\n"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n){0,4}?\s+\.vgpr_spill_count:\s+(\d+)", text):
        meta[m.group(1)] = tuple(int(x) for x in m.group(2, 3, 4))
    return kernels, meta


@pytest.fixture(scope="module")
def isa():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed to build the project, and to read its kernels"
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "hash_join.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-Wno-unused-result",
                               "-Wno-unused-value", "--cuda-device-only", "-S", os.path.join(CSRC, "hash_join.hip"), "-o", out],
                              stderr=subprocess.DEVNULL)
        return _parse(open(out).read())


def _ours(kernels):
    return [n for n in kernels if n.startswith("_ZN3mmr") and "hash_" in n]


def _name(H, W, self_join):
    return f"{JOIN}Li{H}ELi{W}ELb{int(self_join)}EEEv"


def _one(kernels, H, W, self_join):
    hits = [n for n in kernels if n.startswith(_name(H, W, self_join))]
    assert len(hits) == 1, (H, W, self_join, hits)
    return hits[0]


def test_the_kernel_set(isa):
    kernels, _ = isa
    for H in (1, 2, 3, 4):
        for W in (1, 4):
            for s in (True, False):
                _one(kernels, H, W, s)
    ours = _ours(kernels)
    assert len([n for n in ours if n.startswith(JOIN)]) == 16
    assert sorted(n for n in ours if not n.startswith(JOIN)) == sorted(
        n for n in ours if n.startswith(("_ZN3mmr16hash_fill_kernel", "_ZN3mmr16hash_emit_kernel")))
    assert len(ours) == 18, ours


def test_no_scratch_and_no_spills(isa):
    kernels, meta = isa
    for name in _ours(kernels):
        assert name in meta, name
        assert meta[name] == (0, 0, 0), (name, meta[name])        # private segment, SGPR spills, VGPR spills


def test_popcounts_scalar_row_loads_and_no_inline_assembly(isa):
    kernels, _ = isa
    for name in _ours(kernels):
        assert not any(i.startswith(";;#ASM") for i in kernels[name]), name
    for name in (n for n in _ours(kernels) if n.startswith(JOIN)):
        ops = collections.Counter(i.split()[0] for i in kernels[name])
        assert ops["v_bcnt_u32_b32"] > 0, name
        assert any(op.startswith("global_atomic_add_x2") for op in ops), (name, "one 64-bit atomic add per wave")
        # the rows of the uniform side: scalar loads inside the row loop, feeding v_xor as SGPR operands
        lo, hi = _hot_loop(kernels[name])
        body = kernels[name][lo:hi]
        assert any(i.startswith("s_load_dword") for i in body), name
        assert any(re.match(r"v_xor_b32\S* v\d+, s\d+, v\d+", i) for i in body), name
        assert not any(i.split()[0].startswith(("global_load", "ds_read", "buffer_load")) for i in body), name


def _hot_loop(lines):
    """[lo, hi) of the row loop's hot path: from the last label in front of the first v_xor_b32 (only the hot path XORs:
    the append path counts a | b and a & b) to the branch that skips the append path, the first one after it"""
    first = next(n for n, i in enumerate(lines) if i.startswith("v_xor_b32"))
    lo = max(n for n in range(first) if lines[n].startswith(".LBB"))
    hi = next(n for n in range(first, len(lines)) if lines[n].startswith("s_cbranch"))
    return lo + 1, hi + 1


def test_hot_loop_valu_count(isa):
    kernels, _ = isa
    for self_join in (True, False):
        lines = kernels[_one(kernels, 3, 1, self_join)]
        lo, hi = _hot_loop(lines)
        body = lines[lo:hi]
        assert body[-1].startswith("s_cbranch_vcc"), body[-1]     # wave-uniform: taken unless some lane has a match
        ops = collections.Counter(i.split()[0] for i in body)
        valu = sum(c for op, c in ops.items() if op.startswith("v_"))
        pairs, words = 2 * 4, 3                                   # RU x HJ_CPL pairs a step, H x W words a pair
        assert ops["v_xor_b32_e32"] == 2 * pairs * words
        assert ops["v_bcnt_u32_b32"] == 2 * pairs * words
        # the docstring's figures: at most 133 VALU a step; a compiler that folds the threshold into the count chain
        # (v_bcnt's addend) would need fewer
        assert valu <= 133, (valu, ops)
        assert valu >= 4 * pairs * words + pairs                  # xor + count per half-word, one min per pair: the floor
