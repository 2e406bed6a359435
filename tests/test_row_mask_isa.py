"""CPU: the row-mask (filtered search) kernels, checked without a GPU.

1. ISA: search.hip and range.hip compiled with `hipcc -S` for gfx950.  The scan kernels' LDS ring and k-loops run on
   hand-counted `s_waitcnt vmcnt(N)` / `lgkmcnt(N)`; a load added inside the ring breaks those counts.  For every scan
   kernel the MASKED instantiation must emit the same global_load_lds instructions and the same counted waits (the
   ring's wait in front of its s_barrier, the k-loops' waits in front of their MFMAs) as the unmasked one; its only
   added loads are the mask words.  Neither form may spill to memory.
2. Host argument checks: a wrong mask length, dtype or device raises before any launch, and the C ABI rejects a
   misaligned mask pointer on the host.
"""
import collections
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-modal-retrieval-system-image-search-and-data-governance_amd", "csrc")

# mangled-name prefixes of the scan kernels that take the MASKED flag (their last template argument); the 16-bit ones are
# templates over the element type, their first argument: t = uint16_t = bf16_t, all these two translation units hold
SCAN_KERNELS = ("_ZN3mmr11scan_kernelIt", "_ZN3mmr13scan16_kernelIt", "_ZN3mmr16scan_f32s_kernelI",
                "_ZN3mmr17scan_split_kernelI", "_ZN3mmr17range_scan_kernelIt")


def _compile(src, out):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-Wno-unused-result",
                             "-Wno-unused-value", "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out],
                            stderr=subprocess.DEVNULL)


def _parse(text):
    """-> ({kernel: [instruction, ...]}, {kernel: (private segment bytes, sgpr spills, vgpr spills)})"""
    kernels, cur = {}, None
    for ln in text.splitlines():
        t = ln.strip()
        if ln and not ln[0].isspace() and t.startswith("_Z") and ":" in t:
            cur = t.split(":")[0]
            kernels[cur] = []
        elif t.startswith(".Lfunc_end"):
            cur = None
        elif cur and t and not t.startswith((";", ".")):
            kernels[cur].append(t)
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)\n\s+\.sgpr_count:\s+\d+\n"
                         r"\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n){0,4}?\s+\.vgpr_spill_count:\s+(\d+)", text):
        meta[m.group(1)] = tuple(int(x) for x in m.group(2, 3, 4))
    return kernels, meta


@pytest.fixture(scope="module")
def isa():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as td:
        outs = {s: os.path.join(td, s + ".s") for s in ("search.hip", "range.hip")}
        procs = [_compile(s, o) for s, o in outs.items()]
        assert all(p.wait() == 0 for p in procs), "hipcc -S failed"
        kernels, meta = {}, {}
        for o in outs.values():
            k, m = _parse(open(o).read())
            kernels.update(k)
            meta.update(m)
    return kernels, meta


def _pairs(kernels):
    """(masked name, unmasked name) of every scan kernel: the MASKED flag is the last template argument"""
    out = []
    for name in kernels:
        if name.startswith(SCAN_KERNELS) and "Lb1EEEv" in name:
            i = name.rindex("Lb1EEEv")
            twin = name[:i] + "Lb0EEEv" + name[i + len("Lb1EEEv"):]
            assert twin in kernels, name
            out.append((name, twin))
    return out


def _mnemonics(instrs, pred):
    return [i.split()[0] for i in instrs if pred(i.split()[0])]


def test_every_scan_kernel_has_a_masked_twin(isa):
    kernels, _ = isa
    pairs = _pairs(kernels)
    # scan_kernel x3 (E 128/256/512), scan16 x1 (768), scan_f32s x4, scan_split x4, range_scan x (4 E x 2 forms)
    assert len(pairs) == 3 + 1 + 4 + 4 + 8, sorted(p[0] for p in pairs)


def _ring_waits(instrs):
    """The hand-counted waits: the ring's `s_waitcnt vmcnt(N)` in front of its s_barrier (the last vmcnt wait before it)
    and the k-loops' counted `s_waitcnt lgkmcnt(N)`, N > 0 (the compiler's own LDS / scalar waits are lgkmcnt(0))."""
    out = []
    for n, ins in enumerate(instrs):
        op = ins.split()[0]
        if op == "s_barrier":
            for back in instrs[max(0, n - 16):n][::-1]:
                if back.startswith("s_waitcnt") and "vmcnt" in back:
                    out.append(back + " -> s_barrier")
                    break
        elif op == "s_waitcnt" and "lgkmcnt" in ins and "lgkmcnt(0)" not in ins:
            out.append(ins)
    return collections.Counter(out)


def test_masked_scans_keep_the_ring_and_waits_of_the_unmasked_ones(isa):
    kernels, _ = isa
    for masked, plain in _pairs(kernels):
        a, b = kernels[masked], kernels[plain]
        is_glds = lambda m: m.startswith("global_load_lds")
        assert collections.Counter(_mnemonics(a, is_glds)) == collections.Counter(_mnemonics(b, is_glds)), masked
        assert _ring_waits(a) == _ring_waits(b), (masked, _ring_waits(a) - _ring_waits(b), _ring_waits(b) - _ring_waits(a))
        assert any(w.endswith("s_barrier") for w in _ring_waits(a)), masked
        # the additions: one vector load of the tiles' mask words (two in the self-join: the query row's word), no scalar
        # load but the row_mask kernel argument
        is_gload = lambda m: m.startswith(("global_load", "buffer_load", "flat_load")) and not m.startswith("global_load_lds")
        extra = len(_mnemonics(a, is_gload)) - len(_mnemonics(b, is_gload))
        assert extra == (2 if "Lb1ELb1EEEv" in masked else 1), (masked, extra)
        is_sload = lambda m: m.startswith(("s_load", "s_buffer_load"))
        assert len(_mnemonics(a, is_sload)) <= len(_mnemonics(b, is_sload)) + 1, masked


def test_scan_kernels_do_not_spill(isa):
    kernels, meta = isa
    for masked, plain in _pairs(kernels):
        for name in (masked, plain):
            assert name in meta, name
            scratch, _, vgpr_spills = meta[name]
            assert scratch == 0 and vgpr_spills == 0, (name, meta[name])
        # SGPR spills go to VGPR lanes, not memory; the masked form adds none
        assert meta[masked][1] <= meta[plain][1], (masked, meta[masked], meta[plain])


# ------------------------------------------------------------------ host argument checks (no launch, no GPU)
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def test_c_abi_rejects_a_misaligned_mask_before_any_launch(lib):
    L = lib.lib()
    # pointers are never dereferenced: the checks return first
    rc = L.mmr_cosine_topk_masked(16, 16, 1, 4, 100, 512, 10, 1.0, 1.0, None, 18, 16, 16, 0, 0, 16, 1 << 30, 0)
    assert rc == -22 and b"row_mask" in L.mmr_last_error()
    rc = L.mmr_cosine_topk_split_masked(16, 16, 16, 16, None, 4, 100, 512, 10, 1.0, 1.0, None, 2, 16, 16, 0, 0, 16, 1 << 30, 0)
    assert rc == -22 and b"row_mask" in L.mmr_last_error()
    rc = L.mmr_cosine_range_masked(16, 16, None, 1, 4, 100, 512, 0.5, 1.0, 1.0, None, None, 1, 8, 8, 16, 16, 16, 16, 16, 16,
                                   1 << 30, 0)
    assert rc == -22 and b"row_mask" in L.mmr_last_error()
    rc = L.mmr_gallery_self_join_masked(16, None, 1, 100, 512, 0.5, 1.0, 1.0, None, None, 3, 8, 8, 16, 16, 16, 16, 16, 16,
                                        1 << 30, 0)
    assert rc == -22 and b"row_mask" in L.mmr_last_error()
    assert L.mmr_row_mask_pack(16, 2, 100, 16, 0) == -22
    assert L.mmr_row_mask_pack(16, None, 100, 18, 0) == -22
    assert L.mmr_row_mask_pack(None, None, 0, None, 0) == 0          # N == 0: nothing to do
    assert L.mmr_version() == 1


def test_python_mask_checks_raise_before_any_launch(lib):
    """Wrong length, dtype or device of row_mask: ValueError on the host (these tensors never reach a kernel; the
    gallery is a meta tensor, so nothing could be launched even if a check were missing)."""
    from mmr_amd import search

    for bad in (torch.ones(99, dtype=torch.bool), torch.ones(100, dtype=torch.uint8), torch.ones(100, 1, dtype=torch.bool),
                torch.ones(100, dtype=torch.bool, device="meta")):
        with pytest.raises(ValueError):
            search._check_row_mask(bad, 100, torch.device("cuda:0"))
    with pytest.raises(ValueError):
        search._check_row_mask([True] * 100, 100, torch.device("cuda:0"))
    search._check_row_mask(None, 100, torch.device("cuda:0"))     # no mask: nothing to check
