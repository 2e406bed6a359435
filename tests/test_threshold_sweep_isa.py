"""CPU: the threshold-sweep kernels' ISA, checked without a GPU (the way test_row_mask_isa.py checks the other scans).

sweep.hip compiled with `hipcc -S` for gfx950.  sweep_scan_kernel runs range_scan_kernel's LDS ring and k-loop on
hand-counted `s_waitcnt vmcnt(N)` / `lgkmcnt(N)`; its labels, grid and counts are loaded once, before the ring.  Every
instantiation must have a masked twin that emits the same global_load_lds instructions and the same counted waits, one
extra vector load (the mask words) and no extra scalar load beyond the kernel argument.  No kernel of the file spills.
The 160 KiB LDS limit is a static_assert on the kernel's config struct (dynamic LDS does not show in the metadata), so a
layout that exceeds it fails this compile.
"""
import collections
import os
import shutil
import tempfile

import pytest

from test_fp16_scan_isa import _twin
from test_row_mask_isa import _compile, _mnemonics, _parse

# sweep_scan_kernel<bf16_t, E, MASKED> (t = uint16_t = bf16_t; an empty argument pack follows MASKED): all sweep.hip holds
SWEEP_SCAN = "_ZN3mmr17sweep_scan_kernelIt"


@pytest.fixture(scope="module")
def isa():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "sweep.s")
        assert _compile("sweep.hip", out).wait() == 0, "hipcc -S failed"
        text = open(out).read()
        return _parse(text) + (_with_asm_marks(text),)


def _with_asm_marks(text):
    """{kernel: [line, ...]} like _parse's first result, but keeping the `;;#ASMSTART` / `;;#ASMEND` marks the compiler
    puts around inline assembly"""
    kernels, cur = {}, None
    for ln in text.splitlines():
        t = ln.strip()
        if ln and not ln[0].isspace() and t.startswith("_Z") and ":" in t:
            cur = t.split(":")[0]
            kernels[cur] = []
        elif t.startswith(".Lfunc_end"):
            cur = None
        elif cur and t and (t.startswith(";;#ASM") or not t.startswith((";", "."))):
            kernels[cur].append(t)
    return kernels


def _ring_waits(lines):
    """The hand-counted waits: the `s_waitcnt vmcnt(N)` in front of an s_barrier (the last vmcnt wait before it) and the
    k-loop's counted `s_waitcnt lgkmcnt(N)`, N > 0, which are inline assembly.  (The compiler gives the epilogue's LDS
    reads partial lgkmcnt waits of its own; those are not inside ASMSTART / ASMEND.)"""
    out = []
    instrs = [l for l in lines if not l.startswith(";;#ASM")]
    for n, ins in enumerate(instrs):
        if ins.split()[0] == "s_barrier":
            for back in instrs[max(0, n - 16):n][::-1]:
                if back.startswith("s_waitcnt") and "vmcnt" in back:
                    out.append(back + " -> s_barrier")
                    break
    for n, ins in enumerate(lines):
        if ins.startswith("s_waitcnt lgkmcnt(") and "lgkmcnt(0)" not in ins and n and lines[n - 1] == ";;#ASMSTART":
            out.append(ins)
    return collections.Counter(out)


def _pairs(kernels):
    out = []
    for name in kernels:
        if name.startswith(SWEEP_SCAN) and _twin(name) is not None:
            twin = _twin(name)
            assert twin in kernels, name
            out.append((name, twin))
    return out


def test_every_sweep_scan_has_a_masked_twin(isa):
    kernels, _, _ = isa
    scans = [k for k in kernels if k.startswith(SWEEP_SCAN)]
    pairs = _pairs(kernels)
    assert len(pairs) == 4 and len(scans) == 8, sorted(scans)       # E in {128, 256, 512, 768} x {masked, unmasked}


def test_masked_sweep_scans_keep_the_ring_and_waits_of_the_unmasked_ones(isa):
    kernels, _, marked = isa
    for masked, plain in _pairs(kernels):
        a, b = kernels[masked], kernels[plain]
        wa, wb = _ring_waits(marked[masked]), _ring_waits(marked[plain])
        is_glds = lambda m: m.startswith("global_load_lds")
        assert collections.Counter(_mnemonics(a, is_glds)) == collections.Counter(_mnemonics(b, is_glds)), masked
        assert len(_mnemonics(a, is_glds)) > 0, masked
        assert wa == wb, (masked, wa - wb, wb - wa)
        assert any(w.endswith("s_barrier") for w in wa), masked
        assert any("lgkmcnt" in w and not w.endswith("s_barrier") for w in wa), masked
        is_gload = lambda m: m.startswith(("global_load", "buffer_load", "flat_load")) and not m.startswith("global_load_lds")
        extra = len(_mnemonics(a, is_gload)) - len(_mnemonics(b, is_gload))
        assert extra == 1, (masked, extra)
        is_sload = lambda m: m.startswith(("s_load", "s_buffer_load"))
        assert len(_mnemonics(a, is_sload)) <= len(_mnemonics(b, is_sload)) + 1, masked


def test_no_sweep_kernel_spills(isa):
    kernels, meta, _ = isa
    ours = [k for k in kernels if k.startswith("_ZN3mmr")]
    assert any("sweep_recheck_kernel" in k for k in ours) and any("sweep_finish_kernel" in k for k in ours)
    assert any("sweep_grid_kernel" in k for k in ours)
    for name in ours:
        assert name in meta, name
        scratch, _, vgpr_spills = meta[name]
        assert scratch == 0 and vgpr_spills == 0, (name, meta[name])
    for masked, plain in _pairs(kernels):
        assert meta[masked][1] <= meta[plain][1], (masked, meta[masked], meta[plain])
