"""CPU: the per-query-mask scan kernels (deep_qmask.hip, sweep_qmask.hip), checked without a GPU in the manner of
test_row_mask_isa.py / test_fp16_scan_isa.py.  This checks wait counts and spills only.

The two translation units are compiled with `hipcc -S` for gfx950, next to a stub that instantiates the SHARED-mask twins
from the headers: scan_kernel / scan16_kernel<T, E, true> (topk_scan_body.h) and sweep_scan_kernel<T, E, true>
(sweep_scan_body.h).  A per-query kernel must have its twin's global_load_lds instructions and its twin's hand-counted
waits, plus exactly the delta its placement of the mask words implies:

  top-k scans   the task's words are staged in LDS before the ring, behind one extra workgroup barrier, and each tile's
                word is read by ONE inline-assembly ds_read_b32 issued in front of the tile's k-loop (LDS reads return in
                order, so the k-loop's counted lgkmcnt(N > 0) waits are the twin's, unchanged) and named in ONE extra
                inline-assembly `s_waitcnt lgkmcnt(0)` behind it.  The ring's vmcnt waits are the twin's; the staging
                barrier may add one `vmcnt(0) -> s_barrier` in front of the ring.
  sweep         the words are staged beside the labels, before the barrier the body already has, and read by ordinary LDS
                loads in the binning epilogue, where every wait is the compiler's: the inline-assembly waits and the
                ring's counted vmcnt(N > 0) waits are the twin's, with no delta.  The barrier in front of the ring closes the
                staging in both kernels; the vmcnt(0) the compiler puts in front of it waits for the twin's one mask word
                or for the staging loop's loads, so that one `vmcnt(0) -> s_barrier` record may differ.
"""
import collections
import os
import shutil
import subprocess
import tempfile

import pytest

from test_fp16_scan_isa import _mnemonics, _parse, _ring_waits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-modal-retrieval-system-image-search-and-data-governance_amd", "csrc")

STUB = r"""
#include "topk_scan_body.h"
#include "sweep_scan_body.h"
namespace mmr {
#define TOPK_ARGS(T) (const T *, const T *, int, int64_t, int, int, int, int, float *, float *, const uint32_t *)
#define TWINS(T)                                                          \
    template __global__ void scan_kernel<T, 128, true> TOPK_ARGS(T);      \
    template __global__ void scan_kernel<T, 256, true> TOPK_ARGS(T);      \
    template __global__ void scan_kernel<T, 512, true> TOPK_ARGS(T);      \
    template __global__ void scan16_kernel<T, 768, true> TOPK_ARGS(T);    \
    template __global__ void sweep_scan_kernel<T, 128, true>(SweepScanArgs);  \
    template __global__ void sweep_scan_kernel<T, 256, true>(SweepScanArgs);  \
    template __global__ void sweep_scan_kernel<T, 512, true>(SweepScanArgs);  \
    template __global__ void sweep_scan_kernel<T, 768, true>(SweepScanArgs);
TWINS(bf16_t)
TWINS(f16_t)
}
"""

# mangled names, (prefix, what follows <element type, E>): t = uint16_t = bf16_t, DF16_ = _Float16.  The per-query sweep
# is sweep_scan_kernel<T, E, false, QMaskArgs>; the twins are the MASKED = true instantiations.
QM = {"scan": ("_ZN3mmr14scan_qm_kernelI", "EEv"), "scan16": ("_ZN3mmr16scan16_qm_kernelI", "EEv"),
      "sweep": ("_ZN3mmr17sweep_scan_kernelI", "Lb0EJNS_9QMaskArgsEEEEv")}
TWIN = {"scan": ("_ZN3mmr11scan_kernelI", "Lb1EEEv"), "scan16": ("_ZN3mmr13scan16_kernelI", "Lb1EEEv"),
        "sweep": ("_ZN3mmr17sweep_scan_kernelI", "Lb1EJEEEv")}
ARGS = {"scan": [f"{t}Li{e}E" for t in ("t", "DF16_") for e in (128, 256, 512)], "scan16": [f"{t}Li768E" for t in ("t", "DF16_")],
        "sweep": [f"{t}Li{e}E" for t in ("t", "DF16_") for e in (128, 256, 512, 768)]}


@pytest.fixture(scope="module")
def isa():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as td:
        stub = os.path.join(td, "twins.hip")
        with open(stub, "w") as f:
            f.write(STUB)
        srcs = {"deep_qmask": os.path.join(CSRC, "deep_qmask.hip"), "sweep_qmask": os.path.join(CSRC, "sweep_qmask.hip"), "twins": stub}
        outs = {n: os.path.join(td, n + ".s") for n in srcs}
        procs = [subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-Wno-unused-result",
                                   "-Wno-unused-value", "-I", CSRC, "--cuda-device-only", "-S", srcs[n], "-o", outs[n]],
                                  stderr=subprocess.DEVNULL) for n in srcs]
        assert all(p.wait() == 0 for p in procs), "hipcc -S failed"
        kernels, meta, marked = {}, {}, {}
        for n, o in outs.items():
            k, m, a = _parse(open(o).read())
            assert not set(k) & set(kernels), (n, sorted(set(k) & set(kernels)))      # the stub repeats no kernel of the project's
            kernels.update(k)
            meta.update(m)
            marked.update(a)
    return kernels, meta, marked


def _find(kernels, name, args):
    prefix, rest = name
    hits = [n for n in kernels if n.startswith(prefix + args + rest)]
    assert len(hits) == 1, (prefix, args, rest, hits)
    return hits[0]


def _pairs(kernels, kind):
    return [(_find(kernels, QM[kind], a), _find(kernels, TWIN[kind], a)) for a in ARGS[kind]]


def _twins(kernels):
    """the stub's kernels"""
    return {_find(kernels, TWIN[kind], a) for kind in ARGS for a in ARGS[kind]}


def _asm(lines, what):
    """inline-assembly statements (the line right behind ;;#ASMSTART) that start with `what`"""
    return [l for n, l in enumerate(lines) if n and lines[n - 1] == ";;#ASMSTART" and l.startswith(what)]


def _split_waits(waits):
    ring = collections.Counter({w: c for w, c in waits.items() if w.endswith("s_barrier")})
    kloop = collections.Counter({w: c for w, c in waits.items() if not w.endswith("s_barrier")})
    return ring, kloop


def test_the_kernel_set(isa):
    kernels, _, _ = isa
    twins = _twins(kernels)
    assert len(twins) == 2 * (3 + 1 + 4), sorted(twins)
    ours = [n for n in kernels if n.startswith("_ZN3mmr") and n not in twins]
    scans = [n for n in ours if n.startswith(tuple(p for p, _ in QM.values()))]
    assert len(scans) == 6 + 2 + 8, scans
    rescore = [n for n in ours if n.startswith("_ZN3mmr22deep_rescore_qm_kernelI")]
    assert len(rescore) == 12                      # 3 element types x 4 E
    assert len(ours) == len(scans) + len(rescore) + 1, ours          # + row_masks_pack_kernel


def test_no_scratch_and_no_vgpr_spills(isa):
    kernels, meta, _ = isa
    twins = _twins(kernels)
    for n in kernels:
        if n.startswith("_ZN3mmr") and n not in twins:
            assert n in meta, n
            scratch, _, vgpr_spills = meta[n]
            assert scratch == 0 and vgpr_spills == 0, (n, meta[n])


@pytest.mark.parametrize("kind", ["scan", "scan16"])
def test_topk_scans_keep_the_ring_and_the_counted_waits(isa, kind):
    kernels, _, marked = isa
    is_glds = lambda m: m.startswith("global_load_lds")
    for qm, twin in _pairs(kernels, kind):
        a, b = kernels[qm], kernels[twin]
        assert collections.Counter(_mnemonics(a, is_glds)) == collections.Counter(_mnemonics(b, is_glds)), qm
        assert len(_mnemonics(a, is_glds)) > 0, qm
        (ra, ka), (rb, kb) = _split_waits(_ring_waits(marked[qm])), _split_waits(_ring_waits(marked[twin]))
        assert ka == kb and sum(ka.values()) > 0, (qm, ka - kb, kb - ka)          # the k-loop's counted lgkmcnt(N > 0) waits
        extra = ra - rb
        assert not (rb - ra) and set(extra) <= {"s_waitcnt vmcnt(0) -> s_barrier"} and sum(extra.values()) <= 1, (qm, ra, rb)
        # the delta: one LDS word read in front of each k-loop, one lgkmcnt(0) that names it behind the loop
        assert len(_asm(marked[qm], "ds_read_b32")) == 1 and len(_asm(marked[twin], "ds_read_b32")) == 0, qm
        assert len(_asm(marked[qm], "s_waitcnt lgkmcnt(0)")) == len(_asm(marked[twin], "s_waitcnt lgkmcnt(0)")) + 1, qm
        assert len(_asm(marked[qm], "ds_read_b128")) == len(_asm(marked[twin], "ds_read_b128")), qm
        # no other memory access entered the ring: the vector loads and stores are the twin's but for the staging's loads
        n_store = lambda k: len(_mnemonics(k, lambda m: m.startswith("global_store")))
        assert n_store(a) == n_store(b), qm


def test_sweep_scans_keep_the_ring_and_the_counted_waits(isa):
    kernels, _, marked = isa
    is_glds = lambda m: m.startswith("global_load_lds")
    for qm, twin in _pairs(kernels, "sweep"):
        a, b = kernels[qm], kernels[twin]
        assert collections.Counter(_mnemonics(a, is_glds)) == collections.Counter(_mnemonics(b, is_glds)), qm
        assert len(_mnemonics(a, is_glds)) > 0, qm
        wa, wb = _ring_waits(marked[qm]), _ring_waits(marked[twin])
        diff = (wa - wb) + (wb - wa)
        assert set(diff) <= {"s_waitcnt vmcnt(0) -> s_barrier"} and sum(diff.values()) <= 1, (qm, wa - wb, wb - wa)
        assert any(w.endswith("s_barrier") for w in wa), qm                                # the ring's vmcnt waits (E = 768: a 2-slot ring, vmcnt(0) only)
        assert any(not w.endswith("s_barrier") for w in wa), qm                            # the k-loop's counted lgkmcnt(N > 0)
        assert len(_asm(marked[qm], "s_waitcnt")) == len(_asm(marked[twin], "s_waitcnt")), qm
        assert len(_asm(marked[qm], "ds_read")) == len(_asm(marked[twin], "ds_read")), qm
