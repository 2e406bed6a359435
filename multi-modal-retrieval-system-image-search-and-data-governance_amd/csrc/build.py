"""Builds csrc/libmmr_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

    python -m mmr_amd.csrc.build        # or: __graft_entry__.build()

The shared library has no torch / python dependency: it links only the HIP runtime and
exports the C ABI declared in include/mmr.h.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ["api_common.cpp", "comm.cpp", "search.hip", "gemm.hip", "vit_ops.hip", "attention.hip", "tower.hip", "preprocess.hip", "range.hip",
           "sweep.hip", "deep_topk.hip", "search_f16.hip", "range_f16.hip", "sweep_f16.hip", "decide.hip", "decide_f16.hip", "deep_qmask.hip", "sweep_qmask.hip",
           "hash_join.hip", "assign.hip", "assign_f16.hip", "cluster.hip", "silhouette.hip", "silhouette_f16.hip", "kmeanspp.hip", "cluster_rank.hip", "image_hash.hip",
           "tip_train.hip", "augment.hip", "tip_grid.hip", "jpeg_host.cpp", "jpeg.hip", "jpeg_entropy.hip", "row_lists.hip",
           "jpeg_encode_host.cpp", "jpeg_encode.hip"]
LIB = os.path.join(HERE, "libmmr_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip",
         "-Wno-unused-result", "-Wno-unused-value"] + os.environ.get("MMR_EXTRA_HIPCC_FLAGS", "").split()


# per-source flags.  attention.hip (and vit_ops.hip, which held the attention kernels and keeps the flags it was tuned
# and verified with): keep MFMA results in arch VGPRs -- the attention kernels post-process every
# accumulator with VALU code, and the default AGPR form costs a v_accvgpr_read/write per element (measured: streaming
# attention 502 -> 463 us at ViT-L/14@336 B=128).  The GEMM and scan kernels already compile AGPR-free.
# -fno-honor-nans drops the canonicalising v_max x,x clang puts in front of every fmaxf on an MFMA result (30 of the
# 56 max instructions in the streaming-attention loop: 455 -> 440 us); nothing in those files tests for NaN.
# augment.hip: its coefficient tables must be Pillow's integers, so no double multiply-add may be fused; the __d*_rn
# intrinsics are plain inline operators in this toolchain's headers and would contract under the default.
# tip_grid.hip: the same, for its thresholds fl(fl(i * step) + lo) in fp64 and its logits fl(L0 + fl(cache * alpha)) in fp32.
_ATTENTION_FLAGS = ["-mllvm", "-amdgpu-mfma-vgpr-form=1", "-fno-honor-nans"]
PER_SOURCE_FLAGS = {"attention.hip": _ATTENTION_FLAGS,
                    "vit_ops.hip": _ATTENTION_FLAGS,
                    "augment.hip": ["-ffp-contract=off"],
                    "tip_grid.hip": ["-ffp-contract=off"]}


def _obj(src):
    return os.path.join(HERE, "_obj", os.path.splitext(src)[0] + ".o")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(os.path.join(HERE, "_obj"), exist_ok=True)
    headers = [os.path.join(HERE, f) for f in os.listdir(HERE) if f.endswith((".h", ".inc"))]
    headers.append(os.path.join(HERE, "..", "..", "include", "mmr.h"))
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(HERE, s))]

    def compile_one(src):
        sp, op = os.path.join(HERE, src), _obj(src)
        if force or _stale(op, [sp] + headers):
            cmd = [HIPCC] + FLAGS + PER_SOURCE_FLAGS.get(src, []) + ["-c", sp, "-o", op]
            if verbose:
                print("[mmr build]", " ".join(cmd), flush=True)
            subprocess.check_call(cmd)
            return True
        return False

    with ThreadPoolExecutor(max_workers=4) as ex:
        rebuilt = list(ex.map(compile_one, srcs))
    objs = [_obj(s) for s in srcs]
    if force or any(rebuilt) or _stale(LIB, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl"]
        if verbose:
            print("[mmr build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
