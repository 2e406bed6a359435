"""CPU: host-side logic, the C-ABI surface (no compute launches), and the N>1 search path on gloo."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import mmr_amd
from mmr_amd import config, synth, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def test_library_exports_every_header_symbol(lib):
    L = lib.lib()
    names = sorted(lib.HEADER.functions)
    assert len(names) >= 18
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert L.mmr_version() == 1


def test_argument_validation_happens_before_any_launch(lib):
    L = lib.lib()
    # every one of these returns on the host, so they are safe without a GPU
    rc = L.mmr_cosine_topk(0, 0, 1, 4, 100, 512, 0, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -22 and b"k=0" in L.mmr_last_error()
    rc = L.mmr_cosine_topk(0, 0, 1, 4, 100, 512, 10, -1.0, 1.0, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -22 and b"scale" in L.mmr_last_error()
    rc = L.mmr_cosine_topk(0, 0, 1, 4, 100, 100, 10, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -95 and b"E=100" in L.mmr_last_error()
    rc = L.mmr_cosine_topk(0, 0, 7, 4, 100, 512, 10, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -22 and b"dtype" in L.mmr_last_error()
    rc = L.mmr_cosine_topk(16, 16, 1, 4, 100, 512, 10, 1.0, 1.0, 16, 16, 0, 0, 16, 8, 0)
    assert rc == -28 and b"workspace" in L.mmr_last_error()
    assert L.mmr_cosine_topk(0, 0, 1, 0, 100, 512, 10, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0) == 0      # Q == 0: nothing to do
    assert L.mmr_l2norm_rows(0, 1, 0, 512, 0) == 0
    assert L.mmr_topk_merge(0, 0, 0, 1, 1, 1.0, 0, 0, 0, 0) == -22
    # merge limits: k <= 64 and parts * k <= 1024, refused before any launch (dummy non-null pointers)
    assert L.mmr_topk_merge(16, 16, 17, 1, 64, 1.0, 16, 16, 16, 0) == -22 and b"exceeds 1024" in L.mmr_last_error()
    assert L.mmr_topk_merge_packed(16, 17, 1, 64, 1.0, 16, 16, 16, 0) == -22 and b"exceeds 1024" in L.mmr_last_error()
    assert L.mmr_topk_merge(16, 16, 1, 1, 65, 1.0, 16, 16, 16, 0) == -22 and b"k=65" in L.mmr_last_error()
    assert L.mmr_topk_merge_packed(16, 1, 1, 65, 1.0, 16, 16, 16, 0) == -22 and b"k=65" in L.mmr_last_error()
    assert L.mmr_cosine_topk(16, 16, 1, 4, 100, 512, 65, 1.0, 1.0, 16, 16, 0, 0, 16, 1 << 30, 0) == -22
    assert b"k=65" in L.mmr_last_error()
    need = L.mmr_search_workspace_bytes(1_000_000, 512, 256, 10)
    assert 30e6 < need < 80e6


def test_tower_layout(lib):
    from mmr_amd.clip import _tower_cfg_struct
    L = lib.lib()
    ccfg = mmr_amd.get_config("ViT-B/32")
    c = _tower_cfg_struct(ccfg.vision)
    total = L.mmr_tower_weights_bytes(ctypes.byref(c))
    n_matrix = 768 * 3072 + 12 * (3 * 768 * 768 + 768 * 768 + 2 * 768 * 3072) + 512 * 768
    assert n_matrix * 2 < total < n_matrix * 2 * 1.02            # bf16 matrices + small fp32 vectors
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    seen = []
    for layer in range(12):
        for p in range(lib.P_LN1_W, lib.P_FC2_B + 1):
            assert L.mmr_tower_param_span(ctypes.byref(c), p, layer, ctypes.byref(off), ctypes.byref(nb)) == 0
            assert off.value % 256 == 0 and off.value + nb.value <= total
            seen.append((off.value, nb.value))
    seen.sort()
    assert all(a[0] + a[1] <= b[0] for a, b in zip(seen, seen[1:])), "tensor spans overlap"
    assert L.mmr_tower_param_span(ctypes.byref(c), lib.P_TOK_EMB, 0, ctypes.byref(off), ctypes.byref(nb)) == -22
    assert L.mmr_tower_param_span(ctypes.byref(c), lib.P_QKV_W, 12, ctypes.byref(off), ctypes.byref(nb)) == -22
    bad = _tower_cfg_struct(ccfg.vision)
    bad.heads = 8
    assert L.mmr_tower_weights_bytes(ctypes.byref(bad)) == 0
    t = _tower_cfg_struct(ccfg.text)
    assert L.mmr_tower_param_span(ctypes.byref(t), lib.P_TOK_EMB, 0, ctypes.byref(off), ctypes.byref(nb)) == 0
    assert nb.value == 49408 * 512 * 2


def test_configs_and_weights():
    assert mmr_amd.available_models() == ["ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px"]
    assert config.get_config("openai/clip-vit-large-patch14").name == "ViT-L/14"
    with pytest.raises(RuntimeError):
        config.get_config("RN50")
    c = config.get_config("ViT-L/14@336px")
    assert c.vision.tokens == 577 and c.vision.patch_k == 588 and c.vision.patch_k_pad == 640
    w1 = weights.make_vision_weights(config.get_config("tiny-test").vision, seed=0)
    w2 = weights.make_vision_weights(config.get_config("tiny-test").vision, seed=0)
    w3 = weights.make_vision_weights(config.get_config("tiny-test").vision, seed=1)
    assert all(torch.equal(w1[k], w2[k]) for k in w1)                      # deterministic
    assert not torch.equal(w1["v.proj"], w3["v.proj"])
    assert all(torch.equal(v, v.bfloat16().float()) for v in w1.values())  # bf16-representable


def test_tokenize_surface():
    from mmr_amd.clip import tokenize
    ids = synth.synth_token_ids(4, 77, 49408, seed=1)
    out = tokenize(ids)
    assert out.shape == (4, 77) and out.dtype == torch.int32 and torch.equal(out, ids)
    short = tokenize([[49406, 320, 1125, 49407]])
    assert short.shape == (1, 77) and short[0, :4].tolist() == [49406, 320, 1125, 49407] and short[0, 4:].sum() == 0
    with pytest.raises(RuntimeError):
        tokenize(["a diagram", "a dog"])                 # no BPE vocabulary offline
    with pytest.raises(RuntimeError):
        tokenize([list(range(1, 90))])                   # too long, like clip.tokenize
    t = tokenize([list(range(1, 90))], truncate=True)
    assert t.shape == (1, 77) and t[0, -1] == 89


def test_tokenize_strings_with_a_merge_table(tmp_path):
    from mmr_amd.clip import tokenize
    p = tmp_path / "merges.txt"
    p.write_text("#version: 0.2\nc a\nca t</w>\n")
    out = tokenize(["cat", "a cat"], bpe_path=str(p))
    assert out.shape == (2, 77) and out[0, 0] == out[1, 0] and (out[0] != 0).sum() == 3   # SOT cat EOT


def test_load_without_checkpoint_raises_instead_of_encoding_noise(tmp_path):
    """clip.load("ViT-B/32") with no checkpoint reachable must not hand back a random-weight model silently."""
    with pytest.raises(FileNotFoundError) as e:
        mmr_amd.load("ViT-B/32", device="cuda")
    assert "synthetic" in str(e.value)
    with pytest.raises(FileNotFoundError):
        mmr_amd.load("ViT-L/14", device="cuda", download_root=str(tmp_path))
    with pytest.raises(FileNotFoundError):
        mmr_amd.load_text_encoder("IDEA-CCNL/Taiyi-CLIP-Roberta-large-326M-Chinese", device="cuda")
    with pytest.raises(RuntimeError):
        mmr_amd.load("RN50", device="cuda")            # unknown architecture: same error as before


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mmr_amd import search
    with pytest.raises(RuntimeError):
        mmr_amd.load("tiny-test", device="cpu")
    with pytest.raises(RuntimeError):
        search.cosine_topk(torch.randn(1, 512), torch.randn(8, 512), 1)


# ------------------------------------------------------------------ N > 1 on gloo (CPU)
def _sharded_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from mmr_amd import search
    from oracle import search_ref

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        gal = synth.synth_unit_rows(3001, 512, seed=31).bfloat16()
        bounds = [0, 1200, 3001]                                   # ragged shards
        local = gal[bounds[rank]:bounds[rank + 1]]
        queries = synth.synth_unit_rows(6, 512, seed=32).bfloat16()

        def local_search(qs, g, k):                                # the oracle stands in for the HIP kernels
            i, _, d = search_ref.cosine_topk(qs, g, k)
            return torch.from_numpy(i), torch.from_numpy(d)

        def merge(idx_parts, dot_parts, scale):
            i, s, d = search_ref.topk_merge(idx_parts.numpy(), dot_parts.numpy(), scale)
            return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(d)

        index = search.ShardedGalleryIndex(local, local_search=local_search, merge=merge)
        assert index.total_rows == 3001 and index.offset == bounds[rank]
        score, idx = index.search(queries, 10, 100.0)
        oi, os_, _ = search_ref.cosine_topk(queries, gal, 10, 100.0)
        ok = bool(np.array_equal(idx.numpy(), oi) and np.array_equal(score.numpy(), os_))
        # k larger than the smaller shard: empty slots (-1) must not leak into the merge
        score2, idx2 = index.search(queries, 40, 1.0)
        oi2, _, _ = search_ref.cosine_topk(queries, gal, 40, 1.0)
        ok = ok and bool(np.array_equal(idx2.numpy(), oi2))
        # a single 1-D query (the reference's ref_feature form): 1-D results on the sharded path too
        s1, i1 = index.search(queries[0], 10, 100.0)
        ok = ok and i1.shape == (10,) and s1.shape == (10,) and bool(np.array_equal(i1.numpy(), oi[0]))
        # pipelined batches: batch i's all-gather is in flight while batch i+1 is searched locally
        outs = index.search_pipelined([queries[:2], queries[2:5], queries[5:]], 10, 100.0)
        ok = ok and bool(np.array_equal(torch.cat([o[1] for o in outs]).numpy(), oi))
        ok = ok and bool(np.array_equal(torch.cat([o[0] for o in outs]).numpy(), os_))
        pend = index.search_async(queries, 10, 100.0)          # explicit handle form
        ok = ok and bool(np.array_equal(pend.result()[1].numpy(), oi))
        # bench.py's post-run proof (search.verify_exact_topk): its all-reduce logic on a real 2-rank group
        verdict, detail = search.verify_exact_topk(index, local, queries, 10)
        ok = ok and verdict == "ok" and detail["ranks"] == 2 and detail["rescored_max_abs_err"] < 1e-12
        v40, _ = search.verify_exact_topk(index, local, queries, 40)     # k beyond what the short shard... still exact
        ok = ok and v40 == "ok"

        # ... and it must FAIL on a wrong merge.  (i) a merge that drops the best candidate of rank 1's shard:
        def merge_drops(idx_parts, dot_parts, scale):
            dot_parts = dot_parts.clone()
            dot_parts[1, :, 0] = -2.0                          # rank 1's best row is pushed out of every merged list
            return merge(idx_parts, dot_parts, scale)

        bad = search.ShardedGalleryIndex(local, local_search=local_search, merge=merge_drops)
        vb, _ = search.verify_exact_topk(bad, local, queries, 10)
        ok = ok and vb.startswith("FAILED") and "missing from the merged list" in vb

        # (ii) ranks that disagree: rank 1 alone swaps two entries of its merged list
        def merge_disagrees(idx_parts, dot_parts, scale):
            sc, ii, dd = merge(idx_parts, dot_parts, scale)
            if rank == 1:
                ii = ii.clone(); dd = dd.clone()
                ii[:, [0, 1]] = ii[:, [1, 0]]
                dd[:, [0, 1]] = dd[:, [1, 0]]
            return sc, ii, dd

        bad2 = search.ShardedGalleryIndex(local, local_search=local_search, merge=merge_disagrees)
        vb2, _ = search.verify_exact_topk(bad2, local, queries, 10)
        # rank 1's list is out of order, rank 0's is fine: rank 0 learns of it through the checksum all-reduce
        ok = ok and vb2.startswith("FAILED") and "ranks disagree" in vb2 and (("order" in vb2) == (rank == 1))
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


def test_sharded_search_world2_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29000 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
    results = sorted(q.get(timeout=5) for _ in range(2))
    assert results == [(0, True), (1, True)]
    assert all(p.exitcode == 0 for p in procs)


def test_bench_starts_its_own_ranks_and_fails_clearly_without_devices():
    """`python bench.py --gpus N` (no launcher) must start N ranks itself and -- on a node without N GPUs -- exit non-zero
    with a device message from the ranks, not an argparse-level refusal and not a rendezvous hang.  (Here: no GPU at all.)"""
    import subprocess
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("this node could actually run two ranks")
    variants = [["--gpus", "2"]] + ([["--gpus", "1", "--spawn"]] if torch.cuda.device_count() == 0 else [])
    for argv in variants:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv, "--steps", "1", "--warmup", "0"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and r.stdout.strip() == ""
        assert "exited with code" in r.stderr                       # the parent reports which rank went first
        assert ("needs an MI355X" in r.stderr) or ("device(s)" in r.stderr), r.stderr


# ------------------------------------------------------------------ gallery cache formats (host-side)
def test_feature_cache_formats_round_trip(tmp_path):
    from mmr_amd import gallery
    import pickle

    feats = synth.synth_unit_rows(7, 512, seed=3).bfloat16()
    keys = [f"cls{i % 2}/img_{i}.jpg" for i in range(7)]
    p = tmp_path / "caches" / "search" / "features.pkl"
    gallery.save_feature_cache(str(p), keys, feats)
    # exactly what the reference's build_cache reads back: dict {relpath: np.float32[512]}
    d = pickle.load(open(p, "rb"))
    assert list(d.keys()) == keys and d[keys[3]].dtype == np.float32 and d[keys[3]].shape == (512,)
    k2, f2 = gallery.load_feature_cache(str(p))
    assert k2 == keys and torch.equal(f2, feats.float())
    # a cache written the reference's way (per-image .cpu().numpy() rows) loads the same
    ref_style = {k: feats[i].float().numpy() for i, k in enumerate(keys)}
    pickle.dump(ref_style, open(tmp_path / "ref.pkl", "wb"))
    k3, f3 = gallery.load_feature_cache(str(tmp_path / "ref.pkl"))
    assert k3 == keys and torch.equal(f3, feats.float())
    with pytest.raises(ValueError):
        gallery.save_feature_cache(str(p), keys[:3], feats)
    # the loader is allow-listed: a cache file that names anything but numpy's array helpers raises before it runs

    class Evil:
        def __reduce__(self):
            return (os.system, ("echo pwned > /tmp/mmr_cache_pwned",))

    if os.path.exists("/tmp/mmr_cache_pwned"):
        os.remove("/tmp/mmr_cache_pwned")
    pickle.dump({"a.jpg": Evil()}, open(tmp_path / "evil.pkl", "wb"))
    with pytest.raises(pickle.UnpicklingError):
        gallery.load_feature_cache(str(tmp_path / "evil.pkl"))
    assert not os.path.exists("/tmp/mmr_cache_pwned")
    pickle.dump({"a.jpg": np.array(["x"], dtype=object)}, open(tmp_path / "obj.pkl", "wb"))
    with pytest.raises(pickle.UnpicklingError):
        gallery.load_feature_cache(str(tmp_path / "obj.pkl"))
    pickle.dump([1, 2, 3], open(tmp_path / "list.pkl", "wb"))
    with pytest.raises(pickle.UnpicklingError):
        gallery.load_feature_cache(str(tmp_path / "list.pkl"))
    labels = torch.arange(7)
    gallery.save_split_features(str(tmp_path / "c"), "val", feats.float(), labels)
    f4, l4 = gallery.load_split_features(str(tmp_path / "c"), "val")
    assert torch.equal(f4, feats.float()) and torch.equal(l4, labels)
    assert [b.shape[0] for b in gallery.batched(list(range(10)), lambda i: torch.zeros(3, 4, 4), 4)] == [4, 4, 2]


def test_fold_layernorm_identity():
    """Host-side weight folding for mmr_tower_cfg.fold_ln: rstd*(h@W'^T - mean*c) + b' equals LN(h)@W^T + b."""
    from mmr_amd.clip import fold_layernorm
    g = torch.Generator().manual_seed(5)
    d, n = 128, 192
    W = (torch.randn(n, d, generator=g) * 0.05).bfloat16().float()
    b = torch.randn(n, generator=g) * 0.02
    gamma = 1 + 0.1 * torch.randn(d, generator=g)
    beta = 0.05 * torch.randn(d, generator=g)
    h = torch.randn(7, d, generator=g) * 3 + 0.5
    Wf, bf, c = fold_layernorm(W, b, gamma, beta)
    assert Wf.dtype == torch.bfloat16 and bf.shape == (n,) and c.shape == (n,)
    assert torch.equal(c, Wf.double().sum(1).float())            # row sums of the ROUNDED folded weight
    mean = h.double().mean(1, keepdim=True)
    var = h.double().var(1, unbiased=False, keepdim=True)
    rstd = (var + 1e-5).rsqrt()
    folded = rstd * (h.double() @ Wf.double().t() - mean * c.double()) + bf.double()
    ref = torch.nn.functional.layer_norm(h.double(), (d,), gamma.double(), beta.double(), 1e-5) @ W.double().t() + b.double()
    # the only difference is the bf16 rounding of W*gamma (2^-9 relative per weight)
    assert (folded - ref).abs().max().item() <= 2 ** -8 * ref.abs().max().item()


def test_fold_ln_layout_adds_column_sums():
    from mmr_amd import _lib
    from mmr_amd.clip import _tower_cfg_struct
    ccfg = mmr_amd.get_config("tiny-test")
    L = _lib.lib()
    plain, fold = _tower_cfg_struct(ccfg.vision), _tower_cfg_struct(ccfg.vision, fold_ln=True)
    d, m = ccfg.vision.width, ccfg.vision.mlp
    extra = ccfg.vision.layers * (((3 * d * 4 + 255) // 256 + (m * 4 + 255) // 256) * 256)
    assert L.mmr_tower_weights_bytes(ctypes.byref(fold)) == L.mmr_tower_weights_bytes(ctypes.byref(plain)) + extra
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.mmr_tower_param_span(ctypes.byref(fold), _lib.P_QKV_C, 1, ctypes.byref(off), ctypes.byref(nb)) == 0
    assert nb.value == 3 * d * 4
    assert L.mmr_tower_param_span(ctypes.byref(plain), _lib.P_QKV_C, 0, ctypes.byref(off), ctypes.byref(nb)) != 0
    bert = _lib.TowerCfg(kind=2, width=128, layers=2, heads=2, mlp=512, tokens=64, embed_dim=128, vocab=1000,
                         ln_eps=1e-12, fold_ln=1)
    assert L.mmr_tower_weights_bytes(ctypes.byref(bert)) == 0      # post-LN towers cannot fold


def test_header_is_plain_c99_and_links_against_the_library(tmp_path):
    """include/mmr.h is the drop-in boundary: it must compile as C (no C++/torch types) and a C program must link
    against libmmr_hip.so using nothing but that header."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include "mmr.h"\n'
                   'int main(void) {\n'
                   '    mmr_tower_cfg c = {0};\n'
                   '    c.kind = 0; c.width = 768; c.layers = 12; c.heads = 12; c.mlp = 3072; c.tokens = 50;\n'
                   '    c.embed_dim = 512; c.image_size = 224; c.patch = 32; c.ln_eps = 1e-5f;\n'
                   '    printf("%d %zu %zu\\n", mmr_version(), mmr_tower_weights_bytes(&c), mmr_search_workspace_bytes(1000000, 512, 256, 10));\n'
                   '    return 0;\n}\n')
    inc = os.path.join(root, "include")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-fsyntax-only", str(src)])
    from mmr_amd import _lib
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "abi"
    subprocess.check_call([gcc, "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-l:libmmr_hip.so",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    if out.returncode == 0:        # layout queries need no GPU; a box without the HIP runtime libraries may fail to start
        ver, wbytes, ws = out.stdout.split()
        assert int(ver) >= 1 and int(wbytes) > 170_000_000 and int(ws) > 0


# ------------------------------------------------------------------ hand-counted s_waitcnt: fail the BUILD, not a parity test
def _kernel_isa(src):
    """{mangled kernel name: [instruction mnemonic, ...]} of one .hip source compiled for gfx950 (device code only) with
    the flags the build gives that source."""
    import shutil
    import subprocess
    import tempfile
    from mmr_amd.csrc.build import PER_SOURCE_FLAGS
    flags = PER_SOURCE_FLAGS.get(src, [])
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "multi-modal-retrieval-system-image-search-and-data-governance_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-Wno-unused-result",
                               "-Wno-unused-value", "--cuda-device-only", "-S", *flags, os.path.join(csrc, src), "-o", out],
                              stderr=subprocess.DEVNULL)
        text = open(out).read()
    kernels, cur = {}, None
    for ln in text.splitlines():
        t = ln.strip()
        if ln and not ln[0].isspace() and t.startswith("_Z") and ":" in t:
            cur = t.split(":")[0]
            kernels[cur] = []
        elif t.startswith(".Lfunc_end"):
            cur = None
        elif cur and t and not t.startswith((";", ".")):
            kernels[cur].append(t.split()[0])
    return kernels


def test_counted_vmcnt_waits_match_the_instructions_hipcc_emits():
    """gemm256_persist_kernel's counted `s_waitcnt vmcnt(N)` name the previous tile's epilogue stores and this
    tile's bias loads as the youngest queue entries -- correct only if hipcc emits exactly GEMM2P_STORES = 16 stores and NIW
    bias loads per tile, once per tile width.  The persistent attention kernel likewise counts 4 output stores per query
    block.  A toolchain that merges, splits or duplicates those instructions must fail HERE, at build time, not as a rare
    wrong LDS read on the GPU."""
    g = _kernel_isa("gemm.hip")
    persist = {k: v for k, v in g.items() if "gemm256_persist_kernel" in k}
    assert len(persist) == 3                                   # EPI_BIAS_BF16, QuickGELU, exact GELU
    for name, ins in persist.items():
        stores = [i for i in ins if i.startswith("global_store")]
        reg_loads = [i for i in ins if i.startswith("global_load") and "lds" not in i]
        # two run_tile instantiations (full tiles NIW = 4, half tiles NIW = 2): 16 stores each; 4 + 2 bias loads
        assert len(stores) == 32 and all(s == "global_store_dwordx4" for s in stores), (name, len(stores))
        assert len(reg_loads) == 6 and all(l == "global_load_dwordx4" for l in reg_loads), (name, reg_loads)
        assert "scratch_store_dword" not in ins and not any(i.startswith("scratch_") for i in ins), name   # no spills
    v = _kernel_isa("attention.hip")
    att = {k: ins for k, ins in v.items() if "attention_kernel" in k and "stream" not in k}
    assert len(att) == 9                                       # NT in {2,4,6} x {plain, causal, masked}
    for name, ins in att.items():
        nt = int(name.split("attention_kernelILi")[1][0])
        nq = 2 if nt > 4 else 1                                # query blocks per wave
        stores = [i for i in ins if i.startswith("global_store")]
        q_loads = [i for i in ins if i == "global_load_dwordx4"]
        assert len(stores) == 4 * nq and all(s == "global_store_dwordx2" for s in stores), (name, stores)
        assert len(q_loads) == 2 * (2 * nq), (name, len(q_loads))          # two load_q sites x NQ blocks x 2 halves
        assert not any(i.startswith("scratch_") for i in ins), name
