"""GPU: phash / dhash / whash of decoded images (csrc/image_hash.hip through mmr_amd.dedup) against the PIL + numpy oracle
of image_hash_helpers.py.

Bytes before bits: hash bits are a lossy view of the resized images (a wrong pixel rarely flips one), so every size first
compares the intermediate results -- the (hs+1) x hs and 4hs x 4hs planes, the hs x hs block sums and the S x S image of
whash -- with Pillow's bytes, and only then the hashes and status words with the rule path, bit for bit.

Sizes (image_hash_helpers.SIZES, (H, W)) are chosen around the kernels' geometry: the horizontal pass stages rows in groups
of 4 pixels (widths 1, 5, 9, 70, 131, 257, 1025 leave a partial group, 255 and 257 an odd row stride), a thread owns 4
neighbouring output columns or a 2..64-lane group shares one (9 / 17 / 32 / 64 wide targets with 1 to hundreds of taps),
a workgroup owns a share of the rows and takes up to 32 at a time (1, 3, 7, 8, 33, 97, 513 rows; 1600 -> 9 columns
exceeds the 1024 taps a lane group keeps in registers), the vertical pass strides over 256-thread blocks
(S = 8 .. 1024).  Every target meets its identity pass (9 and 17 wide, 8 and 16 high, 32, 64, 256), upscaling (1 x 1, 7 x 5,
3 x 200) and sides on both sides of a power of two.  One 1200 x 1600 image is the large case.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import image_hash_helpers as ih
from mmr_amd import dedup

pytestmark = pytest.mark.gpu

ALL_SIZES = ih.SIZES + [ih.BIG]
DEBUG_W_SIZES = set(ih.SIZES)               # the S x S image is compared for the sizes up to 513 x 1025


def _dev(arr, device):
    return torch.from_numpy(np.array(arr)).to(device)        # a copy: the fixtures are read-only


_results = {}


def _run(h, w, hs, device):
    """all fixtures of one size in one call, with the intermediates: computed once per (size, hs)"""
    key = (h, w, hs)
    if key not in _results:
        names = [n for n, _ in ih.fixtures(h, w)]
        plan = dedup.ImageHashPlan([_dev(a, device) for _, a in ih.fixtures(h, w)], hs, debug=(h, w) in DEBUG_W_SIZES)
        hashes, status = plan.run()
        torch.cuda.synchronize(device)
        scratch = [{k: v.cpu().numpy() for k, v in plan.scratch(r).items()} for r in range(len(names))]
        _results[key] = (names, hashes.cpu().numpy(), status.cpu().numpy(), scratch)
    return _results[key]


@pytest.mark.parametrize("hs", ih.HASH_SIZES)
@pytest.mark.parametrize("hw", ALL_SIZES)
def test_intermediate_bytes_are_pillows(hw, hs, device):
    h, w = hw
    names, _, _, scratch = _run(h, w, hs, device)
    for r, (name, arr) in enumerate(ih.fixtures(h, w)):
        want = ih.planes(arr, hs)
        assert np.array_equal(scratch[r]["dhash_plane"], want["dhash"]), (name, "dhash plane")
        assert np.array_equal(scratch[r]["phash_plane"], want["phash"]), (name, "phash plane")
        assert np.array_equal(scratch[r]["sums"], ih.block_sums(want["whash"], hs)), (name, "block sums")
        if hw in DEBUG_W_SIZES:
            assert np.array_equal(scratch[r]["whash_image"], want["whash"]), (name, "whash image")


@pytest.mark.parametrize("hs", ih.HASH_SIZES)
@pytest.mark.parametrize("hw", ALL_SIZES)
def test_hashes_and_status_equal_the_rule_path(hw, hs, device):
    h, w = hw
    names, hashes, status, _ = _run(h, w, hs, device)
    hexes = dedup.hashes_to_hex(hashes, hs)
    for r, name in enumerate(names):
        words, st, lit = ih.expected(h, w, hs, name)
        assert status[r] == st, (name, status[r], st)
        assert np.array_equal(hashes[r], words), name
        if st == 0:
            assert hexes[r] == lit, name


def _mixed(device, sizes=None):
    """every fixture of every (small) size: [(h, w, name, device tensor)]"""
    sizes = ih.SIZES if sizes is None else sizes
    return [(h, w, name, _dev(a, device)) for h, w in sizes for name, a in ih.fixtures(h, w)]


@pytest.mark.parametrize("hs", ih.HASH_SIZES)
def test_mixed_batch_equals_per_image_calls(hs, device):
    items = _mixed(device)
    perm = np.random.default_rng(hs).permutation(len(items)).tolist()
    probe = items[perm[0]]
    batch = [items[i] for i in perm]
    mid = len(batch) // 2
    batch.insert(mid, probe)
    batch.append(probe)                                    # the same image first, in the middle and last
    hashes, status = dedup.image_hashes([t for *_, t in batch], hs, return_status=True)
    hashes, status = hashes.cpu().numpy(), status.cpu().numpy()
    assert np.array_equal(hashes[0], hashes[mid]) and np.array_equal(hashes[0], hashes[-1])
    assert status[0] == status[mid] == status[-1]
    for r, (h, w, name, t) in enumerate(batch):
        words, st, _ = ih.expected(h, w, hs, name)
        assert np.array_equal(hashes[r], words) and status[r] == st, (h, w, name)
    for r in (0, 5, len(batch) - 2):                       # batch of 1
        one, st1 = dedup.image_hashes([batch[r][3]], hs, return_status=True)
        assert one.shape == (1, 3, hs * hs // 64) and np.array_equal(one.cpu().numpy()[0], hashes[r]) and int(st1[0]) == status[r]


def test_seventy_tiny_images_in_one_call(device):
    rng = np.random.default_rng(70)
    arrs = [rng.integers(0, 256, (int(rng.integers(1, 12)), int(rng.integers(1, 12)), 3), dtype=np.uint8) for _ in range(70)]
    hashes, status = dedup.image_hashes([_dev(a, device) for a in arrs], 8, return_status=True)
    hashes, status = hashes.cpu().numpy(), status.cpu().numpy()
    for r, a in enumerate(arrs):
        bits, st = ih.rule_bits(a, 8)
        assert status[r] == st and np.array_equal(hashes[r], np.stack([ih.pack(bits[k]) for k in ih.KINDS])), (r, a.shape)


def test_small_workspace_splits_the_batch(device, monkeypatch):
    sizes = [(97, 131), (64, 257), (33, 70)]
    items = _mixed(device, sizes)
    imgs = [t for *_, t in items]
    want, want_st = dedup.image_hashes(imgs, 8, return_status=True)
    calls = []
    real = dedup.ImageHashPlan

    class Counting(real):
        def __init__(self, images, *a, **k):
            calls.append(len(images))
            super().__init__(images, *a, **k)

    monkeypatch.setattr(dedup, "ImageHashPlan", Counting)
    limit = 8 * 64 * (41 + 64) + 4096                      # about eight of the largest images
    got, got_st = dedup.image_hashes(imgs, 8, return_status=True, max_workspace_bytes=limit)
    assert len(calls) >= 3 and sum(calls) == len(imgs)
    assert torch.equal(got, want) and torch.equal(got_st, want_st)
    with pytest.raises(MemoryError, match="max_workspace_bytes"):
        dedup.image_hashes(imgs, 8, max_workspace_bytes=1024)


def test_batch_tensor_equals_list(device):
    rng = np.random.default_rng(4)
    stack = rng.integers(0, 256, (5, 33, 70, 3), dtype=np.uint8)
    t = _dev(stack, device)
    a, sa = dedup.image_hashes(t, 16, return_status=True)
    b, sb = dedup.image_hashes([t[i] for i in range(5)], 16, return_status=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    bits, _ = ih.rule_bits(stack[3], 16)
    assert np.array_equal(a[3].cpu().numpy(), np.stack([ih.pack(bits[k]) for k in ih.KINDS]))


def test_greyscale_equals_equal_channels(device):
    for h, w in ((7, 5), (33, 70), (97, 131), (64, 257)):
        g = np.asarray(ih.to_L(dict(ih.fixtures(h, w))["natural"]))
        rgb = np.repeat(g[:, :, None], 3, axis=2)
        for hs in ih.HASH_SIZES:
            a, sa = dedup.image_hashes([_dev(g, device)], hs, return_status=True)
            b, sb = dedup.image_hashes([_dev(rgb, device)], hs, return_status=True)
            assert torch.equal(a, b) and torch.equal(sa, sb)
            bits, st = ih.rule_bits(g, hs)
            assert int(sa[0]) == st and np.array_equal(a[0].cpu().numpy(), np.stack([ih.pack(bits[k]) for k in ih.KINDS]))


def test_every_kinds_subset(device):
    items = _mixed(device, [(8, 9), (97, 131), (64, 257)])
    imgs = [t for *_, t in items]
    for hs in ih.HASH_SIZES:
        full, full_st = dedup.image_hashes(imgs, hs, return_status=True)
        for mask in range(1, 8):
            kinds = tuple(k for i, k in enumerate(dedup.HASH_KINDS) if mask >> i & 1)
            rows = [i for i in range(3) if mask >> i & 1]
            got, st = dedup.image_hashes(imgs, hs, kinds=kinds, return_status=True)
            assert torch.equal(got, full[:, rows]), kinds
            assert torch.equal(st, full_st & ((mask & 1) | (mask >> 1 & 2))), kinds      # a status bit belongs to its kind


def test_workspace_contents_do_not_leak(device):
    items = _mixed(device, [(7, 5), (97, 131), (64, 257)])
    outs = []
    for fill in (0x00, 0xFF):
        plan = dedup.ImageHashPlan([t for *_, t in items], 16)
        plan.workspace.fill_(fill)
        plan.hashes.fill_(-7)
        plan.status.fill_(-7)
        h, s = plan.run()
        torch.cuda.synchronize(device)
        outs.append((h.clone(), s.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for r, (h, w, name, _) in enumerate(items):
        words, st, _ = ih.expected(h, w, 16, name)
        assert np.array_equal(outs[1][0][r].cpu().numpy(), words) and int(outs[1][1][r]) == st


def test_graph_capture_and_replay_on_new_pixels(device):
    sizes = [(97, 131), (64, 257), (8, 9)]
    first = [_dev(dict(ih.fixtures(h, w))["natural"], device) for h, w in sizes]
    second = [dict(ih.fixtures(h, w))["noise"] for h, w in sizes]
    plan = dedup.ImageHashPlan(first, 8)
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        plan.run()                                          # warm up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.run()
    for t, a in zip(first, second):
        t.copy_(_dev(a, device))                            # new pixels in the same buffers
    plan.hashes.zero_()
    torch.cuda.synchronize(device)
    graph.replay()
    torch.cuda.synchronize(device)
    for r, (h, w) in enumerate(sizes):
        words, st, _ = ih.expected(h, w, 8, "noise")
        assert np.array_equal(plan.hashes[r].cpu().numpy(), words) and int(plan.status[r]) == st


def test_bad_descriptor_is_reported_not_run(device):
    from mmr_amd import _lib

    plan = dedup.ImageHashPlan([_dev(dict(ih.fixtures(33, 70))["natural"], device)] * 2, 8)
    L = _lib.lib()
    args = (plan.hashes.data_ptr(), plan.status.data_ptr(), plan.workspace.data_ptr(), plan.workspace.numel(), _lib.stream_ptr(device))
    for bad in ((None, 2, 8, 7), (plan.desc.data_ptr(), 2, 12, 7), (plan.desc.data_ptr(), 2, 8, 0), (plan.desc.data_ptr(), 2, 8, 8),
                (plan.desc.data_ptr(), 70000, 8, 7)):
        assert L.mmr_image_hashes(*bad, *args) == _lib._C["MMR_EINVAL"]
        assert b"mmr_image_hashes" in L.mmr_last_error()
    # a workspace smaller than the descriptors need: rejected on the device, nothing written outside it
    _lib.check(L.mmr_image_hashes(plan.desc.data_ptr(), 2, 8, 7, plan.hashes.data_ptr(), plan.status.data_ptr(),
                                  plan.workspace.data_ptr(), plan.sizes[1][2] + 64, _lib.stream_ptr(device)))
    torch.cuda.synchronize(device)
    words, st, _ = ih.expected(33, 70, 8, "natural")
    assert int(plan.status[0]) == st and np.array_equal(plan.hashes[0].cpu().numpy(), words)
    assert int(plan.status[1]) == _lib._C["MMR_IMAGE_HASH_BAD_DESC"] and not plan.hashes[1].any()
    with pytest.raises(ValueError, match="16384"):
        dedup.image_hashes([torch.zeros(1, 16385, dtype=torch.uint8, device=device)])


def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "image_hash_dedup_synthetic.py")
    spec = importlib.util.spec_from_file_location("image_hash_dedup_synthetic", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_find_image_duplicates_end_to_end(device):
    keys, arrays, sizes, planted = _example().planted_set(images=30, copies=12, seed=1)
    order = np.argsort(-sizes, kind="stable")
    found = dedup.find_image_duplicates(keys, [_dev(a, device) for a in arrays], 5, order=order)
    # the oracle's hashes, a plain Hamming loop over all pairs, and keep_first
    words = []
    for a in arrays:
        bits, _ = ih.rule_bits(a, 8)
        words.append(np.stack([ih.pack(bits[k]) for k in ih.KINDS]).view(np.uint64)[:, 0])
    I, J = [], []
    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            if min(bin(int(x) ^ int(y)).count("1") for x, y in zip(words[i], words[j])) <= 5:
                I.append(i)
                J.append(j)
    keep, dup = dedup.keep_first(len(keys), np.array(I, dtype=np.int64), np.array(J, dtype=np.int64), order)
    want = [(keys[r], keys[int(dup[r])]) for r in order.tolist() if not keep[r]]
    assert found == want
    assert sorted(want) == sorted((c, o) for c, o, _ in planted)       # the fixture itself: the oracle finds every planted pair, nothing else
