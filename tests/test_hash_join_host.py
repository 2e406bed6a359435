"""CPU: the host side of the perceptual-hash joins -- hex packing, the C ABI's argument checks (no launch: there is no
GPU here, so a call that got as far as a launch would return MMR_EIO, not the code asserted), and the keep/drop list of
``find_hash_duplicates`` over a brute-force pair list."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from mmr_amd import dedup


def _popcount_rows(a, b):
    """Hamming distance per hash kind of two [H, W] int64 arrays, from a uint8 view (independent of the numpy version)"""
    x = np.bitwise_xor(a.view(np.uint64), b.view(np.uint64))
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[0], -1), axis=1).sum(axis=1)


@pytest.mark.parametrize("digits", [16, 64])
def test_hashes_from_hex_round_trip(digits):
    rnd = random.Random(digits)
    n, H = 24, 3
    vals = [[rnd.getrandbits(4 * digits) for _ in range(H)] for _ in range(n)]
    vals[0] = [0] * H
    vals[1] = [(1 << (4 * digits)) - 1] * H                 # all ones: every word negative as int64
    vals[2][0] = 1 << (4 * digits - 1)                      # only the top bit
    rows = [tuple(f"{v:0{digits}x}" for v in r) for r in vals]
    rows[3] = tuple(s.upper() for s in rows[3])             # hex digits in either case
    t = dedup.hashes_from_hex(rows)
    W = 1 if digits == 16 else 4
    assert t.dtype == torch.int64 and tuple(t.shape) == (n, H, W) and not t.is_cuda
    a = t.numpy()
    assert (a[1] == -1).all() and (a[0] == 0).all() and a[2, 0, 0] == np.iinfo(np.int64).min
    for i in range(n):
        for j in range(n):
            want = [bin(vals[i][h] ^ vals[j][h]).count("1") for h in range(H)]
            assert _popcount_rows(a[i], a[j]).tolist() == want, (i, j)
    # big-endian words: word 0 holds the most significant 64 bits
    for h in range(H):
        words = [int(np.uint64(w)) for w in a[5, h].view(np.uint64)]
        assert sum(w << (64 * (W - 1 - k)) for k, w in enumerate(words)) == vals[5][h]


def test_hashes_from_hex_mixed_lengths_and_single_strings():
    t = dedup.hashes_from_hex([("ff", "0" * 63 + "1"), ("0f", "8" + "0" * 63)])
    assert tuple(t.shape) == (2, 2, 4)                      # a 64-digit kind makes W = 4; the short kind is zero-extended
    assert t[0, 0].tolist() == [0, 0, 0, 0xFF] and t[0, 1].tolist() == [0, 0, 0, 1]
    assert t[1, 1].tolist() == [np.iinfo(np.int64).min, 0, 0, 0]
    one = dedup.hashes_from_hex(["00ff00ff00ff00ff", "ffffffffffffffff"])
    assert tuple(one.shape) == (2, 1, 1) and one[1, 0, 0].item() == -1


@pytest.mark.parametrize("rows", [
    [("0123456789abcdef", "00"), ("0123456789abcdef",)],                 # ragged: a row with fewer hashes
    [("0123456789abcdef",), ("0123456789abcde",)],                       # ragged: a shorter string of the same kind
    [("0123456789abcdeg",)],                                             # not hexadecimal
    [("0x23456789abcdef",)],
    [("+123456789abcdef",)],
    [("0123_56789abcdef",)],
    [(" 123456789abcdef",)],
    [("",)],
    [("0" * 65,)],                                                       # more than 64 digits
    [("0", "0", "0", "0", "0")],                                         # more than 4 kinds
    [(b"00",)],
    [],
])
def test_hashes_from_hex_rejects(rows):
    with pytest.raises(ValueError):
        dedup.hashes_from_hex(rows)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def test_hash_join_abi_rejects_bad_arguments_before_any_launch(lib):
    L = lib.lib()
    EINVAL, ENOSPC = -22, -28
    thr5 = (ctypes.c_int32 * 4)(5, 5, 5, 5)
    off = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    one_on = (ctypes.c_int32 * 4)(-1, -1, 0, -1)
    p = 4096            # any aligned non-null value: every call below returns before it is touched

    def self_call(h=p, N=100, H=3, W=1, thr=thr5, mask=0, cap=16, oi=p, oj=p, od=p, counts=p, ws=p, wsb=1 << 40):
        return L.mmr_hash_self_join(h, N, H, W, thr, mask, cap, oi, oj, od, counts, ws, wsb, 0)

    def cross_call(q=p, M=10, r=p, N=100, H=3, W=1, thr=thr5, mask=0, cap=16, oq=p, orf=p, od=p, counts=p, ws=p, wsb=1 << 40):
        return L.mmr_hash_cross_join(q, M, r, N, H, W, thr, mask, cap, oq, orf, od, counts, ws, wsb, 0)

    for call in (self_call, cross_call):
        assert call(H=0) == EINVAL and b"H=0" in L.mmr_last_error()
        assert call(H=5) == EINVAL and b"H=5" in L.mmr_last_error()
        assert call(W=3) == EINVAL and b"W=3" in L.mmr_last_error()
        assert call(W=0) == EINVAL and call(W=2) == EINVAL
        assert call(thr=off) == EINVAL and b"threshold" in L.mmr_last_error()
        assert call(H=2, thr=one_on) == EINVAL                           # the enabled entry lies past H
        assert call(thr=None) == EINVAL and b"null" in L.mmr_last_error()
        assert call(N=2 ** 31) == EINVAL and b"N=" in L.mmr_last_error()
        assert call(N=2 ** 31 - 1) == EINVAL
        assert call(N=-1) == EINVAL
        assert call(cap=-1) == EINVAL and b"cap" in L.mmr_last_error()
        assert call(od=p + 4) == EINVAL and b"aligned" in L.mmr_last_error()
        assert call(counts=p + 4) == EINVAL and b"aligned" in L.mmr_last_error()
        assert call(mask=p + 2) == EINVAL and b"aligned" in L.mmr_last_error()
        assert call(ws=p + 8) == EINVAL and b"aligned" in L.mmr_last_error()
        assert call(counts=0) == EINVAL and b"null" in L.mmr_last_error()
        assert call(ws=0) == EINVAL
        assert call(wsb=64) == ENOSPC and b"workspace" in L.mmr_last_error()
        need = L.mmr_hash_join_workspace_bytes(0, 100, 3, 1, 16)
        assert call(wsb=need - 1) == ENOSPC
    assert self_call(h=p + 4) == EINVAL and b"aligned" in L.mmr_last_error()
    assert self_call(h=0) == EINVAL and b"null" in L.mmr_last_error()
    assert self_call(oi=p + 2) == EINVAL and b"aligned" in L.mmr_last_error()
    assert self_call(oi=0) == EINVAL and b"null" in L.mmr_last_error()
    assert cross_call(q=p + 4) == EINVAL and b"aligned" in L.mmr_last_error()
    assert cross_call(r=p + 12) == EINVAL and b"aligned" in L.mmr_last_error()
    assert cross_call(q=0) == EINVAL and b"null" in L.mmr_last_error()
    assert cross_call(r=0) == EINVAL and b"null" in L.mmr_last_error()
    assert cross_call(M=2 ** 31) == EINVAL and b"M=" in L.mmr_last_error()
    assert cross_call(M=-1) == EINVAL


def test_hash_join_workspace_bytes(lib):
    L = lib.lib()
    sizes = [L.mmr_hash_join_workspace_bytes(0, 1_000_000, 3, 1, cap) for cap in (0, 1, 16, 1000, 1 << 16, 1 << 20, 1 << 24)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)          # monotone in cap
    assert sizes[-1] >= 4 * 8 * (1 << 24)                                 # two (key, distance) lists of cap: append + sorted
    assert sizes[-1] < 8 * 8 * (1 << 24)
    # O(cap): the row count and the hash shape do not enter
    assert L.mmr_hash_join_workspace_bytes(500, 10, 4, 4, 1 << 16) == sizes[4]
    for bad in ((0, 10, 0, 1, 16), (0, 10, 5, 1, 16), (0, 10, 3, 3, 16), (0, -1, 3, 1, 16), (-1, 10, 3, 1, 16), (0, 10, 3, 1, -1)):
        assert L.mmr_hash_join_workspace_bytes(*bad) == 0, bad


def _brute_pairs(h, thr):
    """numpy: the pairs i < j with any enabled kind within its threshold, sorted, and their distances [P, H]"""
    a = h.numpy()
    n, H = a.shape[:2]
    out, dist = [], []
    for i in range(n):
        for j in range(i + 1, n):
            d = _popcount_rows(a[i], a[j])
            if any(t >= 0 and d[k] <= t for k, t in enumerate(thr)):
                out.append((i, j))
                dist.append(d.tolist())
    return out, dist


def _reference_loop(similar, order):
    """find_and_remove_duplicate_images (reference tool/find_repeated_in_same_folder.py:59-95) over a similarity set"""
    kept, dups = [], []
    for img in order:
        of = next((ref for ref in kept if (img, ref) in similar), None)
        if of is None:
            kept.append(img)
        else:
            dups.append((img, of))
    return dups


def test_find_hash_duplicates_is_keep_first_over_the_pairs(monkeypatch):
    rng = np.random.default_rng(5)
    n, H = 60, 3
    base = rng.integers(0, 2 ** 63, size=(12, H, 1), dtype=np.int64)
    a = base[rng.integers(0, 12, size=n)].copy()
    flips = rng.integers(0, 4, size=(n, H))                              # near copies: up to 3 flipped bits per kind
    for r in range(n):
        for k in range(H):
            for b in rng.choice(64, size=flips[r, k], replace=False):
                a[r, k, 0] ^= np.int64(1) << np.int64(b) if b < 63 else np.iinfo(np.int64).min
    hashes = torch.from_numpy(a)
    thr = (5, -1, 4)
    pairs, dist = _brute_pairs(hashes, thr)
    assert 20 < len(pairs) < n * (n - 1) // 2
    calls = []

    def stub(h, thresholds=5, **kw):
        calls.append((h, thresholds))
        i = torch.tensor([p[0] for p in pairs], dtype=torch.int64)
        j = torch.tensor([p[1] for p in pairs], dtype=torch.int64)
        return i, j, torch.tensor(dist, dtype=torch.int32).reshape(-1, H)

    monkeypatch.setattr(dedup, "hash_duplicate_pairs", stub)
    keys = [f"img_{r:03d}.jpg" for r in range(n)]
    similar = {(x, y) for x, y in pairs} | {(y, x) for x, y in pairs}
    sizes = rng.integers(1, 50, size=n)                                  # ties: the stable sort keeps row order among them
    for order in (None, np.argsort(-sizes, kind="stable")):
        got = dedup.find_hash_duplicates(keys, hashes, thr, order=order)
        keep, dup = dedup.keep_first(n, [p[0] for p in pairs], [p[1] for p in pairs], order)
        visit = list(range(n)) if order is None else order.tolist()
        assert got == [(keys[r], keys[int(dup[r])]) for r in visit if not keep[r]]
        assert got == [(keys[x], keys[y]) for x, y in _reference_loop(similar, visit)]
        assert len(got) > 10
    assert len(calls) == 2 and calls[0][0] is hashes and calls[0][1] == thr
    with pytest.raises(ValueError):
        dedup.find_hash_duplicates(keys[:-1], hashes, thr)


def test_threshold_and_tensor_checks_need_no_gpu():
    h = torch.zeros(4, 3, 1, dtype=torch.int64)
    with pytest.raises(ValueError):
        dedup.hash_duplicate_pairs(h.to(torch.int32))
    with pytest.raises(ValueError):
        dedup.hash_duplicate_pairs(torch.zeros(4, 5, 1, dtype=torch.int64))
    with pytest.raises(ValueError):
        dedup.hash_duplicate_pairs(torch.zeros(4, 3, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        dedup.hash_duplicate_pairs(h)                                    # a CPU tensor: there is no CPU path
    arr, thr = dedup._hash_thresholds(5, 3)
    assert list(arr) == [5, 5, 5] and thr == [5, 5, 5]
    assert list(dedup._hash_thresholds((5, -1, 0), 3)[0]) == [5, -1, 0]
    for bad in ((5, 5), (-1, -1, -1), -1, (5.5, 1, 1)):
        with pytest.raises(ValueError):
            dedup._hash_thresholds(bad, 3)
    packed = torch.tensor([0x0003 | (0xFFFF << 16) | (0x0100 << 32) | (0xFFFF << 48) - (1 << 64)], dtype=torch.int64)
    assert dedup._unpack_dist(packed, 3).tolist() == [[3, -1, 256]]
