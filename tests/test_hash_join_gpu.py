"""GPU: the perceptual-hash joins (csrc/hash_join.hip through mmr_amd.dedup) against a numpy brute force over all pairs.

Every comparison is exact: the same pairs, in the same (i, j) order, with the same distances.  The oracle's population
count is a 256-entry table over a uint8 view, so it does not depend on the numpy version.

Sizes are chosen around the kernel's geometry (csrc/hash_join.hip): a tile is TILE = 1024 rows by 1024 columns, a lane's
four columns lie STRIDE = 256 apart, a wave is 64 lanes.  So 63 / 64 / 65 and 257 cross the wave and the column stride
inside one (diagonal, partial) tile, 1000 is one partial tile, 1023 / 1024 / 1025 sit on the tile edge, 2049 and 4099
have a last tile of 1 and 3 rows behind 2 and 4 full ones (3 and 15 tiles on or above the diagonal).
"""
import ctypes

import numpy as np
import pytest
import torch

from mmr_amd import dedup

pytestmark = pytest.mark.gpu

TILE, STRIDE, WAVE = 1024, 256, 64
_T8 = np.array([bin(v).count("1") for v in range(256)], dtype=np.uint8)
_ONES = np.int64(-1)
_TOP = np.iinfo(np.int64).min                                  # bit 63 alone


def _dist(a, b):
    """[m, H, W] x [n, H, W] int64 -> Hamming distances [m, n, H] int32"""
    x = a.view(np.uint64)[:, None] ^ b.view(np.uint64)[None]
    m, n, H, W = x.shape
    return _T8[np.ascontiguousarray(x).view(np.uint8).reshape(m, n, H, W * 8)].sum(-1, dtype=np.int32)


def _match(d, thr):
    on = np.array([t >= 0 for t in thr])
    return ((d <= np.array(thr)[None, None]) & on[None, None]).any(-1)


def _masked_dist(d, thr):
    out = d.copy()
    out[..., [k for k, t in enumerate(thr) if t < 0]] = -1
    return out


def _brute_self(h, thr, block=256):
    """-> (i, j, dist [P, H]) of every pair i < j within a threshold, sorted by (i, j); -1 in dist for a disabled kind"""
    n = h.shape[0]
    I, J, D = [], [], []
    for r0 in range(0, n, block):
        d = _dist(h[r0:r0 + block], h)
        ok = _match(d, thr) & (np.arange(r0, min(r0 + block, n))[:, None] < np.arange(n)[None])
        i, j = np.nonzero(ok)
        I.append(i + r0)
        J.append(j)
        D.append(_masked_dist(d[i, j], thr))
    return np.concatenate(I), np.concatenate(J), np.concatenate(D).reshape(-1, h.shape[1])


def _brute_cross(q, r, thr, block=256):
    I, J, D = [], [], []
    for r0 in range(0, q.shape[0], block):
        d = _dist(q[r0:r0 + block], r)
        i, j = np.nonzero(_match(d, thr))
        I.append(i + r0)
        J.append(j)
        D.append(_masked_dist(d[i, j], thr))
    if not I:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, r.shape[1]), np.int32)
    return np.concatenate(I), np.concatenate(J), np.concatenate(D).reshape(-1, r.shape[1])


def _thr_list(thr, H):
    return [thr] * H if isinstance(thr, int) else list(thr)


def _random_hashes(rng, n, H, W):
    return rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, size=(n, H, W), dtype=np.int64, endpoint=True)


def _flip(rng, row, kind, nbits, spread=False):
    """flip `nbits` distinct bits of hash `kind` of row [H, W] in place; spread: round-robin over the W words"""
    W = row.shape[1]
    if spread:
        per_word = [len(range(w, nbits, W)) for w in range(W)]
        picks = [(w, int(b)) for w in range(W) for b in rng.choice(64, size=per_word[w], replace=False)]
    else:
        picks = [(int(p) // 64, int(p) % 64) for p in rng.choice(64 * W, size=nbits, replace=False)]
    for w, b in picks:
        row[kind, w] ^= _TOP if b == 63 else np.int64(1) << np.int64(b)


def _plant(rng, h, src, dst, kind, nbits, spread=False):
    """row dst: hash `kind` = row src's with `nbits` bits flipped; its other hashes stay random (no match through them)"""
    h[dst, kind] = h[src, kind]
    _flip(rng, h[dst], kind, nbits, spread)


def _check_self(h_np, thr, dev, **kw):
    i, j, d = dedup.hash_duplicate_pairs(torch.from_numpy(h_np).to(dev), thr, **kw)
    assert i.dtype == torch.int64 and j.dtype == torch.int64 and d.dtype == torch.int32 and i.is_cuda
    bi, bj, bd = _brute_self(h_np, _thr_list(thr, h_np.shape[1]))
    assert np.array_equal(i.cpu().numpy(), bi) and np.array_equal(j.cpu().numpy(), bj)
    assert d.shape == (bi.size, h_np.shape[1]) and np.array_equal(d.cpu().numpy(), bd)
    return bi, bj, bd


def _planted_set(n, thr, seed, H=3, W=1):
    """Random hashes with traps and plants.  Traps: an all-zero row, an all-ones row, rows with bit 63 set, and at N = 65
    two all-zero rows (3 and 64: the last row of the set, alone in the second wave) so that an unused lane filled with
    zeros would invent pairs.  Plants at every distance 0..thr+2, each through one kind only (d % H): inside the first
    (diagonal) tile, from the first tile into a later one, and inside the last, partial, tile while it has free rows."""
    rng = np.random.default_rng(seed)
    h = _random_hashes(rng, n, H, W)
    if n >= 8:
        h[3] = 0
        h[5] = _ONES
        h[6, :, 0] |= _TOP
        h[n - 1, :, 0] |= _TOP
    if n == 65:
        h[64] = 0
    if n == 2:
        _plant(rng, h, 0, 1, 0, thr)
        return h
    if n < 40:
        return h
    taken = {3, 5, 6, n - 1, 64}
    last0 = (n - 1) // TILE * TILE                              # first row of the last tile

    def pick(lo, hi):
        cand = [r for r in rng.permutation(np.arange(lo, hi)).tolist() if r not in taken]
        assert cand, (lo, hi)
        taken.add(cand[0])
        return cand[0]

    for d in range(thr + 3):
        spans = [(0, min(n, TILE), 0, min(n, TILE))]            # inside the first tile
        if last0 > 0:
            spans.append((last0, n, last0, n))                  # inside the last, partial, tile, while it has free rows
            spans.append((0, TILE, TILE, n))                    # across two tiles
        for lo_a, hi_a, lo_b, hi_b in spans:
            free = len([r for r in range(lo_b, hi_b) if r not in taken])
            if free < (2 if lo_a == lo_b else 1):
                continue
            _plant(rng, h, pick(lo_a, hi_a), pick(lo_b, hi_b), d % H, d)
    return h


@pytest.mark.parametrize("thr", [0, 5])
@pytest.mark.parametrize("n", [1, 2, WAVE - 1, WAVE, WAVE + 1, STRIDE + 1, 1000, TILE - 1, TILE, TILE + 1, 2 * TILE + 1,
                               4 * TILE + 3])
def test_self_join_sizes_plants_and_traps(device, n, thr):
    h = _planted_set(n, thr, seed=1000 * thr + n)
    bi, bj, _ = _check_self(h, thr, device)
    pairs = set(zip(bi.tolist(), bj.tolist()))
    if n == 1:
        assert not pairs
    if n == 2:
        assert pairs == {(0, 1)}                               # planted at distance exactly thr
    if n == WAVE + 1:
        assert (3, 64) in pairs and sum(1 for p in pairs if 3 in p or 64 in p) == 1
    if n >= 40:
        assert len(pairs) >= thr + 1                           # the plants at 0..thr match; thr+1, thr+2 do not


def test_plants_cover_the_tile_layout():
    """host only: where the planted pairs of the largest set fall"""
    h = _planted_set(4 * TILE + 3, 5, seed=5 * 1000 + 4 * TILE + 3)
    bi, bj, bd = _brute_self(h, [5, 5, 5])
    same_first = (bi < TILE) & (bj < TILE)
    across = (bi < TILE) & (bj >= TILE)
    in_last = (bi >= 4 * TILE) & (bj >= 4 * TILE)
    assert same_first.sum() >= 6 and across.sum() >= 6
    assert in_last.sum() == 1                                  # the 3-row last tile has room for one pair (one row is a trap)
    assert sorted(set(bd[bd >= 0].tolist()) & set(range(6))) == list(range(6))      # every distance 0..thr is present


def test_last_partial_tile_holds_pairs(device):
    n = TILE + 300                                             # the second tile is partial and wide enough for plants
    h = _planted_set(n, 5, seed=77)
    bi, bj, _ = _check_self(h, 5, device)
    assert ((bi >= TILE) & (bj >= TILE)).sum() >= 6 and ((bi < TILE) & (bj >= TILE)).sum() >= 6


def test_any_rule_and_disabled_kinds(device):
    rng = np.random.default_rng(21)
    n = 300
    h = _random_hashes(rng, n, 3, 1)
    _plant(rng, h, 10, 200, 0, 5)                              # kind 0 only
    _plant(rng, h, 11, 201, 1, 3)                              # kind 1 only
    _plant(rng, h, 12, 202, 2, 0)                              # kind 2 only
    _plant(rng, h, 13, 203, 0, 6)                              # none: one past the threshold
    _plant(rng, h, 13, 203, 1, 7)
    _plant(rng, h, 13, 203, 2, 8)
    bi, bj, _ = _check_self(h, 5, device)
    assert sorted(zip(bi.tolist(), bj.tolist())) == [(10, 200), (11, 201), (12, 202)]
    bi, bj, bd = _check_self(h, (5, -1, 5), device)
    assert sorted(zip(bi.tolist(), bj.tolist())) == [(10, 200), (12, 202)]          # the kind-1-only pair is gone
    assert (bd[:, 1] == -1).all()
    bi, bj, _ = _check_self(h, (-1, 3, -1), device)
    assert list(zip(bi.tolist(), bj.tolist())) == [(11, 201)]
    bi, bj, _ = _check_self(h, (5, 6, 8), device)                                    # a threshold per kind
    assert (13, 203) in set(zip(bi.tolist(), bj.tolist()))


@pytest.mark.parametrize("H,thr", [(1, (3,)), (2, (0, 4)), (4, (0, 5, 2, 7)), (4, (-1, -1, -1, 1))])
def test_other_hash_counts(device, H, thr):
    rng = np.random.default_rng(30 + H)
    n = TILE + 476                                             # two tiles
    h = _random_hashes(rng, n, H, 1)
    rows = rng.permutation(n)
    for k in range(H):
        for d in range(max(thr[k], 0) + 2):
            src, dst = rows[:2].tolist()
            rows = rows[2:]
            _plant(rng, h, src, dst, k, d)
    bi, _, _ = _check_self(h, thr, device)
    assert bi.size == sum(t + 1 for t in thr if t >= 0)


@pytest.mark.parametrize("H", [1, 2, 3, 4])
def test_four_word_hashes(device, H):
    rng = np.random.default_rng(40 + H)
    n, thr = TILE + 76, 5
    h = _random_hashes(rng, n, H, 4)
    h[7] = 0
    h[8] = _ONES
    rows = rng.permutation(np.arange(10, n))
    want = set()
    for k in range(H):
        for d in (thr, thr + 1):                               # bits spread over all four words: 2+1+1+1 and 2+2+1+1
            src, dst = rows[:2].tolist()
            rows = rows[2:]
            _plant(rng, h, src, dst, k, d, spread=True)
            assert all((h[src, k, w] != h[dst, k, w]) for w in range(4))
            if d == thr:
                want.add((min(src, dst), max(src, dst)))
    bi, bj, _ = _check_self(h, thr, device)
    assert set(zip(bi.tolist(), bj.tolist())) == want
    # distances up to 256 need the 16-bit fields: the all-zero against the all-ones row
    i, j, d = dedup.hash_duplicate_pairs(torch.from_numpy(h[7:9].copy()).to(device), 256)
    assert i.tolist() == [0] and j.tolist() == [1] and d.tolist() == [[256] * H]


def _dense(n=300):
    rng = np.random.default_rng(50)
    return rng.integers(0, 256, size=(n, 3, 1), dtype=np.int64)                      # 8 random bits, the rest zero


def test_dense_tile_and_retry(device):
    h = _dense()
    bi, _, _ = _check_self(h, 5, device)
    assert bi.size > 10000                                     # thousands of matches in the one tile
    bi, _, bd = _check_self(h, 64, device, cap=16)             # every pair, through the retry at the reported size
    assert bi.size == 300 * 299 // 2 == 44850 and bd.max() <= 8
    with pytest.raises(MemoryError):
        dedup.hash_duplicate_pairs(torch.from_numpy(h).to(device), 64, cap=16, max_pairs=1000)


def test_raw_abi_overflow_counts_on_and_writes_nothing_past_cap(device):
    from mmr_amd import _lib

    L = _lib.lib()
    h = torch.from_numpy(_dense()).to(device)
    cap, guard = 16, 64
    need = L.mmr_hash_join_workspace_bytes(0, 300, 3, 1, cap)
    ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=device)
    oi = torch.full((cap + guard,), -7, dtype=torch.int32, device=device)
    oj = torch.full((cap + guard,), -7, dtype=torch.int32, device=device)
    od = torch.full((cap + guard,), -7, dtype=torch.int64, device=device)
    counts = torch.full((1 + guard,), -7, dtype=torch.int64, device=device)
    thr = (ctypes.c_int32 * 3)(64, 64, 64)
    _lib.check(L.mmr_hash_self_join(h.data_ptr(), 300, 3, 1, thr, None, cap, oi.data_ptr(), oj.data_ptr(), od.data_ptr(),
                                    counts.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr(device)))
    torch.cuda.synchronize()
    assert counts[0].item() == 44850
    assert (counts[1:] == -7).all() and (oi[cap:] == -7).all() and (oj[cap:] == -7).all() and (od[cap:] == -7).all()
    assert (ws[need:] == 0x5A).all()
    # what was stored is `cap` of the matching pairs, in order
    i, j = oi[:cap].cpu().numpy().astype(np.int64), oj[:cap].cpu().numpy().astype(np.int64)
    assert ((0 <= i) & (i < j) & (j < 300)).all() and (np.diff(i * 300 + j) > 0).all()
    dist = _dist(h.cpu().numpy()[i], h.cpu().numpy())[np.arange(cap), j]
    packed = sum(dist[:, k].astype(np.int64) << (16 * k) for k in range(3)) | (0xFFFF << 48) - (1 << 64)
    assert np.array_equal(od[:cap].cpu().numpy(), packed)      # an absent kind (h = 3) reads 0xFFFF
    # cap = 0 counts only
    _lib.check(L.mmr_hash_self_join(h.data_ptr(), 300, 3, 1, thr, None, 0, None, None, None, counts.data_ptr(), ws.data_ptr(),
                                    need, _lib.stream_ptr(device)))
    assert counts[0].item() == 44850 and (counts[1:] == -7).all()


def test_row_mask(device):
    rng = np.random.default_rng(60)
    n = TILE + 476
    h = _random_hashes(rng, n, 3, 1)
    rows = rng.permutation(n)
    for p in range(60):
        _plant(rng, h, int(rows[2 * p]), int(rows[2 * p + 1]), p % 3, p % 6)
    keep = rng.random(n) < 0.7
    keep[rows[0]] = keep[rows[1]] = True                       # one planted pair surely live,
    keep[rows[2]], keep[rows[3]] = True, False                 # one with a dead row,
    keep[rows[4]], keep[rows[5]] = False, True                 # one with the other row dead
    ht = torch.from_numpy(h).to(device)
    i, j, d = dedup.hash_duplicate_pairs(ht, 5, row_mask=torch.from_numpy(keep).to(device))
    live = np.flatnonzero(keep)
    bi, bj, bd = _brute_self(h[live], [5, 5, 5])               # the compacted set, ids mapped back
    assert 10 < bi.size < 60
    assert np.array_equal(i.cpu().numpy(), live[bi]) and np.array_equal(j.cpu().numpy(), live[bj])
    assert np.array_equal(d.cpu().numpy(), bd)
    full = dedup.hash_duplicate_pairs(ht, 5)
    ones = dedup.hash_duplicate_pairs(ht, 5, row_mask=torch.ones(n, dtype=torch.bool, device=device))
    assert full[0].numel() == 60 and all(torch.equal(a, b) for a, b in zip(full, ones))
    none = dedup.hash_duplicate_pairs(ht, 5, row_mask=torch.zeros(n, dtype=torch.bool, device=device))
    assert none[0].numel() == 0 and tuple(none[2].shape) == (0, 3)


@pytest.mark.parametrize("m,n", [(130, 257), (257, 130), (TILE + 76, TILE + 6)])
def test_cross_join(device, m, n):
    rng = np.random.default_rng(70 + m)
    q, r = _random_hashes(rng, m, 3, 1), _random_hashes(rng, n, 3, 1)
    q[0], r[1], r[n - 1] = 0, 0, 0                            # equal rows across the sets: query 0 matches refs 1 and n-1
    q[m - 1], r[0] = _ONES, _ONES
    for p, (qi, ri) in enumerate(zip(rng.permutation(np.arange(1, m - 1))[:24].tolist(),
                                     rng.permutation(np.arange(2, n - 1))[:24].tolist())):
        r[ri] = q[qi]                                          # a copy, or a near copy through one kind
        if p % 4:
            r[ri] = _random_hashes(rng, 1, 3, 1)[0]
            r[ri, p % 3] = q[qi, p % 3]
            _flip(rng, r[ri], p % 3, p % 8)
    r[n // 2] = q[m // 2]                                      # two refs equal to one query: the lowest row is its match
    r[n // 2 + 1] = q[m // 2]
    qt, rt = torch.from_numpy(q).to(device), torch.from_numpy(r).to(device)
    for thr in (0, 5, (5, -1, 2)):
        off, idx, d = dedup.hash_cross_matches(qt, rt, thr)
        bi, bj, bd = _brute_cross(q, r, _thr_list(thr, 3))
        assert bi.size >= 8
        want_off = np.concatenate([[0], np.cumsum(np.bincount(bi, minlength=m))])
        assert off.dtype == torch.int64 and np.array_equal(off.cpu().numpy(), want_off)
        assert np.array_equal(idx.cpu().numpy(), bj) and np.array_equal(d.cpu().numpy(), bd)
        is_dup, match = dedup.cross_set_duplicates(qt, rt, thr)
        first = np.full(m, -1, dtype=np.int64)
        first[bi[::-1]] = bj[::-1]                             # the lowest matching ref row of each query
        assert np.array_equal(match.cpu().numpy(), first) and np.array_equal(is_dup.cpu().numpy(), first >= 0)
    assert match[0].item() == 1 and match[m - 1].item() == 0
    assert 0 <= match[m // 2].item() <= n // 2 and (off[m // 2 + 1] - off[m // 2]).item() >= 2
    # the default is the reference's: threshold 0
    assert all(torch.equal(a, b) for a, b in zip(dedup.hash_cross_matches(qt, rt), dedup.hash_cross_matches(qt, rt, 0)))
    # a ref mask: the result on the live refs, ids mapped back
    keep = rng.random(n) < 0.6
    keep[1] = False
    off, idx, d = dedup.hash_cross_matches(qt, rt, 5, ref_row_mask=torch.from_numpy(keep).to(device))
    live = np.flatnonzero(keep)
    bi, bj, bd = _brute_cross(q, r[live], [5, 5, 5])
    assert np.array_equal(off.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(bi, minlength=m))]))
    assert np.array_equal(idx.cpu().numpy(), live[bj]) and np.array_equal(d.cpu().numpy(), bd)


def test_empty_sets(device):
    e = torch.zeros(0, 3, 1, dtype=torch.int64, device=device)
    one = torch.zeros(1, 3, 1, dtype=torch.int64, device=device)
    for h in (e, one):
        i, j, d = dedup.hash_duplicate_pairs(h, 5)
        assert i.numel() == 0 and j.numel() == 0 and tuple(d.shape) == (0, 3)
    off, idx, d = dedup.hash_cross_matches(e, one)
    assert off.tolist() == [0] and idx.numel() == 0
    off, idx, d = dedup.hash_cross_matches(one, e)
    assert off.tolist() == [0, 0] and idx.numel() == 0
    is_dup, match = dedup.cross_set_duplicates(one, e)
    assert is_dup.tolist() == [False] and match.tolist() == [-1]


def _sparse(n=70001, plants=500, seed=90):
    rng = np.random.default_rng(seed)
    h = _random_hashes(rng, n, 3, 1)
    rows = rng.permutation(n)[:2 * plants].reshape(plants, 2)
    for p, (a, b) in enumerate(rows.tolist()):
        _plant(rng, h, a, b, p % 3, p % 3 if p % 2 else 2 - p % 3)       # distances 0..2 through each kind
    planted = sorted((min(a, b), max(a, b)) for a, b in rows.tolist())
    return h, planted


def test_larger_sparse_set_returns_exactly_the_plants(device):
    """N = 70 001 (69 tiles a side, 2415 on or above the diagonal), thr = 2: 2.45e9 pairs of random 64-bit hashes hold an
    accidental pair within distance 2 with probability 3 * 2.45e9 * 2081 / 2^64 < 1e-6, and the seed is fixed."""
    h, planted = _sparse()
    i, j, d = dedup.hash_duplicate_pairs(torch.from_numpy(h).to(device), 2)
    i, j, d = i.cpu().numpy(), j.cpu().numpy(), d.cpu().numpy()
    # on the CPU: every returned pair's distances, recomputed; each must be a match with the distances returned
    x = h[i].view(np.uint64) ^ h[j].view(np.uint64)
    re = _T8[np.ascontiguousarray(x).view(np.uint8).reshape(i.size, 3, 8)].sum(-1, dtype=np.int32)
    assert np.array_equal(d, re) and (re.min(axis=1) <= 2).all()
    assert list(zip(i.tolist(), j.tolist())) == planted        # the planted set, nothing accidental, sorted
    assert len(planted) == 500


def test_two_runs_are_bit_identical(device):
    dense = torch.from_numpy(_dense()).to(device)
    sparse = torch.from_numpy(_sparse(n=20001, plants=300, seed=91)[0]).to(device)
    for h, thr in ((dense, 5), (sparse, 2)):
        a = dedup.hash_duplicate_pairs(h, thr)
        b = dedup.hash_duplicate_pairs(h, thr)
        assert a[0].numel() > 250 and all(torch.equal(x, y) for x, y in zip(a, b))
    a = dedup.hash_cross_matches(dense[:130], dense, 3)
    b = dedup.hash_cross_matches(dense[:130], dense, 3)
    assert a[1].numel() > 1000 and all(torch.equal(x, y) for x, y in zip(a, b))
