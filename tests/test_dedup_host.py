"""CPU: the greedy keep/drop pass of the near-duplicate tool, and host-side argument checks of the range / self-join ABI."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from mmr_amd import dedup


def _reference_loop(n, pairs, order):
    """find_and_remove_duplicate_images (reference tool/find_repeated_in_same_folder.py:59-95), transcribed with the
    hash comparison replaced by membership in the pair list."""
    similar = set()
    for a, b in pairs:
        similar.add((a, b))
        similar.add((b, a))
    reference_images = []
    duplicate_images = []
    for img in order:
        is_duplicate = False
        duplicate_of = None
        for ref in reference_images:
            if (img, ref) in similar:
                is_duplicate = True
                duplicate_of = ref
                break
        if not is_duplicate:
            reference_images.append(img)
        else:
            duplicate_images.append((img, duplicate_of))
    return reference_images, duplicate_images


def _check(n, pairs, order=None):
    i = [p[0] for p in pairs]
    j = [p[1] for p in pairs]
    keep, dup = dedup.keep_first(n, np.array(i, dtype=np.int64), np.array(j, dtype=np.int64), order)
    visit = list(range(n)) if order is None else list(order)
    kept, dups = _reference_loop(n, pairs, visit)
    assert sorted(np.flatnonzero(keep).tolist()) == sorted(kept)
    assert [(r, int(dup[r])) for r in visit if not keep[r]] == dups
    assert all(dup[r] == -1 for r in range(n) if keep[r])
    return keep, dup


def test_chain_keeps_the_far_end():
    # a~b, b~c, a!~c: b goes (duplicate of a), c stays because its only partner was dropped
    keep, dup = _check(3, [(0, 1), (1, 2)])
    assert keep.tolist() == [True, False, True] and dup.tolist() == [-1, 0, -1]


def test_star_and_first_kept_partner_wins():
    keep, dup = _check(6, [(0, 5), (2, 5), (1, 2), (3, 4), (0, 3)])
    assert dup[5] == 0 and dup[3] == 0


def test_order_dependence():
    pairs = [(0, 1), (1, 2)]
    keep_a, _ = _check(3, pairs, [0, 1, 2])
    keep_b, dup_b = _check(3, pairs, [1, 0, 2])
    assert keep_a.tolist() != keep_b.tolist()
    assert keep_b.tolist() == [False, True, False] and dup_b.tolist() == [1, -1, 1]


def test_exhaustive_small_graphs_all_orders():
    rng = np.random.default_rng(3)
    n = 5
    all_pairs = list(itertools.combinations(range(n), 2))
    for trial in range(40):
        pairs = [p for p in all_pairs if rng.random() < 0.35]
        pairs = [(b, a) if rng.random() < 0.5 else (a, b) for a, b in pairs]    # either orientation
        for order in itertools.islice(itertools.permutations(range(n)), 0, 120, 7):
            _check(n, pairs, list(order))


def test_random_large_against_reference_loop():
    rng = np.random.default_rng(11)
    n = 300
    pairs = sorted({tuple(sorted(rng.choice(n, 2, replace=False).tolist())) for _ in range(400)})
    _check(n, pairs)
    _check(n, pairs, rng.permutation(n).tolist())


def test_keep_first_rejects_bad_input():
    with pytest.raises(ValueError):
        dedup.keep_first(3, [0], [3])
    with pytest.raises(ValueError):
        dedup.keep_first(3, [0], [1], order=[0, 0, 1])
    keep, dup = dedup.keep_first(4, [], [])
    assert keep.all() and (dup == -1).all()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def test_range_abi_rejects_bad_arguments_before_any_launch(lib):
    L = lib.lib()
    EINVAL, ENOSPC, ENOTSUP = -22, -28, -95
    nan = float("nan")
    cnt = 16        # any non-null value: every call below returns before it is touched

    def rng_call(q=16, g=16, dt=1, Q=4, N=100, E=512, thr=0.5, scale=1.0, cap=8, cand=8, outs=16, counts=cnt, ws=16, wsb=1 << 40):
        return L.mmr_cosine_range(q, g, 0, dt, Q, N, E, thr, scale, 0.0, 0, 0, cap, cand, outs, outs, outs, 0, counts, ws, wsb, 0)

    def join_call(g=16, dt=1, N=100, E=512, thr=0.5, cap=8, cand=8, outs=16, ws=16, wsb=1 << 40):
        return L.mmr_gallery_self_join(g, 0, dt, N, E, thr, 1.0, 0.0, 0, 0, cap, cand, outs, outs, outs, 0, cnt, ws, wsb, 0)

    assert rng_call(E=1024) == ENOTSUP and b"E=1024" in L.mmr_last_error()
    assert rng_call(E=100) == ENOTSUP
    assert join_call(E=384) == ENOTSUP
    assert rng_call(Q=0) == EINVAL and b"Q=0" in L.mmr_last_error()
    assert rng_call(Q=-3) == EINVAL
    assert rng_call(q=0) == EINVAL and b"null" in L.mmr_last_error()
    assert rng_call(g=0) == EINVAL and b"null" in L.mmr_last_error()
    assert rng_call(counts=0) == EINVAL
    assert rng_call(outs=0) == EINVAL
    assert join_call(g=0) == EINVAL
    assert rng_call(thr=nan) == EINVAL and b"threshold" in L.mmr_last_error()
    assert join_call(thr=float("inf")) == EINVAL
    assert rng_call(scale=0.0) == EINVAL and b"scale" in L.mmr_last_error()
    assert rng_call(dt=7) == EINVAL and b"dtype" in L.mmr_last_error()
    assert rng_call(cand=0) == EINVAL and b"cand_cap" in L.mmr_last_error()
    assert rng_call(q=8) == EINVAL and b"aligned" in L.mmr_last_error()
    assert rng_call(wsb=64) == ENOSPC and b"workspace" in L.mmr_last_error()
    assert join_call(wsb=64) == ENOSPC
    assert rng_call(ws=0) == EINVAL


def test_range_workspace_size(lib):
    L = lib.lib()
    bf = L.mmr_range_workspace_bytes(1_000_000, 512, 256, 1 << 16, 1, 0)
    f32_split = L.mmr_range_workspace_bytes(1_000_000, 512, 256, 1 << 16, 0, 1)
    f32_nosplit = L.mmr_range_workspace_bytes(1_000_000, 512, 256, 1 << 16, 0, 0)
    assert 4 * 8 * (1 << 16) <= bf < 16e6                     # four 8-byte lists of cand_cap + sort storage
    assert bf < f32_split < bf + 1e6                           # + the bf16 copy of the queries
    assert f32_nosplit >= f32_split + 1_000_000 * 512 * 2      # + the gallery's hi half
    assert L.mmr_range_workspace_bytes(100, 512, 1, 0, 1, 0) == 0
    assert L.mmr_range_workspace_bytes(100, 512, 1, 8, 5, 0) == 0
