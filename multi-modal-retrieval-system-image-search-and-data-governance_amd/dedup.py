"""Near-duplicate detection over an embedding gallery -- the data-governance half of the project.

The reference compares every image with every image it has kept so far, on the CPU (O(N^2) hash comparisons):
    find_and_remove_duplicate_images       reference tool/find_repeated_in_same_folder.py:59-105
    (also tool/find_repeated.py, tool/delete repeated.py)
Here the pairwise test is one GPU self-join of the gallery above a cosine threshold (``search.gallery_self_join``,
exact fp64 decisions), and the reference's greedy keep/drop loop runs on the host over the resulting pair list
(``keep_first``), linear in the number of pairs.  Nothing here touches a file: deleting what ``find_duplicates``
reports is the caller's business.

Order matters.  The reference visits images sorted by file size, largest first (find_repeated_in_same_folder.py:73),
so which copy survives depends on that order; here the visit order is the caller's ``order`` argument (default: row
order).  Pass ``order=np.argsort(-sizes, kind="stable")`` to reproduce the reference's choice.

The reference's OWN predicate is not a cosine but a perceptual-hash rule, and it has its own calls here:
    are_images_similar: phash / dhash / whash, any Hamming distance <= 5   reference tool/find_repeated_in_same_folder.py:38-54
    dhash of a train image within a threshold of a test image's          reference tool/delete repeated.py:11,120-135
``hash_duplicate_pairs`` / ``find_hash_duplicates`` answer the first and ``hash_cross_matches`` /
``cross_set_duplicates`` the second, each by one integer-exact GPU join over all pairs (csrc/hash_join.hip).  Computing
the hashes stays with the caller (``hashes_from_hex`` packs the strings the reference prints).
"""
import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch


def near_duplicate_pairs(gallery: torch.Tensor, threshold: float, scale: float = 1.0, **caps):
    """All row pairs ``i < j`` of ``gallery`` (on the GPU) with fp64 ``dot(row i, row j) >= threshold``, sorted by
    ``(i, j)``: ``(i int64, j int64, dot64 fp64)`` device tensors.  For unit rows ``threshold`` is a cosine.
    ``caps``: ``max_pairs`` / ``cap`` / ``cand_cap`` as in ``search.cosine_range``."""
    from .search import gallery_self_join

    i, j, _, dot64 = gallery_self_join(gallery, threshold, scale, **caps)
    return i, j, dot64


def _as_np(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.int64).reshape(-1)


def keep_first(n: int, i, j, order: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The reference's greedy pass over a pair list: rows are visited in ``order`` (default ``0..n-1``); a row is a
    duplicate of the FIRST KEPT row, in visit order, that it is paired with and that was visited before it; a row paired
    only with rows that were themselves dropped is kept.

    ``i``, ``j``: the matching pairs (any order, either orientation; e.g. ``near_duplicate_pairs``).
    Returns ``(keep bool [n], duplicate_of int64 [n])`` with ``duplicate_of = -1`` for kept rows.  Host work, linear in
    n plus the number of pairs (after one sort of the pairs)."""
    n = int(n)
    a, b = _as_np(i), _as_np(j)
    if a.shape != b.shape:
        raise ValueError("i and j must have the same length")
    if a.size and (min(a.min(), b.min()) < 0 or max(a.max(), b.max()) >= n):
        raise ValueError(f"pair ids must lie in [0, {n})")
    order = np.arange(n, dtype=np.int64) if order is None else _as_np(order)
    if order.shape != (n,) or not np.array_equal(np.sort(order), np.arange(n)):
        raise ValueError("order must be a permutation of range(n)")
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n, dtype=np.int64)
    # orient every pair as (later row, earlier row) in visit order; drop self pairs
    pa, pb = pos[a], pos[b]
    later = np.where(pa > pb, a, b)
    earlier = np.where(pa > pb, b, a)
    live = pa != pb
    later, earlier = later[live], earlier[live]
    # per later row, its earlier partners in visit order
    srt = np.lexsort((pos[earlier], pos[later]))
    later, earlier = later[srt], earlier[srt]
    keep = np.ones(n, dtype=bool)
    dup = np.full(n, -1, dtype=np.int64)
    # rows are decided in visit order, and a row's partners all precede it, so they are decided when it is reached
    starts = np.flatnonzero(np.r_[True, later[1:] != later[:-1]]) if later.size else np.empty(0, dtype=np.int64)
    ends = np.r_[starts[1:], later.size]
    for s, e in zip(starts.tolist(), ends.tolist()):
        r = int(later[s])
        for u in earlier[s:e].tolist():
            if keep[u]:
                keep[r] = False
                dup[r] = u
                break
    return keep, dup


def find_duplicates(keys: Sequence, features: torch.Tensor, threshold: float,
                    order: Optional[Sequence[int]] = None, **caps):
    """``find_and_remove_duplicate_images`` without the file system: ``keys[r]`` names row r of ``features`` (e.g. its
    path); returns the reference's list ``[(duplicate_key, kept_key), ...]`` in visit order.  Two rows are duplicates
    when their fp64 dot product is at least ``threshold`` (the cosine for L2-normalised features)."""
    n = len(keys)
    if features.shape[0] != n:
        raise ValueError(f"{n} keys for {features.shape[0]} feature rows")
    i, j, _ = near_duplicate_pairs(features, threshold, **caps)
    keep, dup = keep_first(n, i, j, order)
    visit = range(n) if order is None else _as_np(order).tolist()
    return [(keys[r], keys[int(dup[r])]) for r in visit if not keep[r]]


# ---------------------------------------------------------------------------------------------------------------------
# Perceptual-hash joins

_HASH_CAP_INIT = 1 << 16            # first output capacity; a call that reports more matches is repeated once at that size
_HASH_MAX_PAIRS = 1 << 27           # default ceiling on the pairs a call may allocate room for (40 B of workspace and output per pair)
_HEX_DIGITS = frozenset("0123456789abcdefABCDEF")


def hashes_from_hex(rows) -> torch.Tensor:
    """Hex strings -> the hash tensor of the joins: int64 ``[N, H, W]`` on the CPU.

    ``rows[r]`` is a tuple of H hex strings -- the reference's ``(str(phash), str(dhash), str(whash))`` -- or one string
    (H = 1).  All strings of one kind have the same length, at most 64 hex digits; every kind is parsed big-endian into
    W 64-bit words, W = 1 if no kind has more than 16 digits (hash_size 8) and 4 otherwise (hash_size 16), shorter kinds
    zero-extended.  Word 0 holds the most significant bits; any fixed bit order would do, the Hamming distance does not
    depend on it.  A word with its top bit set is a negative int64: the joins count bits, not values.
    Raises ValueError on ragged or non-hex input."""
    rows = [(r,) if isinstance(r, str) else tuple(r) for r in rows]
    if not rows:
        raise ValueError("hashes_from_hex: no rows (the hash count and width come from the first row)")
    H = len(rows[0])
    if not 1 <= H <= 4:
        raise ValueError(f"hashes_from_hex: {H} hashes per row, the joins take 1..4")
    lens = []
    for h, sh in enumerate(rows[0]):
        if not isinstance(sh, str) or not 1 <= len(sh) <= 64:
            raise ValueError(f"hashes_from_hex: row 0, hash {h}: expected 1..64 hex digits, got {sh!r}")
        lens.append(len(sh))
    W = 1 if max(lens) <= 16 else 4
    out = np.zeros((len(rows), H, W), dtype=np.uint64)
    for r, row in enumerate(rows):
        if len(row) != H:
            raise ValueError(f"hashes_from_hex: row {r} has {len(row)} hashes, row 0 has {H}")
        for h, sh in enumerate(row):
            if not isinstance(sh, str) or len(sh) != lens[h]:
                raise ValueError(f"hashes_from_hex: row {r}, hash {h}: expected {lens[h]} hex digits, got {sh!r}")
            if not _HEX_DIGITS.issuperset(sh):
                raise ValueError(f"hashes_from_hex: row {r}, hash {h}: {sh!r} is not hexadecimal")
            v = int(sh, 16)
            for w in range(W):
                out[r, h, w] = (v >> (64 * (W - 1 - w))) & 0xFFFFFFFFFFFFFFFF
    return torch.from_numpy(out.view(np.int64))


def _hash_tensor(x, what: str) -> torch.Tensor:
    """int64 [N,H,W] (or [N,H]: W = 1) on the GPU, contiguous, with H and W the library's"""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.int64:
        raise ValueError(f"{what} must be an int64 tensor [N, H, W] (uint64 bits; see hashes_from_hex)")
    if x.dim() == 2:
        x = x.unsqueeze(-1)
    if x.dim() != 3 or not 1 <= x.shape[1] <= 4 or x.shape[2] not in (1, 4):
        raise ValueError(f"{what} has shape {tuple(x.shape)}; expected [N, H, W] with H in 1..4 and W in (1, 4)")
    if not x.is_cuda:
        raise RuntimeError(f"{what} must live on the GPU (there is no CPU path)")
    if x.shape[0] >= 2 ** 31 - 1:
        raise ValueError(f"{what}: {x.shape[0]} rows exceed int32 row ids")
    return x.contiguous()


def _hash_thresholds(thresholds, H: int):
    """an int, or a length-H sequence of ints (negative: that kind is off) -> (ctypes int32[H], list)"""
    if isinstance(thresholds, (int, np.integer)):
        thr = [int(thresholds)] * H
    else:
        thr = [int(t) for t in thresholds]
        if len(thr) != H or any(t != u for t, u in zip(thr, thresholds)):
            raise ValueError(f"thresholds must be an int or {H} ints, got {thresholds!r}")
    if all(t < 0 for t in thr):
        raise ValueError("every threshold is negative: no hash kind is enabled")
    thr = [min(max(t, -1), 2 ** 31 - 1) for t in thr]
    return (ctypes.c_int32 * H)(*thr), thr


def _unpack_dist(packed: torch.Tensor, H: int) -> torch.Tensor:
    """the C ABI's packed distances (16 bits per kind) -> int32 [P, H], -1 for a disabled kind"""
    shifts = torch.arange(H, dtype=torch.int64, device=packed.device) * 16
    d = (packed.unsqueeze(1) >> shifts) & 0xFFFF
    return torch.where(d == 0xFFFF, torch.full_like(d, -1), d).to(torch.int32)


def _hash_call(queries, refs, thresholds, mask_words, cap, max_pairs):
    """mmr_hash_self_join (queries None) or mmr_hash_cross_join under ``_retry.run``, with the output capacity ``cap``.
    -> (first ids int32 [P], second ids int32 [P], packed distances int64 [P]), sorted."""
    from . import _lib, _retry
    from .search import _workspace

    L = _lib.lib()
    if not hasattr(L, "mmr_hash_self_join"):
        raise RuntimeError("this libmmr_hip.so has no hash joins: rebuild it")
    N, H, W = refs.shape
    M = 0 if queries is None else queries.shape[0]
    thr, _ = _hash_thresholds(thresholds, H)
    dev = refs.device
    cap = _HASH_CAP_INIT if cap is None else int(cap)
    if cap < 0:
        raise ValueError(f"cap={cap} must be >= 0")
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    outs = None

    def launch(cap):
        nonlocal outs
        ws = _workspace(L.mmr_hash_join_workspace_bytes(M, N, H, W, cap), dev)
        outs = [torch.empty(max(cap, 1), dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int64)]
        tail = (H, W, thr, _lib.ptr(mask_words), cap, *(o.data_ptr() for o in outs), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                _lib.stream_ptr(dev))
        if queries is None:
            _lib.check(L.mmr_hash_self_join(refs.data_ptr(), N, *tail))
        else:
            _lib.check(L.mmr_hash_cross_join(queries.data_ptr(), M, refs.data_ptr(), N, *tail))
        return counts.tolist()

    matches, = _retry.run(launch, (cap,), max_pairs,
                          lambda c, caps: f"hash join: {c[0]} matches exceed the capacity {caps[0]} the first call reported",
                          lambda need: f"hash join at thresholds {list(thr)} needs room for {need[0]} pairs, above "
                                       f"max_pairs={max_pairs}: lower the thresholds or raise max_pairs")
    return tuple(o[:matches] for o in outs)


def _hash_mask_words(row_mask, N: int, device):
    from .search import _check_row_mask, _pack_row_mask

    _check_row_mask(row_mask, N, device)
    return None if row_mask is None else _pack_row_mask(row_mask, None, N)


def hash_duplicate_pairs(hashes: torch.Tensor, thresholds=5, *, row_mask: Optional[torch.Tensor] = None,
                         max_pairs: int = _HASH_MAX_PAIRS, cap: Optional[int] = None):
    """All row pairs ``i < j`` of ``hashes`` that the reference's ``are_images_similar`` calls similar
    (tool/find_repeated_in_same_folder.py:38-54): for SOME hash kind h, the Hamming distance of the two rows' hashes is
    ``<= thresholds[h]``.  One GPU pass over all pairs, integer-exact.

    ``hashes``: int64 ``[N, H, W]`` on the GPU (``hashes_from_hex``; ``[N, H]`` means W = 1), H = 1..4 kinds of W = 1 or 4
    64-bit words.  ``thresholds``: one int for every kind (the reference's 5) or a length-H sequence; a negative entry
    turns its kind off.  ``row_mask`` (bool [N] on the same device): a pair counts only if both rows are True.
    Returns ``(i int64 [P], j int64 [P], dist int32 [P, H])`` on the device, sorted by ``(i, j)``; ``dist[p, h]`` is the
    distance of kind h, -1 for a kind that is off.  ``cap`` is the first call's capacity; a call that finds more pairs is
    repeated once at the reported size, unless that exceeds ``max_pairs`` (MemoryError)."""
    h = _hash_tensor(hashes, "hashes")
    words = _hash_mask_words(row_mask, h.shape[0], h.device)
    a, b, d = _hash_call(None, h, thresholds, words, cap, max_pairs)
    return a.to(torch.int64), b.to(torch.int64), _unpack_dist(d, h.shape[1])


def find_hash_duplicates(keys: Sequence, hashes: torch.Tensor, thresholds=5, order: Optional[Sequence[int]] = None):
    """``find_and_remove_duplicate_images`` (tool/find_repeated_in_same_folder.py:59-105) without the file system and
    with its own predicate: ``keys[r]`` names row r of ``hashes``; returns the reference's list
    ``[(duplicate_key, kept_key), ...]`` in visit order, by ``keep_first`` over ``hash_duplicate_pairs``.
    ``order=np.argsort(-sizes, kind="stable")`` reproduces the reference's visit order (:73, largest file first)."""
    n = len(keys)
    if hashes.shape[0] != n:
        raise ValueError(f"{n} keys for {hashes.shape[0]} hash rows")
    i, j, _ = hash_duplicate_pairs(hashes, thresholds)
    keep, dup = keep_first(n, i, j, order)
    visit = range(n) if order is None else _as_np(order).tolist()
    return [(keys[r], keys[int(dup[r])]) for r in visit if not keep[r]]


def hash_cross_matches(query_hashes: torch.Tensor, ref_hashes: torch.Tensor, thresholds=0, *,
                       ref_row_mask: Optional[torch.Tensor] = None, max_pairs: int = _HASH_MAX_PAIRS,
                       cap: Optional[int] = None):
    """Every ref row within the thresholds of a query row -- the comparison of tool/delete repeated.py:120-135 (dhash,
    threshold 0 by default) for all M x N pairs in one GPU pass.  Same match rule, tensors and capacities as
    ``hash_duplicate_pairs``; ``ref_row_mask`` (bool [N]): only refs where it is True match.
    Returns CSR ``(offsets int64 [M+1], ref_idx int64 [P], dist int32 [P, H])``: the matches of query q are
    ``ref_idx[offsets[q]:offsets[q+1]]``, rows ascending."""
    from .search import _csr

    q = _hash_tensor(query_hashes, "query_hashes")
    r = _hash_tensor(ref_hashes, "ref_hashes")
    if q.shape[1:] != r.shape[1:] or q.device != r.device:
        raise ValueError(f"query hashes {tuple(q.shape)} on {q.device} do not pair with ref hashes {tuple(r.shape)} on {r.device}")
    words = _hash_mask_words(ref_row_mask, r.shape[0], r.device)
    qi, ri, d = _hash_call(q, r, thresholds, words, cap, max_pairs)
    return _csr(qi, q.shape[0]), ri.to(torch.int64), _unpack_dist(d, r.shape[1])


def cross_set_duplicates(query_hashes: torch.Tensor, ref_hashes: torch.Tensor, thresholds=0, **caps):
    """The decision of tool/delete repeated.py: query row q (a train image) is a duplicate when some ref row (a test
    image) lies within the thresholds.  Returns ``(is_dup bool [M], match int64 [M])`` on the device; ``match[q]`` is the
    LOWEST matching ref row, -1 for none.  The reference keys its test hashes by hash value, so test images with equal
    hashes collapse to one path there and it reports whichever was stored last; here the lowest row is returned.
    ``caps``: ``ref_row_mask`` / ``max_pairs`` / ``cap`` as in ``hash_cross_matches``."""
    offsets, ref_idx, _ = hash_cross_matches(query_hashes, ref_hashes, thresholds, **caps)
    first = offsets[:-1]
    is_dup = offsets[1:] > first
    match = torch.full_like(first, -1)
    match[is_dup] = ref_idx[first[is_dup]]
    return is_dup, match
