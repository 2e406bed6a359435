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
"""
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
