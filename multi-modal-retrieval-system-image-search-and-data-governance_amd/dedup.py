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
``cross_set_duplicates`` the second, each by one integer-exact GPU join over all pairs (csrc/hash_join.hip).

The hashes themselves -- ``calculate_image_hashes``, tool/find_repeated_in_same_folder.py:8-22: imagehash's phash, dhash and
whash per file -- come from ``image_hashes``: decoded uint8 pixels on the GPU in, the joins' int64 ``[N, 3, W]`` tensor out,
every resized byte equal to Pillow's LANCZOS resize (csrc/image_hash.hip).  ``find_image_duplicates`` chains it with the
join and the keep-first pass; ``hashes_from_hex`` / ``hashes_to_hex`` convert to and from the strings the reference prints.
Decoding JPEG files into those pixels is ``jpeg.decode_jpeg``; MD5 stays with the caller.
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


# ---------------------------------------------------------------------------------------------------------------------
# Perceptual hashes of decoded images (csrc/image_hash.hip)

HASH_KINDS = ("phash", "dhash", "whash")        # the reference's tuple order; bit h of the C ABI's `kinds` mask is kind h
_image_table_cache = {}


def dct_cosine_table(hash_size: int) -> np.ndarray:
    """fp64 ``[hs, 4 hs]``: ``cos(pi (2x+1) v / 2n)``, n = 4 hs, by ``math.cos`` -- the numbers phash multiplies by, on the
    device and in any host restatement alike."""
    import math

    n = 4 * hash_size
    return np.array([[math.cos(math.pi * (2 * x + 1) * v / (2 * n)) for x in range(n)] for v in range(hash_size)], dtype=np.float64)


def whash_side(h: int, w: int, hash_size: int) -> int:
    """imagehash's whash ``image_scale``: the largest power of two <= min(w, h), at least ``hash_size``"""
    return max(1 << (min(h, w).bit_length() - 1), hash_size)


def _kinds_mask(kinds) -> Tuple[int, int]:
    kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
    if not kinds or len(set(kinds)) != len(kinds) or any(k not in HASH_KINDS for k in kinds):
        raise ValueError(f"kinds={kinds!r}: expected a non-empty selection of {HASH_KINDS} without repeats")
    if kinds != tuple(k for k in HASH_KINDS if k in kinds):
        raise ValueError(f"kinds={kinds!r} must keep the order of {HASH_KINDS}: the rows of the result follow it")
    return sum(1 << HASH_KINDS.index(k) for k in kinds), len(kinds)


def _check_hash_size(hash_size):
    if hash_size not in (8, 16):
        raise ValueError(f"hash_size={hash_size!r}: the device hashes are built for 8 and 16")


def _lanczos_device(in_size: int, out_size: int, device):
    """(bounds, coeffs, k) of the LANCZOS resize in_size -> out_size on ``device``, cached: image sizes repeat"""
    from .preprocess import resample_tables

    key = (in_size, out_size, str(device))
    hit = _image_table_cache.get(key)
    if hit is None:
        b, c, k = resample_tables(in_size, out_size, 0, out_size, filter="lanczos")
        hit = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device), k)
        if len(_image_table_cache) > 4096:
            _image_table_cache.clear()
        _image_table_cache[key] = hit
    return hit


def _cos_device(hash_size: int, device):
    key = ("cos", hash_size, str(device))
    hit = _image_table_cache.get(key)
    if hit is None:
        hit = _image_table_cache[key] = torch.from_numpy(dct_cosine_table(hash_size)).to(device)
    return hit


def _desc_dtype():
    """numpy view of mmr_image_hash_desc, field for field from the header"""
    from . import _lib

    return _lib.struct_dtype("mmr_image_hash_desc")


def _image_list(images):
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise ValueError(f"a batch tensor must be uint8 [B,H,W,3], got {tuple(images.shape)}")
        images = list(images.unbind(0))
    images = list(images)
    if not images:
        raise ValueError("empty batch")
    out = []
    for im in images:
        if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or not (im.dim() == 2 or (im.dim() == 3 and im.shape[2] == 3)):
            raise ValueError(f"expected uint8 [H,W,3] or [H,W] tensors, got {getattr(im, 'dtype', type(im))} "
                             f"{tuple(getattr(im, 'shape', ()))}")
        if not im.is_cuda:
            raise RuntimeError("images must live on the GPU (there is no CPU path)")
        if im.device != images[0].device:
            raise ValueError("images live on different devices")
        out.append(im.contiguous())
    return out


class ImageHashPlan:
    """One ``mmr_image_hashes`` call, prepared: descriptors and coefficient tables uploaded, workspace and outputs allocated.
    ``run()`` enqueues the three kernels on the current stream and returns ``(hashes int64 [B,K,W], status int32 [B])``, the
    plan's own buffers.  It allocates and copies nothing, so it can be captured in a graph and replayed after the pixels
    of ``images`` were overwritten in place.  ``debug=True`` keeps whash's resized S x S image of every row (``debug_w``)."""

    def __init__(self, images, hash_size: int = 8, kinds=HASH_KINDS, debug: bool = False):
        from . import _lib

        _check_hash_size(hash_size)
        self.mask, self.K = _kinds_mask(kinds)
        self.hash_size, self.images = hash_size, _image_list(images)
        L, dev = _lib.lib(), self.images[0].device
        if not hasattr(L, "mmr_image_hashes"):
            raise RuntimeError("this libmmr_hip.so has no image hashes: rebuild it")
        B = len(self.images)
        if B > 65535:
            raise ValueError(f"{B} images in one call; at most 65535 (image_hashes splits larger batches)")
        desc = np.zeros(B, dtype=_desc_dtype())
        self.tables, self.sizes, self.debug_w = [], [], []
        cos = _cos_device(hash_size, dev)
        off = 0
        for i, im in enumerate(self.images):
            h, w = int(im.shape[0]), int(im.shape[1])
            need = L.mmr_image_hash_scratch_bytes(h, w, hash_size, self.mask)
            if need == 0:
                raise ValueError(L.mmr_last_error().decode())
            S = whash_side(h, w, hash_size)
            d = desc[i]
            d["img"], d["H"], d["W"], d["channels"] = im.data_ptr(), h, w, 1 if im.dim() == 2 else 3
            for tag, ow, oh in (("d", hash_size + 1, hash_size), ("p", 4 * hash_size, 4 * hash_size), ("w", S, S)):
                hb, hc, hk = _lanczos_device(w, ow, dev)
                vb, vc, vk = _lanczos_device(h, oh, dev)
                self.tables += [hb, hc, vb, vc]
                d["hb_" + tag], d["hc_" + tag], d["hk_" + tag] = hb.data_ptr(), hc.data_ptr(), hk
                d["vb_" + tag], d["vc_" + tag], d["vk_" + tag] = vb.data_ptr(), vc.data_ptr(), vk
            d["cos_table"], d["scratch_off"] = cos.data_ptr(), off
            if debug and self.mask & 4:
                self.debug_w.append(torch.zeros(S, S, dtype=torch.uint8, device=dev))
                d["debug_w"] = self.debug_w[-1].data_ptr()
            self.sizes.append((h, w, off))
            off += need
        self.tables.append(cos)
        nbytes = L.mmr_image_hashes_workspace_bytes(desc.ctypes.data, B, hash_size, self.mask)
        if nbytes == 0:
            raise ValueError(L.mmr_last_error().decode())
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.desc = torch.from_numpy(desc.view(np.uint8).reshape(B, -1)).to(dev)
        self.hashes = torch.empty(B, self.K, hash_size * hash_size // 64, dtype=torch.int64, device=dev)
        self.status = torch.empty(B, dtype=torch.int32, device=dev)

    def run(self):
        from . import _lib

        _lib.check(_lib.lib().mmr_image_hashes(self.desc.data_ptr(), len(self.images), self.hash_size, self.mask,
                                               self.hashes.data_ptr(), self.status.data_ptr(), self.workspace.data_ptr(),
                                               self.workspace.numel(), _lib.stream_ptr(self.hashes.device)))
        return self.hashes, self.status

    def scratch(self, row: int):
        """Test aid: the intermediate results of image ``row`` after ``run()``, read back from the workspace:
        ``dict(sums int64 [hs,hs], dhash_plane uint8 [hs,hs+1], phash_plane uint8 [4hs,4hs], whash_image uint8 [S,S])``,
        the entries of the enabled kinds (``whash_image`` only with ``debug=True``)."""
        from . import _lib

        h, w, off = self.sizes[row]
        hs = self.hash_size
        o = (ctypes.c_int64 * 6)()
        _lib.check(_lib.lib().mmr_image_hash_scratch_layout(h, w, hs, self.mask, o))
        ws, out = self.workspace, {}
        if self.mask & 4:
            out["sums"] = ws[off + o[0]: off + o[0] + hs * hs * 8].view(torch.int64).reshape(hs, hs).clone()
            if self.debug_w:
                out["whash_image"] = self.debug_w[row]
        if self.mask & 2:
            out["dhash_plane"] = ws[off + o[1]: off + o[1] + hs * (hs + 1)].reshape(hs, hs + 1).clone()
        if self.mask & 1:
            out["phash_plane"] = ws[off + o[2]: off + o[2] + 16 * hs * hs].reshape(4 * hs, 4 * hs).clone()
        return out


def image_hashes(images, hash_size: int = 8, kinds=HASH_KINDS, return_status: bool = False,
                 max_workspace_bytes: int = 1 << 30):
    """imagehash's ``phash`` / ``dhash`` / ``whash`` (``hash_size`` 8 or 16, every other argument at its default) of decoded
    images, on the GPU: what tool/find_repeated_in_same_folder.py:8-19 computes per file on the CPU.

    ``images``: a list of uint8 ``[H_i, W_i, 3]`` (RGB) or ``[H_i, W_i]`` (greyscale, taken as Pillow's mode L) GPU tensors
    of any sizes up to 16384 a side, or one ``[B, H, W, 3]`` tensor.  Returns int64 ``[N, K, W]`` on the GPU -- the shape and
    bits of ``hashes_from_hex`` over ``str(imagehash)``, kinds in the order of ``kinds`` as a subset of
    ``("phash", "dhash", "whash")`` in that order -- and with ``return_status`` also int32 ``[N]``: bit 0, some phash
    coefficient lies within 2^-32 d[0][0] of the median (imagehash's own bit there depends on its summation order: flat and
    1 x 1 images); bit 1, whash's two middle block sums are equal (imagehash's bits of the blocks equal to the median are
    noise; here they are 0).  Every resized byte equals Pillow's LANCZOS resize; dhash and whash are integer work, phash
    compares fp64 sums with a margin.
    The batch is split into calls whose workspace (about ``H * (5 hs + 1 + S)`` bytes per image) fits
    ``max_workspace_bytes``; one image that does not fit alone is a MemoryError."""
    from . import _lib

    _check_hash_size(hash_size)
    mask, _ = _kinds_mask(kinds)
    imgs = _image_list(images)
    L = _lib.lib()
    if not hasattr(L, "mmr_image_hashes"):
        raise RuntimeError("this libmmr_hip.so has no image hashes: rebuild it")
    chunks, cur, used = [], [], 0
    for im in imgs:
        need = L.mmr_image_hash_scratch_bytes(int(im.shape[0]), int(im.shape[1]), hash_size, mask)
        if need == 0:
            raise ValueError(L.mmr_last_error().decode())
        if need > max_workspace_bytes:
            raise MemoryError(f"one {tuple(im.shape)} image needs {need} bytes of workspace, above max_workspace_bytes={max_workspace_bytes}")
        if cur and (used + need > max_workspace_bytes or len(cur) == 65535):
            chunks.append(cur)
            cur, used = [], 0
        cur.append(im)
        used += need
    chunks.append(cur)
    hs_, st_ = [], []
    for chunk in chunks:
        h, s = ImageHashPlan(chunk, hash_size, kinds).run()
        hs_.append(h)
        st_.append(s)
    hashes = hs_[0] if len(hs_) == 1 else torch.cat(hs_)
    status = st_[0] if len(st_) == 1 else torch.cat(st_)
    return (hashes, status) if return_status else hashes


def hashes_to_hex(hashes, hash_size: int):
    """The inverse of ``hashes_from_hex``: int64 ``[N, K, W]`` (or ``[N, K]``, W = 1) -> N tuples of K strings, each what
    ``str(imagehash)`` prints for that hash: ``hash_size**2 / 4`` lowercase hex digits, big-endian.  ``hash_size`` 8 wants
    W = 1 and 16 wants W = 4."""
    _check_hash_size(hash_size)
    h = hashes.detach().cpu().numpy() if isinstance(hashes, torch.Tensor) else np.asarray(hashes)
    if h.dtype != np.int64:
        raise ValueError(f"hashes must be int64 (uint64 bits), got {h.dtype}")
    if h.ndim == 2:
        h = h[:, :, None]
    W = hash_size * hash_size // 64
    if h.ndim != 3 or h.shape[2] != W:
        raise ValueError(f"hashes of shape {tuple(h.shape)} do not hold hash_size={hash_size} hashes: expected [N, K, {W}]")
    u = np.ascontiguousarray(h).view(np.uint64)
    return [tuple("".join(f"{int(word):016x}" for word in kind) for kind in row) for row in u]


def find_image_duplicates(keys: Sequence, images, thresholds=5, order: Optional[Sequence[int]] = None, **kw):
    """``find_and_remove_duplicate_images`` (tool/find_repeated_in_same_folder.py:59-105) from decoded pixels:
    ``image_hashes(images, **kw)`` followed by ``find_hash_duplicates``.  ``keys[r]`` names image r; returns the reference's
    list ``[(duplicate_key, kept_key), ...]`` in visit order.  ``kw``: ``hash_size`` / ``kinds`` / ``max_workspace_bytes``."""
    n = len(keys)
    count = images.shape[0] if isinstance(images, torch.Tensor) else len(images)
    if count != n:
        raise ValueError(f"{n} keys for {count} images")
    kw.pop("return_status", None)
    return find_hash_duplicates(keys, image_hashes(images, **kw), thresholds, order)
