"""Similarity, L2-normalise and top-k over an embedding gallery -- the "search" half of the hot path.

Host-side mirror of the tensor expressions the reference writes inline:
    similarity = 100. * features.cuda() @ ref_feature.t()      reference code/search_image.py:107
    image_features /= image_features.norm(dim=-1, keepdim=True) reference code/search_image.py:133,157
    output.topk(topk, 1, True, True)                            reference code/utils.py:17
All arithmetic runs in csrc/search.hip through the C ABI (include/mmr.h); torch only owns the
device memory, the stream and (for the sharded index) the RCCL process group.
"""
from typing import Callable, Optional, Tuple

import torch

from . import _lib, _retry


def _as_2d(x: torch.Tensor) -> Tuple[torch.Tensor, bool]:
    if x.dim() == 1:
        return x.unsqueeze(0), True
    if x.dim() != 2:
        raise ValueError(f"expected a 1-D or 2-D tensor, got shape {tuple(x.shape)}")
    return x, False


# dtypes the kernels read as they are; anything else is widened to fp32.  fp16 (what the reference keeps on disk) has
# kernels of its own: no copy, and the ranking is that of the caller's data
_NATIVE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)

def _prep_pair(q: torch.Tensor, gallery: torch.Tensor):
    if not gallery.is_cuda:
        raise RuntimeError("gallery must live on the GPU (there is no CPU path)")
    if gallery.dtype not in _NATIVE_DTYPES:
        gallery = gallery.to(torch.float32)
    q = q.to(device=gallery.device, dtype=gallery.dtype)
    return q.contiguous(), gallery.contiguous()


def l2_normalize(x: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """Row-wise ``x / x.norm(dim=-1, keepdim=True)`` (no epsilon, as the reference)."""
    x2, squeezed = _as_2d(x)
    out = x2 if (inplace and x2.is_contiguous()) else x2.contiguous().clone()
    L = _lib.lib()
    _lib.check(L.mmr_l2norm_rows(out.data_ptr(), _lib.dtype_code(out.dtype), out.shape[0], out.shape[1],
                                 _lib.stream_ptr(out.device)))
    if inplace and out is not x2:
        x2.copy_(out)
        out = x2
    return out.squeeze(0) if squeezed else out


def similarity(features: torch.Tensor, ref_feature: torch.Tensor, scale: float = 100.0) -> torch.Tensor:
    """``scale * features @ ref_feature.t()`` -> fp32 [N] (1-D ref) or [N,Q] (2-D ref).

    Same shape convention as reference code/search_image.py:107; the query is NOT normalised
    here (the reference also scores with an un-normalised mean vector, search_image.py:315,387).
    Materialises the score matrix, so it is meant for the reference's small galleries;
    use ``cosine_topk`` for large ones.
    """
    r2, squeezed = _as_2d(ref_feature)
    if features.is_cuda and r2.dtype != features.dtype:
        # mixed precision (e.g. bf16 cache rows scored against an fp32 mean vector): this is the
        # small-gallery API, so widen both operands to fp32 rather than round the reference vector
        features = features.to(torch.float32)
        r2 = r2.to(torch.float32)
    q, g = _prep_pair(r2, features)
    Q, E = q.shape
    N = g.shape[0]
    out = torch.empty(Q, N, dtype=torch.float32, device=g.device)
    L = _lib.lib()
    _lib.check(L.mmr_similarity(q.data_ptr(), g.data_ptr(), _lib.dtype_code(g.dtype), Q, N, E, float(scale),
                                out.data_ptr(), _lib.stream_ptr(g.device)))
    return out[0] if squeezed else out.t()


def tip_adapter_logits(features: torch.Tensor, clip_weights: torch.Tensor, cache_keys: torch.Tensor,
                       cache_values: torch.Tensor, alpha: float, beta: float, return_clip_logits: bool = False):
    """Fused Tip-Adapter scoring (reference code/main_custom.py:111,124-127):

        clip_logits  = 100. * features @ clip_weights                      # clip_weights [E,C]
        affinity     = features @ cache_keys                               # cache_keys   [E,S]
        cache_logits = ((-1) * (beta - beta * affinity)).exp() @ cache_values * 10     # values [S,C]
        tip_logits   = clip_logits + cache_logits * alpha

    Returns fp32 ``tip_logits [N,C]`` (and ``clip_logits``).  The [N,S] affinity matrix is never written.
    """
    if not features.is_cuda:
        raise RuntimeError("features must live on the GPU (there is no CPU path)")
    dt = features.dtype if features.dtype in _NATIVE_DTYPES else torch.float32
    if clip_weights.dtype != dt or cache_keys.dtype != dt:
        dt = torch.float32
    dev = features.device
    f = features.to(dt).contiguous()
    wt = clip_weights.to(dev, dt).t().contiguous()                 # [C,E]
    kt = cache_keys.to(dev, dt).t().contiguous()                   # [S,E]
    v = cache_values.to(dev, torch.float32).contiguous()           # [S,C]
    N, E = f.shape
    C, S = wt.shape[0], kt.shape[0]
    if wt.shape[1] != E or kt.shape[1] != E or v.shape != (S, C):
        raise ValueError(f"shape mismatch: features {tuple(f.shape)}, clip_weights {tuple(clip_weights.shape)}, "
                         f"cache_keys {tuple(cache_keys.shape)}, cache_values {tuple(cache_values.shape)}")
    tip = torch.empty(N, C, dtype=torch.float32, device=dev)
    clip = torch.empty(N, C, dtype=torch.float32, device=dev) if return_clip_logits else None
    L = _lib.lib()
    _lib.check(L.mmr_tip_adapter_logits(f.data_ptr(), wt.data_ptr(), kt.data_ptr(), v.data_ptr(), _lib.dtype_code(dt),
                                        N, E, C, S, float(alpha), float(beta), tip.data_ptr(), _lib.ptr(clip),
                                        _lib.stream_ptr(dev)))
    return (tip, clip) if return_clip_logits else tip


def gallery_norm_bound(gallery: torch.Tensor) -> torch.Tensor:
    """Largest row L2 norm of ``gallery`` as a 1-element fp32 DEVICE tensor (no host sync): what sizes the
    margin of the fast path's exactness certificate.  One HBM-bound pass."""
    if not gallery.is_cuda:
        raise RuntimeError("gallery must live on the GPU (there is no CPU path)")
    g = gallery.contiguous()
    out = torch.empty(1, dtype=torch.float32, device=g.device)
    L = _lib.lib()
    _lib.check(L.mmr_gallery_norm_bound(g.data_ptr(), _lib.dtype_code(g.dtype), g.shape[0], g.shape[1], out.data_ptr(),
                                        _lib.stream_ptr(g.device)))
    return out


def _check_row_mask(row_mask, N: int, device) -> None:
    """A row mask is a bool tensor [N] on the gallery's device (None: no mask).  Checked before any launch."""
    if row_mask is None:
        return
    if not isinstance(row_mask, torch.Tensor):
        raise ValueError(f"row_mask must be a bool tensor, got {type(row_mask).__name__}")
    if row_mask.dtype != torch.bool:
        raise ValueError(f"row_mask must be a bool tensor, got {row_mask.dtype}")
    if tuple(row_mask.shape) != (N,):
        raise ValueError(f"row_mask has shape {tuple(row_mask.shape)}, the gallery has {N} rows")
    if row_mask.device != torch.device(device):
        raise ValueError(f"row_mask lives on {row_mask.device}, the gallery on {device}")


def _pack_row_mask(keep: torch.Tensor, and_words: Optional[torch.Tensor], N: int, out: Optional[torch.Tensor] = None):
    """bool [N] (AND the packed words ``and_words``) -> the C ABI's mask words, int32 [ceil(N/32)], by one
    mmr_row_mask_pack launch (no host read).  ``out``: written in place when given."""
    nw = max((N + 31) // 32, 1)
    if out is None:
        out = torch.empty(nw, dtype=torch.int32, device=keep.device)
    keep = keep.contiguous()
    _lib.check(_lib.lib().mmr_row_mask_pack(keep.data_ptr(), _lib.ptr(and_words), N, out.data_ptr(),
                                            _lib.stream_ptr(keep.device)))
    return out


def _check_row_masks(row_masks, Q: int, N: int, E: int, device, return_status: bool = False) -> None:
    """``row_masks=`` of the top-k calls: a bool tensor [Q, N] on the gallery's device, or a ``DecisionMasks`` of Q rows over N
    gallery rows there (None: none).  Checked before any launch, with what the per-query call cannot do."""
    if row_masks is None:
        return
    if return_status:
        raise ValueError("row_masks: the per-query call has no certificate and returns no status (return_status=True)")
    if E == 1024:
        raise ValueError("row_masks: E=1024 has no MFMA scan, which the per-query calls are built on")
    dev = torch.device(device)
    if isinstance(row_masks, DecisionMasks):
        w = row_masks.words
        nw = max((N + 31) // 32, 1)
        if row_masks.num_rows != N or w.dim() != 2 or w.shape[0] != Q or w.shape[1] < nw or w.dtype != torch.int32:
            raise ValueError(f"row_masks: decision masks of {tuple(w.shape)} {w.dtype} words over {row_masks.num_rows} rows, "
                             f"the call has {Q} queries over {N} rows")
        if w.device != dev:
            raise ValueError(f"row_masks live on {w.device}, the gallery on {dev}")
        return
    if not isinstance(row_masks, torch.Tensor):
        raise ValueError(f"row_masks must be a bool tensor [Q, N] or DecisionMasks, got {type(row_masks).__name__}")
    if row_masks.dtype != torch.bool:
        raise ValueError(f"row_masks must be a bool tensor, got {row_masks.dtype}")
    if tuple(row_masks.shape) != (Q, N):
        raise ValueError(f"row_masks has shape {tuple(row_masks.shape)}, the call has {Q} queries over {N} rows")
    if row_masks.device != dev:
        raise ValueError(f"row_masks live on {row_masks.device}, the gallery on {dev}")


def _pack_row_masks(keep: torch.Tensor, N: int) -> torch.Tensor:
    """bool [Q, N] -> int32 words [Q, ceil(N/32)] in the C ABI's mask format.  On the GPU one mmr_row_masks_pack launch (no
    host read); a CPU tensor (building masks ahead of time) is packed with tensor arithmetic."""
    Q = keep.shape[0]
    nw = max((N + 31) // 32, 1)
    if keep.is_cuda:
        out = torch.empty(Q, nw, dtype=torch.int32, device=keep.device)
        if Q:
            keep = keep.contiguous()
            _lib.check(_lib.lib().mmr_row_masks_pack(keep.data_ptr(), None, Q, N, nw, out.data_ptr(), _lib.stream_ptr(keep.device)))
        return out
    bits = torch.zeros(Q, nw * 32, dtype=torch.int64)
    bits[:, :N] = keep.to(torch.int64)
    v = (bits.reshape(Q, nw, 32) << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(v >= 1 << 31, v - (1 << 32), v).to(torch.int32)


def _row_masks_words(row_masks, N: int):
    """(words int32 [Q, >= W], stride in words) of checked ``row_masks``: a DecisionMasks' words in place, no copy (a view
    whose rows are not contiguous is copied once); a bool tensor packed by one launch."""
    if isinstance(row_masks, DecisionMasks):
        w = row_masks.words
        if w.shape[1] > 1 and w.stride(1) != 1 or (w.shape[0] > 1 and w.stride(0) < w.shape[1]):
            w = w.contiguous()
        return w, (w.stride(0) if w.shape[0] > 1 else w.shape[1])
    w = _pack_row_masks(row_masks, N)
    return w, w.shape[1]


def _split_fp32(g: torch.Tensor):
    """(hi, lo, resid_bound) of an fp32 gallery: mmr_gallery_split_bf16 into fresh arrays."""
    hi = torch.empty(g.shape, dtype=torch.bfloat16, device=g.device)
    lo = torch.empty(g.shape, dtype=torch.bfloat16, device=g.device)
    resid = torch.zeros(1, dtype=torch.float32, device=g.device)
    _lib.check(_lib.lib().mmr_gallery_split_bf16(g.data_ptr(), g.shape[0], g.shape[1], hi.data_ptr(), lo.data_ptr(),
                                                 resid.data_ptr(), _lib.stream_ptr(g.device)))
    return hi, lo, resid


def leave_out_masks(Q: int, N: int, query_ids, row_ids, device=None) -> "DecisionMasks":
    """Q all-ones masks over N rows with the listed (query, row) pairs cleared, ready for ``row_masks=``: the reference's
    "take a class's sample images out of that class's own gallery" (``construct_dataset``, code/search_image.py:167-182)
    for every query of a batch at once -- pair (q, r) keeps row r out of query q's gallery and in everybody else's."""
    qi = torch.as_tensor(query_ids, dtype=torch.int64).reshape(-1)
    ri = torch.as_tensor(row_ids, dtype=torch.int64).reshape(-1)
    if qi.numel() != ri.numel():
        raise ValueError(f"{qi.numel()} query ids for {ri.numel()} row ids")
    if qi.numel() and (int(qi.min()) < 0 or int(qi.max()) >= Q or int(ri.min()) < 0 or int(ri.max()) >= N):
        raise ValueError(f"pairs must lie in [0, {Q}) x [0, {N})")
    dev = torch.device("cpu") if device is None else torch.device(device)
    keep = torch.ones(Q, N, dtype=torch.bool, device=dev)
    keep[qi.to(dev), ri.to(dev)] = False
    return DecisionMasks.from_bool(keep)


def _norm_bound_arg(norm_bound) -> float:
    """The C calls' gallery_norm_bound: the caller's bound, 0.0 for none (None or <= 0: measured, or the device scalar)."""
    nb = 0.0 if norm_bound is None else float(norm_bound)
    if nb != nb or nb == float("inf"):
        raise ValueError("gallery_norm_bound must be finite")
    return nb


def _split_parts(split, g):
    """(hi, lo, resid_bound) of a pre-split fp32 gallery (mmr_gallery_split_bf16); three Nones for any other gallery."""
    if split is not None and g.dtype == torch.float32:
        return split
    return None, None, None


def _workspace(need: int, dev, have: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``have`` when it holds ``need`` bytes (a caller's workspace only ever grows), else ``max(need, 256)`` new bytes."""
    if have is None or have.numel() < need:
        return torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    return have


def _local_topk(q, g, k, scale, norm_bound, want_dot64, want_status, workspace=None, norm_bound_dev=None, split=None,
                row_mask_words=None):
    """norm_bound: caller's bound (None / <= 0: none); norm_bound_dev: measured device scalar (None: none).
    Neither given -> the C call measures the gallery itself.  split: (hi, lo, resid_bound) of an fp32 gallery
    (mmr_gallery_split_bf16: two bf16 arrays and the device scalar max_row |g - hi|) -> the tiered split search
    (same results).  row_mask_words: packed row mask (_pack_row_mask) -> the *_masked calls; None: the unmasked ones."""
    Q, E = q.shape
    N = g.shape[0]
    dev = g.device
    L = _lib.lib()
    workspace = _workspace(L.mmr_search_workspace_bytes(N, E, Q, k), dev, workspace)
    idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
    score = torch.empty(Q, k, dtype=torch.float32, device=dev)
    dot64 = torch.empty(Q, k, dtype=torch.float64, device=dev) if want_dot64 else None
    status = torch.empty(Q, dtype=torch.int32, device=dev) if want_status else None
    nb = _norm_bound_arg(norm_bound)
    hi, lo, resid = _split_parts(split, g)
    outs = (idx.data_ptr(), score.data_ptr(), _lib.ptr(dot64), _lib.ptr(status), workspace.data_ptr(), workspace.numel(),
            _lib.stream_ptr(dev))
    if hi is not None:
        head = (q.data_ptr(), g.data_ptr(), hi.data_ptr(), lo.data_ptr(), _lib.ptr(resid), Q, N, E, k, float(scale), nb,
                _lib.ptr(norm_bound_dev))
        if row_mask_words is not None:
            _lib.check(L.mmr_cosine_topk_split_masked(*head, row_mask_words.data_ptr(), *outs))
        else:
            _lib.check(L.mmr_cosine_topk_split(*head, *outs))
    else:
        head = (q.data_ptr(), g.data_ptr(), _lib.dtype_code(g.dtype), Q, N, E, k, float(scale), nb, _lib.ptr(norm_bound_dev))
        if row_mask_words is not None:
            _lib.check(L.mmr_cosine_topk_masked(*head, row_mask_words.data_ptr(), *outs))
        else:
            _lib.check(L.mmr_cosine_topk_ex(*head, *outs))
    return idx, score, dot64, status, workspace


def cosine_topk(queries: torch.Tensor, gallery: torch.Tensor, k: int = 10, scale: float = 1.0,
                gallery_norm_bound: Optional[float] = None, return_dot64: bool = False, return_status: bool = False,
                row_mask: Optional[torch.Tensor] = None, row_masks=None):
    """Top-k gallery rows per query, like ``(scale * queries @ gallery.t()).topk(k, 1, True, True)``.

    Returns ``(values fp32 [Q,k], indices int64 [Q,k])`` -- torch.topk's order of results -- plus
    the exact fp64 dots and/or the per-query path status when asked.  Ranking is by
    (-dot, +row index) on fp64 dot products, so ties go to the lowest row id (torch's CPU tie
    order is unspecified) and indices are bit-reproducible against oracle/search_ref.c.
    Empty slots (k > N) hold index -1 / score -inf.  ``k`` goes up to 64; ``cosine_topk_deep`` answers k up to 4096.

    ``gallery_norm_bound`` (an upper bound on any row's L2 norm) sizes the certificate of the fast path.
    Left at None it is MEASURED from the gallery in the same call (one extra streaming pass; a
    ``GalleryIndex`` measures once); a caller who passes a number promises it holds (include/mmr.h).

    ``row_mask`` (bool [N] on the gallery's device): search only the rows where it is True.  The result is exactly the
    one over ``gallery[row_mask]`` with ids mapped back to the original rows; no copy is made (the mask is packed by one
    kernel launch and the scans skip the dead rows).  The norm bound stays a bound over all N rows.

    ``row_masks``: one mask per query (``cosine_topk_deep``'s docstring); the call is then answered by the deep top-k for
    any k, with the same results.  It has no status: ``return_status=True`` with it is a ValueError, and so is E = 1024.
    """
    q2, squeezed = _as_2d(queries)
    if row_masks is not None:
        if gallery.dim() == 2 and q2.shape[1] == gallery.shape[1]:
            _check_row_masks(row_masks, q2.shape[0], gallery.shape[0], gallery.shape[1], gallery.device, return_status)
        return cosine_topk_deep(queries, gallery, k, scale, gallery_norm_bound, return_dot64, row_mask, row_masks=row_masks)
    q, g = _prep_pair(q2, gallery)
    if q.shape[1] != g.shape[1]:
        raise ValueError(f"query dim {q.shape[1]} != gallery dim {g.shape[1]}")
    _check_row_mask(row_mask, g.shape[0], g.device)
    words = None if row_mask is None else _pack_row_mask(row_mask, None, g.shape[0])
    idx, score, dot64, status, _ = _local_topk(q, g, int(k), scale, gallery_norm_bound, return_dot64, return_status,
                                               row_mask_words=words)
    idx = idx.to(torch.int64)
    if squeezed:
        idx, score = idx[0], score[0]
        dot64 = dot64[0] if dot64 is not None else None
    out = (score, idx)
    if return_dot64:
        out = out + (dot64,)
    if return_status:
        out = out + (status,)
    return out


_RANGE_CAND_INIT = 1 << 16          # first candidate-list capacity; a call that needs more retries once with the count
_RANGE_MAX_PAIRS = 1 << 27          # default ceiling on the candidate list a call may allocate (16 B of workspace per pair)


def _range_call(q, g, threshold, scale, norm_bound, norm_bound_dev, split, cap, cand_cap, max_pairs, row_mask_words=None):
    """mmr_cosine_range (q given) or mmr_gallery_self_join (q None) under ``_retry.run``, with the output capacity ``cap``
    and the candidate capacity ``cand_cap``.  -> (first ids int32 [P], second ids int32 [P], score fp32 [P], dot64 fp64 [P]),
    sorted.  row_mask_words: packed row mask -> the *_masked calls."""
    thr = float(threshold)
    if thr != thr or thr in (float("inf"), float("-inf")):
        raise ValueError(f"threshold must be finite (got {threshold})")
    nb = _norm_bound_arg(norm_bound)
    N, E = g.shape
    Q = 0 if q is None else q.shape[0]
    dev = g.device
    hi, _, resid = _split_parts(split, g)
    code = _lib.dtype_code(g.dtype)
    L = _lib.lib()
    cand_cap = int(cand_cap) if cand_cap else _RANGE_CAND_INIT
    cap = cand_cap if cap is None else int(cap)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    mask = () if row_mask_words is None else (row_mask_words.data_ptr(),)
    if q is None:
        call = L.mmr_gallery_self_join_masked if mask else L.mmr_gallery_self_join
        head = (g.data_ptr(), _lib.ptr(hi), code, N, E, thr)
    else:
        call = L.mmr_cosine_range_masked if mask else L.mmr_cosine_range
        head = (q.data_ptr(), g.data_ptr(), _lib.ptr(hi), code, Q, N, E, thr)
    outs = None

    def launch(cap, cand_cap):
        nonlocal outs
        ws = _workspace(L.mmr_range_workspace_bytes(N, E, Q, cand_cap, code, int(hi is not None)), dev)
        outs = [torch.empty(max(cap, 1), dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32, torch.float64)]
        _lib.check(call(*head, float(scale), nb, _lib.ptr(norm_bound_dev), _lib.ptr(resid), *mask, cap, cand_cap,
                        *(o.data_ptr() for o in outs), counts.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
        return counts.tolist()

    # an overflowed candidate list undercounts the matches; the matches never outnumber the candidates
    matches, _ = _retry.run(launch, (cap, cand_cap), max_pairs,
                            lambda c, caps: f"range search: counts {c[0]}/{c[1]} exceed the capacities {caps[0]}/{caps[1]} it reported",
                            lambda need: f"range search at threshold {thr} needs room for {need[1]} candidate pairs, above "
                                         f"max_pairs={max_pairs}: raise the threshold or max_pairs",
                            needed=lambda caps, c: (c[1] if c[1] > caps[1] else c[0], c[1]))
    return tuple(o[:matches] for o in outs)


DEEP_K_MAX = _lib.HEADER.constants["MMR_DEEP_K_MAX"]
_DEEP_SLACK = 4096                  # first capacities: 2 * Q * k + this (see _deep_call)


def _deep_call(q, g, k, scale, norm_bound, norm_bound_dev, split, row_mask_words, max_pairs, tile_cap, surv_cap,
               want_dot64, workspace=None, qmasks=None):
    """mmr_cosine_topk_deep under ``_retry.run``, with the capacities of the tile list and of the survivor list.
    -> (idx int64 [Q,k], score fp32 [Q,k], dot64 fp64 [Q,k] or None, workspace, the last call's counts).

    First capacities: the call lists at least min(k, tiles) (query, tile) pairs per query and keeps at least
    min(k, live rows) survivors; on scattered data both counts stay within 1.7 * Q * k until k nears the number of tiles
    ("deep top-k"), so ``2 * Q * k + 4096`` entries (8 + 32 bytes each) answer those without a
    retry.  Neither list can outgrow ``Q * tiles`` / ``Q * N``, so the capacities stop there.  An overflowed tile list
    undercounts the survivors, which never exceed a tile's rows per listed pair: the retry sizes them by that bound.
    First capacities above ``max_pairs`` raise MemoryError as the retry's do, before any call.  ``qmasks``: (words, stride)
    of per-query masks (``_row_masks_words``) -> mmr_cosine_topk_deep_qmasked, with ``row_mask_words`` as the mask all
    queries share; an fp32 gallery then needs ``split``.
    """
    if not 1 <= k <= DEEP_K_MAX:
        raise ValueError(f"k={k} outside [1, {DEEP_K_MAX}]")
    nb = _norm_bound_arg(norm_bound)
    N, E = g.shape
    Q = q.shape[0]
    dev = g.device
    hi, lo, resid = _split_parts(split, g)
    tile_rows = 16 if (g.dtype == torch.float32 and hi is None) else 32
    max_tiles = max(Q * ((N + tile_rows - 1) // tile_rows), 1)
    max_surv = max(Q * N, 1)
    # fewer tiles than k: the call lists every tile and keeps every row (include/mmr.h), so start there
    first = max(max_tiles, max_surv) if k * tile_rows >= N else 2 * Q * k + _DEEP_SLACK
    tile_cap = min(int(tile_cap) if tile_cap else first, max_tiles)
    surv_cap = min(int(surv_cap) if surv_cap else first, max_surv)
    if tile_cap < 1 or surv_cap < 1:
        raise ValueError("tile_cap and surv_cap must be >= 1")
    if max(tile_cap, surv_cap) > max_pairs:
        raise MemoryError(f"deep top-k with k={k}: first capacities {tile_cap} tiles / {surv_cap} rows exceed max_pairs={max_pairs}"
                          f": lower k, pass tile_cap / surv_cap, or raise max_pairs")
    L = _lib.lib()
    idx = torch.empty(Q, k, dtype=torch.int64, device=dev)
    score = torch.empty(Q, k, dtype=torch.float32, device=dev)
    dot64 = torch.empty(Q, k, dtype=torch.float64, device=dev) if want_dot64 else None
    if Q == 0:
        return idx, score, dot64, workspace, (0, 0)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    code = _lib.dtype_code(g.dtype)
    head = (q.data_ptr(), g.data_ptr(), _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(resid), code, Q, N, E, k, float(scale), nb,
            _lib.ptr(norm_bound_dev))
    qm = () if qmasks is None else (qmasks[0].data_ptr(), int(qmasks[1]))
    call = L.mmr_cosine_topk_deep_qmasked if qm else L.mmr_cosine_topk_deep
    ws_bytes = L.mmr_deep_topk_qmasked_workspace_bytes if qm else L.mmr_deep_topk_workspace_bytes

    def launch(tile_cap, surv_cap):
        nonlocal workspace
        workspace = _workspace(ws_bytes(N, E, Q, k, tile_cap, surv_cap, code, int(hi is not None)), dev, workspace)
        _lib.check(call(*head, *qm, _lib.ptr(row_mask_words), tile_cap, surv_cap, idx.data_ptr(), score.data_ptr(), _lib.ptr(dot64),
                        counts.data_ptr(), workspace.data_ptr(), workspace.numel(), _lib.stream_ptr(dev)))
        return counts.tolist()

    listed, surv = _retry.run(launch, (tile_cap, surv_cap), max_pairs,
                              lambda c, caps: f"deep top-k: counts {c[0]}/{c[1]} exceed the capacities {caps[0]}/{caps[1]} it reported",
                              lambda need: f"deep top-k with k={k} needs room for {need[0]} listed tiles and up to {need[1]} surviving "
                                           f"rows, above max_pairs={max_pairs}: lower k or raise max_pairs",
                              needed=lambda caps, c: (c[0], min(c[0] * tile_rows, max_surv) if c[0] > caps[0] else c[1]))
    return idx, score, dot64, workspace, (listed, surv)


def _check_deep_args(q2, gallery, k, row_mask, row_masks=None) -> None:
    """Shapes, k and the row masks of a deep top-k call, before anything touches the device."""
    if gallery.dim() != 2:
        raise ValueError(f"gallery must be 2-D, got shape {tuple(gallery.shape)}")
    if q2.shape[1] != gallery.shape[1]:
        raise ValueError(f"query dim {q2.shape[1]} != gallery dim {gallery.shape[1]}")
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= DEEP_K_MAX:
        raise ValueError(f"k={k} outside [1, {DEEP_K_MAX}]")
    _check_row_mask(row_mask, gallery.shape[0], gallery.device)
    _check_row_masks(row_masks, q2.shape[0], gallery.shape[0], gallery.shape[1], gallery.device)


def _deep_out(squeezed, idx, score, dot64, return_dot64):
    if squeezed:
        idx, score = idx[0], score[0]
        dot64 = dot64[0] if dot64 is not None else None
    return (score, idx, dot64) if return_dot64 else (score, idx)


def cosine_topk_deep(queries: torch.Tensor, gallery: torch.Tensor, k: int, scale: float = 1.0,
                     gallery_norm_bound: Optional[float] = None, return_dot64: bool = False,
                     row_mask: Optional[torch.Tensor] = None, *, max_pairs: int = _RANGE_MAX_PAIRS,
                     tile_cap: Optional[int] = None, surv_cap: Optional[int] = None, row_masks=None):
    """``cosine_topk`` for ``1 <= k <= 4096``: recall@100, re-rank shortlists, k-NN lists -- the reference's
    ``np.argsort(d)[:shots]`` with an open ``shots`` -- without the [Q,N] score matrix.

    Returns ``(values fp32 [Q,k], indices int64 [Q,k][, dot64 fp64 [Q,k]])``, ranked by (-dot64, +row index) on the
    fixed-order fp64 dots: bit for bit ``cosine_topk``'s result where both accept ``k``, and oracle/search_ref.c's for
    every k.  Empty slots (k above the rows a query can return) hold -1 / -inf / -inf.  ``gallery_norm_bound`` and
    ``row_mask`` as in ``cosine_topk``.  A 1-D query gives 1-D results.

    One pass over the gallery leaves the per-tile maxima of the approximate scores; their k-th largest per query, less
    the scan's error margin, is a threshold no top-k row can fall under, and only the tiles that reach it are re-scored in
    fp64 (include/mmr.h).  ``tile_cap`` / ``surv_cap``: first capacities of the tile and survivor lists (default
    ``2*Q*k + 4096``); a call that reports more is repeated once at the reported sizes, unless they exceed ``max_pairs``
    (MemoryError) -- a query that ties with every row lists the whole gallery.

    ``row_masks``: a mask PER QUERY -- a bool tensor [Q, N] on the gallery's device (packed by one launch) or a
    ``DecisionMasks`` of Q rows over the gallery (``cosine_decide``, ``leave_out_masks``; its words are used in place).
    Row q of the result is exactly this call for query q alone with ``row_mask = row_masks[q]`` (AND ``row_mask`` when
    both are given), in one pass over the gallery for all queries.  An fp32 gallery is split into bf16 halves for the
    call (a ``GalleryIndex`` keeps its split).
    """
    q2, squeezed = _as_2d(queries)
    _check_deep_args(q2, gallery, k, row_mask, row_masks)
    q, g = _prep_pair(q2, gallery)
    words = None if row_mask is None else _pack_row_mask(row_mask, None, g.shape[0])
    qmasks = split = None
    if row_masks is not None:
        qmasks = _row_masks_words(row_masks, g.shape[0])
        split = _split_fp32(g) if g.dtype == torch.float32 else None
    idx, score, dot64, _, _ = _deep_call(q, g, int(k), scale, gallery_norm_bound, None, split, words, max_pairs, tile_cap,
                                         surv_cap, return_dot64, qmasks=qmasks)
    return _deep_out(squeezed, idx, score, dot64, return_dot64)


def _csr(qids: torch.Tensor, Q: int) -> torch.Tensor:
    counts = torch.bincount(qids.to(torch.int64), minlength=Q)
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=qids.device), torch.cumsum(counts, 0)])


def _range_out(Q, squeezed, qids, rows, score, dot64, return_dot64):
    idx = rows.to(torch.int64)
    out = (idx, score) if squeezed else (_csr(qids, Q), idx, score)
    return out + (dot64,) if return_dot64 else out


def cosine_range(queries: torch.Tensor, gallery: torch.Tensor, threshold: float, scale: float = 1.0,
                 gallery_norm_bound: Optional[float] = None, return_dot64: bool = False, *,
                 max_pairs: int = _RANGE_MAX_PAIRS, cap: Optional[int] = None, cand_cap: Optional[int] = None,
                 row_mask: Optional[torch.Tensor] = None):
    """Every gallery row whose dot product with a query is at least ``threshold`` -- the reference's
    ``get_similarity`` + threshold (code/search_image.py:58-117) without the [Q,N] score matrix.

    ``threshold`` applies to the UNSCALED fp64 dot (the cosine for unit rows; the reference's ``100*cos >= t`` is
    ``threshold=t/100``); the decision and the returned ``dot64`` are bit-identical to a brute-force fp64 evaluation in
    oracle/search_ref.c's order, and ``scores = (float)(dot64 * scale)``.

    Returns CSR ``(offsets int64 [Q+1], idx int64 [P], scores fp32 [P])`` (+ ``dot64`` fp64 [P]): the matches of query q
    are ``idx[offsets[q]:offsets[q+1]]``, rows ascending.  A 1-D query gives ``(idx, scores[, dot64])``.
    ``cap`` / ``cand_cap`` are the first call's output and candidate capacities; when the call reports more, it is
    repeated once at the reported size, unless that exceeds ``max_pairs`` (MemoryError).
    ``row_mask`` (bool [N] on the gallery's device): only rows where it is True match (as ``cosine_topk``'s).
    """
    q2, squeezed = _as_2d(queries)
    q, g = _prep_pair(q2, gallery)
    if q.shape[1] != g.shape[1]:
        raise ValueError(f"query dim {q.shape[1]} != gallery dim {g.shape[1]}")
    _check_row_mask(row_mask, g.shape[0], g.device)
    Q = q.shape[0]
    if Q == 0:
        e = torch.empty(0, dtype=torch.int64, device=g.device)
        return _range_out(0, squeezed, e, e, e.float(), e.double(), return_dot64)
    words = None if row_mask is None else _pack_row_mask(row_mask, None, g.shape[0])
    qi, rows, score, dot64 = _range_call(q, g, threshold, scale, gallery_norm_bound, None, None, cap, cand_cap, max_pairs,
                                         words)
    return _range_out(Q, squeezed, qi, rows, score, dot64, return_dot64)


def gallery_self_join(gallery: torch.Tensor, threshold: float, scale: float = 1.0,
                      gallery_norm_bound: Optional[float] = None, *, max_pairs: int = _RANGE_MAX_PAIRS,
                      cap: Optional[int] = None, cand_cap: Optional[int] = None, row_mask: Optional[torch.Tensor] = None):
    """All pairs of gallery rows ``i < j`` with fp64 ``dot(row i, row j) >= threshold``, sorted by ``(i, j)``:
    ``(i int64 [P], j int64 [P], scores fp32 [P], dot64 fp64 [P])``.  Same match rule and capacities as ``cosine_range``.
    ``row_mask`` (bool [N]): a pair qualifies only if both of its rows are True."""
    if not gallery.is_cuda:
        raise RuntimeError("gallery must live on the GPU (there is no CPU path)")
    g = gallery if gallery.dtype in _NATIVE_DTYPES else gallery.float()
    g = g.contiguous()
    _check_row_mask(row_mask, g.shape[0], g.device)
    words = None if row_mask is None else _pack_row_mask(row_mask, None, g.shape[0])
    a, b, score, dot64 = _range_call(None, g, threshold, scale, gallery_norm_bound, None, None, cap, cand_cap, max_pairs,
                                     words)
    return a.to(torch.int64), b.to(torch.int64), score, dot64


SWEEP_T_MAX = _lib.HEADER.constants["MMR_SWEEP_T_MAX"]


def _precision_recall_f1(tp, fp, pos):
    """fp64 numpy ``(precision, recall, f1)`` from integer numpy counts (``pos`` = TP + FN, broadcast against ``tp``), by
    the rule of the reference's ``evaluate_thresholds`` (CLIP/lab3.py:39-65), each 0 where its denominator is 0: the one
    place ``ThresholdSweep.metrics`` and ``Confusion.metrics`` take their arithmetic from."""
    import numpy as np

    tp64, fp64 = tp.astype(np.float64), fp.astype(np.float64)
    pos64 = np.broadcast_to(pos.astype(np.float64), tp.shape)     # TP + FN
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = np.where(tp + fp > 0, tp64 / (tp64 + fp64), 0.0)
        recall = np.where(pos64 > 0, tp64 / pos64, 0.0)
        f1 = np.where(precision + recall > 0, 2.0 * precision * recall / (precision + recall), 0.0)
    return precision, recall, f1


class ThresholdSweep:
    """Exact TP / FP counts of Q labelled queries at every point of a threshold grid (``threshold_sweep``).

    ``thresholds`` fp64 [T]; ``tp``, ``fp`` int64 [Q,T]: live rows of the query's class / of any other class whose fp64
    dot with the query is ``>= thresholds[i]``; ``pos``, ``neg`` int64 [Q]: live rows of each kind whose dot is not NaN
    (all on the gallery's device).  ``fn = pos - tp``, ``tn = neg - fp``.  ``counts``: the call's (rechecked, needed)
    candidate pairs.  ``metrics()`` and ``best()`` are O(Q*T) host arithmetic on one copy of the counts.
    """

    def __init__(self, thresholds, ge, total, counts=None, squeezed=False):
        self.thresholds = thresholds
        self._squeezed = squeezed
        sel = (lambda x: x[0]) if squeezed else (lambda x: x)
        self.fp, self.tp = sel(ge[:, 0]), sel(ge[:, 1])
        self.neg, self.pos = sel(total[:, 0]), sel(total[:, 1])
        self.counts = counts
        self._host = None

    @property
    def fn(self):
        return self.pos.unsqueeze(-1) - self.tp

    @property
    def tn(self):
        return self.neg.unsqueeze(-1) - self.fp

    def _counts_host(self):
        if self._host is None:
            both = torch.cat([self.tp.reshape(-1), self.fp.reshape(-1), self.pos.reshape(-1)]).cpu().numpy()
            n = self.tp.numel()
            self._host = (both[:n].reshape(self.tp.shape), both[n:2 * n].reshape(self.tp.shape),
                          both[2 * n:].reshape(self.pos.shape))
        return self._host

    def metrics(self):
        """fp64 numpy ``(precision, recall, f1)``, each shaped like ``tp``, by the rule of the reference's
        ``evaluate_thresholds`` (CLIP/lab3.py:39-65): precision = TP / (TP + FP), recall = TP / (TP + FN) with
        FN = total positives - TP, f1 = 2 P R / (P + R), each 0 where its denominator is 0."""
        tp, fp, pos = self._counts_host()
        return _precision_recall_f1(tp, fp, pos[..., None])

    def best(self):
        """Per query the FIRST grid index of the largest F1 (the reference's loops update on strict ``>``,
        code/search_image.py:95-103, CLIP/lab3.py:56-62): a dict of numpy arrays ``index`` int64, ``threshold``, ``f1``,
        ``precision``, ``recall`` fp64, [Q] each (scalars for a 1-D query)."""
        import numpy as np

        precision, recall, f1 = self.metrics()
        idx = np.argmax(f1, axis=-1)                     # numpy returns the first maximum
        thr = self.thresholds.cpu().numpy()
        take = lambda m: np.take_along_axis(m, np.expand_dims(idx, -1), -1)[..., 0]
        return {"index": idx.astype(np.int64), "threshold": thr[idx], "f1": take(f1), "precision": take(precision),
                "recall": take(recall)}


def _check_sweep_args(q, N, E, labels, targets, thresholds, device):
    """Shapes, dtypes, devices and the grid's order, before any launch.  -> the grid as a fp64 CPU tensor."""
    if q.dim() != 2 or q.shape[1] != E:
        raise ValueError(f"queries {tuple(q.shape)} do not match the gallery's dim {E}")
    for name, t, n in (("labels", labels, N), ("targets", targets, q.shape[0])):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be an integer tensor, got {type(t).__name__}")
        if t.dtype not in (torch.int32, torch.int64) or t.dim() != 1 or t.shape[0] != n:
            raise ValueError(f"{name} must be an int32 / int64 tensor of shape ({n},), got {t.dtype} {tuple(t.shape)}")
    if labels.device != torch.device(device):
        raise ValueError(f"labels live on {labels.device}, the gallery on {device}")
    if not isinstance(thresholds, torch.Tensor):
        import numpy as np

        arr = np.asarray(thresholds)                 # python floats stay fp64 (torch.as_tensor would round them to fp32)
        if arr.dtype.kind not in "fiu":
            raise ValueError(f"thresholds must be real numbers, got {arr.dtype}")
        thresholds = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64))
    thr = thresholds
    if thr.is_complex() or thr.dtype == torch.bool:
        raise ValueError(f"thresholds must be real numbers, got {thr.dtype}")
    thr = thr.detach().to(device="cpu", dtype=torch.float64).contiguous()
    if thr.dim() != 1 or not 1 <= thr.shape[0] <= SWEEP_T_MAX:
        raise ValueError(f"thresholds must be 1-D with 1..{SWEEP_T_MAX} points, got shape {tuple(thr.shape)}")
    if not bool(torch.isfinite(thr).all()):
        raise ValueError("thresholds must be finite")
    if thr.shape[0] > 1 and not bool((thr[1:] > thr[:-1]).all()):
        raise ValueError("thresholds must be strictly ascending")
    return thr


def _i32(t: torch.Tensor, what: str, device) -> torch.Tensor:
    if t.dtype == torch.int64 and t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
        raise ValueError(f"{what} must fit in int32")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _sweep_call(q, g, labels, targets, thr, norm_bound, norm_bound_dev, split, cand_cap, max_pairs, row_mask_words, squeezed,
                qmasks=None):
    """mmr_threshold_sweep under ``_retry.run``, with the candidate capacity ``cand_cap``.  ``qmasks``: (words, stride) of
    per-query masks (``_row_masks_words``) -> mmr_threshold_sweep_qmasked, ``row_mask_words`` being the mask they share."""
    nb = _norm_bound_arg(norm_bound)
    N, E = g.shape
    Q, T = q.shape[0], thr.shape[0]
    dev = g.device
    hi, _, resid = _split_parts(split, g)
    L = _lib.lib()
    cand_cap = int(cand_cap) if cand_cap else _RANGE_CAND_INIT
    ge = torch.empty(Q, 2, T, dtype=torch.int64, device=dev)
    total = torch.empty(Q, 2, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    code = _lib.dtype_code(g.dtype)
    head = (q.data_ptr(), g.data_ptr(), _lib.ptr(hi), code, Q, N, E, labels.data_ptr(), targets.data_ptr(), thr.data_ptr(), T, nb,
            _lib.ptr(norm_bound_dev), _lib.ptr(resid))
    qm = () if qmasks is None else (qmasks[0].data_ptr(), int(qmasks[1]))
    call = L.mmr_threshold_sweep_qmasked if qm else L.mmr_threshold_sweep

    def launch(cand_cap):
        ws = _workspace(L.mmr_sweep_workspace_bytes(N, E, Q, T, cand_cap, code, int(hi is not None)), dev)
        _lib.check(call(*head, *qm, _lib.ptr(row_mask_words), cand_cap, ge.data_ptr(), total.data_ptr(), counts.data_ptr(),
                        ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
        return counts.tolist()

    done, cands = _retry.run(launch, (cand_cap,), max_pairs,
                             lambda c, caps: f"threshold sweep: {c[1]} candidates exceed the capacity {caps[0]} it reported",
                             lambda need: f"threshold sweep needs room for {need[0]} candidate pairs, above max_pairs={max_pairs}: "
                                          f"use a coarser grid or raise max_pairs")
    return ThresholdSweep(thr.to(dev), ge, total, (done, cands), squeezed)


def threshold_sweep(queries: torch.Tensor, gallery: torch.Tensor, labels: torch.Tensor, targets: torch.Tensor, thresholds,
                    gallery_norm_bound: Optional[float] = None, *, row_mask: Optional[torch.Tensor] = None,
                    cand_cap: Optional[int] = None, max_pairs: int = _RANGE_MAX_PAIRS, row_masks=None) -> ThresholdSweep:
    """The reference's threshold sweep -- ``eval_threshold`` / ``find_thresholds`` (code/search_image.py:39-103) and
    ``evaluate_thresholds`` (CLIP/lab3.py:39-65) -- in one pass over the gallery, exact, without the [Q,N] scores.

    For query q with class ``targets[q]`` and every grid point t: ``tp[q,i]`` = rows with ``labels == targets[q]`` whose
    fp64 dot with the query is ``>= thresholds[i]``, ``fp[q,i]`` the same over the other rows; every count equals a
    brute-force fp64 evaluation in oracle/search_ref.c's order.  ``thresholds``: 1-D, finite, strictly ascending, at
    most 1024 points, on the UNSCALED dot (the reference's ``100*cos >= t`` is ``t/100``).  ``labels`` int [N] on the
    gallery's device, ``targets`` int [Q].  ``row_mask`` (bool [N]): only rows where it is True are counted.
    ``cand_cap``: the first call's candidate capacity; a call that needs more is repeated once at the reported size,
    unless that exceeds ``max_pairs`` (MemoryError).  Cost and the fp32 case: include/mmr.h.

    ``row_masks``: a mask per query (bool [Q, N] or ``DecisionMasks``, as in ``cosine_topk_deep``): query q counts only the
    rows of ``row_masks[q]`` (AND ``row_mask``), and ``total[q]`` is that query's own -- the reference's loop over classes,
    each with its sample images taken out of its own gallery (``leave_out_masks``), as one call and one gallery pass.
    """
    q2, squeezed = _as_2d(queries)
    q, g = _prep_pair(q2, gallery)
    tg = torch.as_tensor(targets).reshape(-1) if squeezed else targets
    thr = _check_sweep_args(q, g.shape[0], g.shape[1], labels, tg, thresholds, g.device)
    _check_row_mask(row_mask, g.shape[0], g.device)
    _check_row_masks(row_masks, q.shape[0], g.shape[0], g.shape[1], g.device)
    words = None if row_mask is None else _pack_row_mask(row_mask, None, g.shape[0])
    qmasks = None if row_masks is None else _row_masks_words(row_masks, g.shape[0])
    return _sweep_call(q, g, _i32(labels, "labels", g.device), _i32(tg, "targets", g.device), thr, gallery_norm_bound, None,
                       None, cand_cap, max_pairs, words, squeezed, qmasks)


class Confusion:
    """``tp``, ``fp``, ``fn``, ``tn`` int64 [Q] of Q decision masks against labels (``DecisionMasks.confusion``), on the
    masks' device.  ``pos = tp + fn`` and ``neg = fp + tn`` are the live rows of each kind."""

    def __init__(self, tp, fp, pos, neg):
        self.tp, self.fp, self.pos, self.neg = tp, fp, pos, neg
        self.fn, self.tn = pos - tp, neg - fp

    def metrics(self):
        """fp64 numpy ``(precision, recall, f1)``, [Q] each, by the rule of ``ThresholdSweep.metrics``."""
        both = torch.stack([self.tp, self.fp, self.pos]).cpu().numpy()
        return _precision_recall_f1(both[0], both[1], both[2])


class DecisionMasks:
    """Q exact row masks over one gallery (``cosine_decide`` / ``GalleryIndex.decide``): bit ``r & 31`` of
    ``words[q, r >> 5]`` is set iff row r is live and its fp64 dot with query q is ``>=`` that query's threshold.

    ``words`` int32 [Q, ceil(N/32)] on the gallery's device, in the row-mask word format of include/mmr.h (bits at or
    past N are 0); ``num_rows`` = N; ``counts``: the call's (rechecked, needed) candidate pairs, None for a combination.
    ``a | b``, ``a & b`` and ``a.andnot(b)`` combine two results over the same rows word by word (one launch); the
    reference's EN-or-CN rule (code/merge_dataset.py:440) is ``en | cn``.
    """

    def __init__(self, words: torch.Tensor, num_rows: int, counts=None):
        self.words, self.num_rows, self.counts = words, int(num_rows), counts

    @classmethod
    def from_bool(cls, keep: torch.Tensor) -> "DecisionMasks":
        """Masks from a bool tensor [Q, N] (True = the row is kept for that query): one packing launch on the GPU."""
        if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or keep.dim() != 2:
            raise ValueError("from_bool takes a bool tensor [Q, N]")
        return cls(_pack_row_masks(keep, keep.shape[1]), keep.shape[1])

    def _combine(self, other, op: int):
        if not isinstance(other, DecisionMasks):
            raise ValueError(f"expected DecisionMasks, got {type(other).__name__}")
        if other.num_rows != self.num_rows or tuple(other.words.shape) != tuple(self.words.shape):
            raise ValueError(f"decision masks of {tuple(self.words.shape)} words over {self.num_rows} rows cannot be combined "
                             f"with masks of {tuple(other.words.shape)} words over {other.num_rows} rows")
        if other.words.device != self.words.device:
            raise ValueError(f"decision masks live on {self.words.device} and {other.words.device}")
        a, b = self.words.contiguous(), other.words.contiguous()
        res = torch.empty_like(a)
        _lib.check(_lib.lib().mmr_row_mask_combine(a.data_ptr(), b.data_ptr(), op, a.numel(), res.data_ptr(),
                                                   _lib.stream_ptr(a.device)))
        return DecisionMasks(res, self.num_rows)

    def __or__(self, other):
        return self._combine(other, 0)

    def __and__(self, other):
        return self._combine(other, 1)

    def andnot(self, other):
        """``self & ~other``: the rows this result passes and ``other`` does not."""
        return self._combine(other, 2)

    def to_bool(self) -> torch.Tensor:
        """bool [Q, N]."""
        shifts = torch.arange(32, dtype=torch.int32, device=self.words.device)
        bits = (self.words.unsqueeze(-1) >> shifts) & 1
        return bits.reshape(self.words.shape[0], -1)[:, :self.num_rows].bool()

    def row_mask(self, i: int) -> torch.Tensor:
        """bool [N]: query i's rows, ready for ``row_mask=`` of ``search`` / ``search_deep`` / ``range_search`` /
        ``threshold_sweep``; ``index.delete_rows(masks.row_mask(i).nonzero())`` drops them."""
        shifts = torch.arange(32, dtype=torch.int32, device=self.words.device)
        return (((self.words[i].unsqueeze(-1) >> shifts) & 1).reshape(-1)[:self.num_rows]).bool()

    def _counts_call(self, labels, targets, row_mask):
        Q, N = self.words.shape[0], self.num_rows
        dev = self.words.device
        _check_row_mask(row_mask, N, dev)
        live = None if row_mask is None else _pack_row_mask(row_mask, None, N)
        out = torch.empty(Q, 4, dtype=torch.int64, device=dev)
        w = self.words.contiguous()
        _lib.check(_lib.lib().mmr_decision_counts(w.data_ptr(), Q, N, _lib.ptr(labels), _lib.ptr(targets), _lib.ptr(live),
                                                  out.data_ptr(), _lib.stream_ptr(dev)))
        return out

    def num_set(self) -> torch.Tensor:
        """int64 [Q]: the rows each query passes."""
        return self._counts_call(None, None, None)[:, 0]

    def confusion(self, labels: torch.Tensor, targets: torch.Tensor, row_mask: Optional[torch.Tensor] = None) -> Confusion:
        """TP / FP / FN / TN of each query's mask, taking the rows with ``labels == targets[q]`` for its positives: the
        ``calc_combined_metrics`` of the reference (CLIP/union_dataset.py:181-231) for a union mask.  ``labels`` int [N]
        on the masks' device, ``targets`` int [Q].  Positives and negatives are counted over every row below N, or over
        the rows of ``row_mask`` (bool [N]) -- pass ``index.live_mask`` after deletions.  Rows whose dot is NaN count
        as negatives or misses here (``threshold_sweep`` leaves them out of its totals)."""
        Q, N = self.words.shape[0], self.num_rows
        dev = self.words.device
        for name, t, n in (("labels", labels, N), ("targets", targets, Q)):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be an integer tensor, got {type(t).__name__}")
            if t.dtype not in (torch.int32, torch.int64) or t.dim() != 1 or t.shape[0] != n:
                raise ValueError(f"{name} must be an int32 / int64 tensor of shape ({n},), got {t.dtype} {tuple(t.shape)}")
        if labels.device != dev:
            raise ValueError(f"labels live on {labels.device}, the masks on {dev}")
        out = self._counts_call(_i32(labels, "labels", dev), _i32(targets, "targets", dev), row_mask)
        return Confusion(out[:, 0], out[:, 1], out[:, 2], out[:, 3])


def _check_decide_args(q, E: int, thresholds) -> torch.Tensor:
    """Query shape and the thresholds of a decide call, before any launch.  -> the thresholds as a fp64 CPU tensor [Q]
    (a python float or a 0-d value is given to every query)."""
    import numpy as np

    if q.dim() != 2 or q.shape[1] != E:
        raise ValueError(f"queries {tuple(q.shape)} do not match the gallery's dim {E}")
    Q = q.shape[0]
    if Q < 1:
        raise ValueError("decide needs at least one query")
    if not isinstance(thresholds, torch.Tensor):
        arr = np.asarray(thresholds)                 # python floats stay fp64 (torch.as_tensor would round them to fp32)
        if arr.dtype.kind not in "fiu":
            raise ValueError(f"thresholds must be real numbers, got {arr.dtype}")
        thresholds = torch.from_numpy(np.array(arr, dtype=np.float64))
    thr = thresholds
    if thr.is_complex() or thr.dtype == torch.bool:
        raise ValueError(f"thresholds must be real numbers, got {thr.dtype}")
    thr = thr.detach().to(device="cpu", dtype=torch.float64)
    if thr.dim() == 0:
        thr = thr.expand(Q)
    if thr.dim() != 1 or thr.shape[0] != Q:
        raise ValueError(f"thresholds must be one number or one per query ({Q}), got shape {tuple(thr.shape)}")
    if not bool(torch.isfinite(thr).all()):
        raise ValueError("thresholds must be finite")
    return thr.contiguous()


def _decide_call(q, g, thr_dev, norm_bound, norm_bound_dev, split, cand_cap, max_pairs, row_mask_words, workspace=None):
    """mmr_cosine_decide under ``_retry.run``, with the candidate capacity ``cand_cap``.  -> (DecisionMasks, workspace)."""
    nb = _norm_bound_arg(norm_bound)
    N, E = g.shape
    Q = q.shape[0]
    dev = g.device
    hi, _, resid = _split_parts(split, g)
    code = _lib.dtype_code(g.dtype)
    L = _lib.lib()
    cand_cap = int(cand_cap) if cand_cap else _RANGE_CAND_INIT
    if cand_cap < 1:
        raise ValueError("cand_cap must be >= 1")
    words = torch.empty(Q, (N + 31) // 32, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)

    def launch(cand_cap):
        nonlocal workspace
        workspace = _workspace(L.mmr_decide_workspace_bytes(N, E, Q, cand_cap, code, int(hi is not None)), dev, workspace)
        _lib.check(L.mmr_cosine_decide(q.data_ptr(), g.data_ptr(), _lib.ptr(hi), code, Q, N, E, thr_dev.data_ptr(), nb,
                                       _lib.ptr(norm_bound_dev), _lib.ptr(resid), _lib.ptr(row_mask_words), cand_cap, words.data_ptr(),
                                       counts.data_ptr(), workspace.data_ptr(), workspace.numel(), _lib.stream_ptr(dev)))
        return counts.tolist()

    done, cands = _retry.run(launch, (cand_cap,), max_pairs,
                             lambda c, caps: f"decide: {c[1]} candidates exceed the capacity {caps[0]} it reported",
                             lambda need: f"decide needs room for {need[0]} candidate pairs, above max_pairs={max_pairs}: "
                                          f"raise max_pairs")
    return DecisionMasks(words, N, (done, cands)), workspace


def cosine_decide(queries: torch.Tensor, gallery: torch.Tensor, thresholds, *, row_mask: Optional[torch.Tensor] = None,
                  norm_bound: Optional[float] = None, cand_cap: Optional[int] = None,
                  max_pairs: int = _RANGE_MAX_PAIRS) -> DecisionMasks:
    """The reference's per-class decision -- ``similarity >= threshold`` with a threshold per class vector
    (code/merge_dataset.py:259-311, the production thresholds of code/union_clip_llava2.py:153-162) -- for Q queries in
    one pass over the gallery, exact, as Q packed row masks: no [Q,N] scores, no pair list, no sort.

    ``thresholds``: one number for every query, or one per query (sequence / tensor of length Q); fp64, finite
    (ValueError otherwise), on the UNSCALED dot (the reference's ``100*cos >= t`` is ``t/100``).  Row r passes query q iff
    its fp64 dot in oracle/search_ref.c's order is ``>= thresholds[q]``: bit for bit a brute-force fp64 evaluation; a tie
    passes, a NaN dot does not.  ``row_mask`` (bool [N]): rows where it is False never pass.  ``norm_bound`` as
    ``cosine_topk``'s ``gallery_norm_bound``.  A 1-D query gives a 1-row result.  ``cand_cap``: the first call's candidate
    capacity; a call that needs more is repeated once at the reported size, unless that exceeds ``max_pairs``
    (MemoryError).  Cost: include/mmr.h.
    """
    q2, _ = _as_2d(queries)
    q, g = _prep_pair(q2, gallery)
    thr = _check_decide_args(q, g.shape[1], thresholds)
    _check_row_mask(row_mask, g.shape[0], g.device)
    words = None if row_mask is None else _pack_row_mask(row_mask, None, g.shape[0])
    return _decide_call(q, g, thr.to(g.device), norm_bound, None, None, cand_cap, max_pairs, words)[0]


_ASSIGN_AMB_INIT = 1 << 16          # first ambiguous-row capacity of an assign call (4 B each)
_ASSIGN_MAX_AMBIGUOUS = 1 << 28     # default ceiling on the ambiguous-row list a call may allocate


def _check_assign_args(g, centroids, bias):
    """Shapes and dtypes of an assign call, before any launch.  -> (centroids [K, E] in the gallery's dtype, bias fp64 [K] on
    the gallery's device or None)."""
    if g.dim() != 2:
        raise ValueError(f"gallery must be [N, E], got shape {tuple(g.shape)}")
    if g.dtype == torch.float32:
        raise ValueError("cosine_assign: fp32 galleries are not supported (bf16 or fp16 only); its 16-bit scan would leave "
                         "18-42 % of the rows to the exact recheck -- cast the gallery, or wait for the three-product form")
    if not isinstance(centroids, torch.Tensor) or centroids.dim() != 2 or centroids.shape[1] != g.shape[1]:
        raise ValueError(f"centroids must be a [K, {g.shape[1]}] tensor")
    if centroids.shape[0] < 1:
        raise ValueError("assign needs at least one centroid")
    c = centroids.to(device=g.device, dtype=g.dtype).contiguous()
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or tuple(bias.shape) != (c.shape[0],) or bias.is_complex() or bias.dtype == torch.bool:
            raise ValueError(f"bias must be a real tensor [{c.shape[0]}]")
        bias = bias.detach().to(device=g.device, dtype=torch.float64).contiguous()
    return c, bias


def _assign_call(g, c, bias, norm_bound, norm_bound_dev, row_mask_words, return_score, amb_cap, max_ambiguous, workspace=None):
    """mmr_cosine_assign under ``_retry.run``, with the capacity ``amb_cap`` of the ambiguous-row list.
    -> (labels int32 [N], best64 fp64 [N] or None, (rechecked, ambiguous), workspace)."""
    nb = _norm_bound_arg(norm_bound)
    N, E = g.shape
    K = c.shape[0]
    dev = g.device
    L = _lib.lib()
    amb_cap = int(amb_cap) if amb_cap else min(_ASSIGN_AMB_INIT, max(int(max_ambiguous), 1))
    if amb_cap < 1:
        raise ValueError("amb_cap must be >= 1")
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    best64 = torch.empty(N, dtype=torch.float64, device=dev) if return_score else None
    counts = torch.zeros(2, dtype=torch.int64, device=dev)

    def launch(amb_cap):
        nonlocal workspace
        workspace = _workspace(L.mmr_assign_workspace_bytes(N, E, K, amb_cap, _lib.dtype_code(g.dtype)), dev, workspace)
        _lib.check(L.mmr_cosine_assign(g.data_ptr(), c.data_ptr(), _lib.dtype_code(g.dtype), N, K, E, _lib.ptr(bias), nb,
                                       _lib.ptr(norm_bound_dev), _lib.ptr(row_mask_words), amb_cap, labels.data_ptr(),
                                       _lib.ptr(best64), counts.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                       _lib.stream_ptr(dev)))
        return counts.tolist()

    done, amb = _retry.run(launch, (amb_cap,), max_ambiguous,
                           lambda c, caps: f"assign: {c[1]} ambiguous rows exceed the capacity {caps[0]} it reported",
                           lambda need: f"assign needs room for {need[0]} ambiguous rows, above max_ambiguous={max_ambiguous}: "
                                        f"raise max_ambiguous")
    return labels, best64, (done, amb), workspace


def cosine_assign(gallery: torch.Tensor, centroids: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
                  row_mask: Optional[torch.Tensor] = None, return_score: bool = False, norm_bound: Optional[float] = None,
                  amb_cap: Optional[int] = None, max_ambiguous: int = _ASSIGN_MAX_AMBIGUOUS, return_counts: bool = False):
    """The arg-max over K centroids for every gallery row -- the assignment step of the reference's ``KMeans``
    (``get_cluster_features``, code/search_image.py:185-292) -- exact, in one device call, with no [N, K] scores.

    ``labels[r]`` (int32 [N]) is the centroid c with the largest ``dot64(gallery[r], centroids[c]) + bias[c]`` in fp64
    (oracle/search_ref.c's fixed-order dot; ``bias`` fp64 [K], None: no term).  Ties go to the lowest c, a NaN score never
    wins, a row whose scores are all NaN and a row where ``row_mask`` (bool [N]) is False get -1.
    ``bias = -0.5 * |c|^2`` gives the Euclidean nearest centroid, no bias the cosine one.  ``return_score``: also the
    exact fp64 score of each row's pair (NaN where the label is -1).  The gallery is bf16 or fp16 and the centroids are
    converted to its dtype; an fp32 gallery raises ValueError.  ``amb_cap``: the first call's capacity for ambiguous rows
    (those the approximate scan cannot decide); a call that needs more is repeated once at the reported size, unless
    that exceeds ``max_ambiguous`` (MemoryError).  ``return_counts``: append ``(rechecked, ambiguous)``.  Cost: include/mmr.h.
    """
    if not gallery.is_cuda:
        raise RuntimeError("gallery must live on the GPU (there is no CPU path)")
    if gallery.dtype not in _NATIVE_DTYPES:
        raise ValueError(f"cosine_assign: gallery dtype {gallery.dtype} (bf16 or fp16 only)")
    g = gallery.contiguous()
    c, b = _check_assign_args(g, centroids, bias)
    _check_row_mask(row_mask, g.shape[0], g.device)
    words = None if row_mask is None else _pack_row_mask(row_mask, None, g.shape[0])
    labels, best64, counts, _ = _assign_call(g, c, b, norm_bound, None, words, return_score, amb_cap, max_ambiguous)
    out = (labels,) + ((best64,) if return_score else ()) + ((counts,) if return_counts else ())
    return out[0] if len(out) == 1 else out


def merge_topk(idx_parts: torch.Tensor, dot_parts: torch.Tensor, scale: float = 1.0):
    """Merge per-shard lists [parts,Q,k] (global int64 ids, fp64 dots) -> (values, indices, dot64)."""
    idx_parts = idx_parts.contiguous()
    dot_parts = dot_parts.contiguous()
    parts, Q, k = idx_parts.shape
    dev = idx_parts.device
    idx = torch.empty(Q, k, dtype=torch.int64, device=dev)
    score = torch.empty(Q, k, dtype=torch.float32, device=dev)
    dot64 = torch.empty(Q, k, dtype=torch.float64, device=dev)
    L = _lib.lib()
    _lib.check(L.mmr_topk_merge(idx_parts.data_ptr(), dot_parts.data_ptr(), parts, Q, k, float(scale),
                                idx.data_ptr(), score.data_ptr(), dot64.data_ptr(), _lib.stream_ptr(dev)))
    return score, idx, dot64


def merge_topk_packed(gathered: torch.Tensor, scale: float = 1.0):
    """Merge the gathered per-shard messages [parts,Q,k,2] int64 (mmr_topk_pack layout) -> (values, indices, dot64)."""
    gathered = gathered.contiguous()
    parts, Q, k, _ = gathered.shape
    dev = gathered.device
    idx = torch.empty(Q, k, dtype=torch.int64, device=dev)
    score = torch.empty(Q, k, dtype=torch.float32, device=dev)
    dot64 = torch.empty(Q, k, dtype=torch.float64, device=dev)
    L = _lib.lib()
    _lib.check(L.mmr_topk_merge_packed(gathered.data_ptr(), parts, Q, k, float(scale), idx.data_ptr(), score.data_ptr(),
                                       dot64.data_ptr(), _lib.stream_ptr(dev)))
    return score, idx, dot64


class GalleryIndex:
    """A device-resident embedding matrix [N,E] with a reusable search workspace.

    Stands where the reference keeps ``test_features`` (code/search_image.py:167-182) and
    scores it against reference vectors; rows are whatever ``encode_image`` produced -- normalised or
    not: the largest row norm is measured once here (device scalar, no host sync) and sizes the
    certificate's margin; a caller-supplied ``norm_bound`` can only widen it.  A contiguous fp32, bf16 or fp16 gallery is
    kept as it is (no copy; fp16 and bf16 need no split either) and queries are converted to its dtype.

    The exactness certificate rests on that measured bound, so ``self.gallery`` is treated as FROZEN after
    construction: change rows through ``update_rows`` (writes them and re-measures) or call
    ``refresh_norm_bound()`` after writing into ``self.gallery`` yourself -- an in-place update that raises a
    row norm without a re-measure would understate the bound and could let the certificate pass wrongly.

    Rows can be deleted and restored without touching the gallery (``delete_rows`` / ``restore_rows`` / ``dedup``):
    the live set is one device word buffer, updated in place, that every search passes as its row mask from the first
    deletion on.  A search captured in a hipGraph after the first deletion therefore sees later deletions, as it sees a
    ``refresh_norm_bound``; a graph captured before the first deletion keeps the unmasked path and does not.  Every search
    method also takes ``row_mask`` (bool [N] on the gallery's device) for one call; the effective mask is
    ``live & row_mask``.  Results equal a fresh index over the live rows with ids mapped back.  The norm bound stays
    measured over all rows (still sound for any subset), so deleting never forces a re-measure.
    """

    def __init__(self, gallery: torch.Tensor, norm_bound: Optional[float] = None, presplit: Optional[bool] = None):
        """``presplit`` (fp32 galleries only; default: on from 4096 rows): keep the gallery's hi / lo bf16 split next to it
        (as many bytes again as the gallery): searches then scan the bf16 ``hi`` half alone first and fall back to the
        three-product scan over both halves only for queries that pass cannot certify -- identical results, about half the
        time of the per-call path on galleries whose top scores are not crowded."""
        if not gallery.is_cuda:
            raise RuntimeError("GalleryIndex needs a CUDA/HIP tensor")
        if gallery.dtype not in _NATIVE_DTYPES:
            gallery = gallery.float()
        self.gallery = gallery.contiguous()
        self.norm_bound = None if norm_bound is None else float(norm_bound)
        self.norm_bound_dev = gallery_norm_bound(self.gallery)
        self._ws_lanes = {}        # lane -> search workspace: searches on different lanes may overlap on different streams
        self._split = None
        if presplit is None:
            presplit = self.gallery.shape[0] >= 4096
        self._presplit = bool(presplit) and self.gallery.dtype == torch.float32 and self.gallery.shape[0] > 0
        self._refresh_split()
        self._live = None          # bool [N] live rows: created by the first delete_rows
        self._live_words = None    # their packed mask words, updated in place; NULL mask (today's path) until then
        self._mask_lanes = {}      # lane -> packed (live & row_mask) words of a call with a row_mask
        self._qsplit = None        # fp32 index without a split: the one the row_masks= calls scan, built by the first of them

    def _refresh_split(self) -> None:
        self._qsplit = None
        if not self._presplit:
            return
        g = self.gallery
        if self._split is None:
            self._split = (torch.empty(g.shape, dtype=torch.bfloat16, device=g.device),
                           torch.empty(g.shape, dtype=torch.bfloat16, device=g.device),
                           torch.zeros(1, dtype=torch.float32, device=g.device))       # max_row |g - hi|, same scalar for life
        L = _lib.lib()
        _lib.check(L.mmr_gallery_split_bf16(g.data_ptr(), g.shape[0], g.shape[1], self._split[0].data_ptr(),
                                            self._split[1].data_ptr(), self._split[2].data_ptr(), _lib.stream_ptr(g.device)))

    @property
    def num_rows(self) -> int:
        return self.gallery.shape[0]

    def refresh_norm_bound(self) -> None:
        """Re-measure the largest row norm into the SAME device scalar (one HBM-bound pass, no host sync), so searches
        already captured in a hipGraph see the new bound too."""
        g = self.gallery
        L = _lib.lib()
        _lib.check(L.mmr_gallery_norm_bound(g.data_ptr(), _lib.dtype_code(g.dtype), g.shape[0], g.shape[1],
                                            self.norm_bound_dev.data_ptr(), _lib.stream_ptr(g.device)))
        self._refresh_split()

    def update_rows(self, rows: torch.Tensor, values: torch.Tensor) -> None:
        """``gallery[rows] = values`` followed by a re-measure of the norm bound (keeps the certificate sound)."""
        self.gallery[rows.to(self.gallery.device)] = values.to(device=self.gallery.device, dtype=self.gallery.dtype)
        self.refresh_norm_bound()

    # ------------------------------------------------------------------ live rows
    def _rows_arg(self, rows) -> torch.Tensor:
        r = torch.as_tensor(rows).reshape(-1)
        if r.dtype == torch.bool or r.is_floating_point() or r.is_complex():
            raise ValueError(f"rows must be integer row ids, got {r.dtype}")
        r = r.to(torch.int64)
        n = self.num_rows
        if r.numel() and (int(r.min()) < 0 or int(r.max()) >= n):
            raise ValueError(f"row ids must lie in [0, {n})")
        return r.to(self.gallery.device)

    def _set_live(self, rows, value: bool) -> None:
        r = self._rows_arg(rows)
        if self._live is None:
            n = self.num_rows
            self._live = torch.ones(n, dtype=torch.bool, device=self.gallery.device)
            self._live_words = torch.empty(max((n + 31) // 32, 1), dtype=torch.int32, device=self.gallery.device)
        self._live[r] = value
        _pack_row_mask(self._live, None, self.num_rows, self._live_words)     # in place: captured searches see it

    def delete_rows(self, rows) -> None:
        """Drop ``rows`` (integer ids) from every later search of this index.  The gallery is not touched."""
        self._set_live(rows, False)

    def restore_rows(self, rows) -> None:
        """Undo ``delete_rows`` for ``rows``."""
        self._set_live(rows, True)

    @property
    def live_mask(self) -> torch.Tensor:
        """bool [N] on the gallery's device: the rows searches can return (a copy)."""
        if self._live is None:
            return torch.ones(self.num_rows, dtype=torch.bool, device=self.gallery.device)
        return self._live.clone()

    def trimmed_centers(self, labels, K: int, **kw):
        """``cluster.trimmed_centers`` of this gallery's live rows: the outlier-trimmed centre of every class
        (``percentile=``, ``metric=``, ``centers=`` as there).  Deleted rows take no part; ``row_mask=`` narrows further."""
        from . import cluster as _cluster

        row_mask = kw.pop("row_mask", None)
        _check_row_mask(row_mask, self.num_rows, self.gallery.device)
        if self._live is not None:
            row_mask = self.live_mask if row_mask is None else self.live_mask & row_mask
        return _cluster.trimmed_centers(self.gallery, labels, K, row_mask=row_mask, **kw)

    def _mask_words(self, row_mask, lane):
        """The packed effective mask of one call: live & row_mask.  None (the unmasked path) while no row was ever deleted
        and no row_mask is given."""
        _check_row_mask(row_mask, self.num_rows, self.gallery.device)
        if row_mask is None:
            return self._live_words
        buf = self._mask_lanes.get(lane)
        if buf is None:
            buf = torch.empty(max((self.num_rows + 31) // 32, 1), dtype=torch.int32, device=self.gallery.device)
            self._mask_lanes[lane] = buf
        return _pack_row_mask(row_mask, self._live_words, self.num_rows, buf)

    def dedup(self, threshold: float, order=None, scale: float = 1.0, **caps):
        """The data-governance pass over the live rows: the self-join at ``threshold``, the reference's greedy keep/drop
        (``dedup.keep_first`` in visit ``order``, default row order), then ``delete_rows`` of the dropped rows.
        Returns ``(dropped, kept_partner)`` int64 tensors: each dropped row and the kept row it duplicates.
        ``caps``: ``max_pairs`` / ``cap`` / ``cand_cap`` as in ``cosine_range``."""
        from . import dedup as _dedup

        i, j, _, _ = self.near_duplicates(threshold, scale, **caps)
        keep, dup = _dedup.keep_first(self.num_rows, i, j, order)
        dropped = torch.from_numpy((~keep).nonzero()[0].astype("int64"))
        partner = torch.from_numpy(dup[dropped.numpy()])
        if dropped.numel():
            self.delete_rows(dropped)
        dev = self.gallery.device
        return dropped.to(dev), partner.to(dev)

    # ------------------------------------------------------------------ searches
    def search(self, queries: torch.Tensor, k: int = 10, scale: float = 1.0, return_dot64: bool = False,
               return_status: bool = False, lane: int = 0, row_mask: Optional[torch.Tensor] = None, row_masks=None):
        """``lane``: which of the index's workspaces the call uses; searches on different lanes may be in flight at once on
        different HIP streams (they only read the gallery), searches on one lane must be stream-ordered.
        ``row_mask``: bool [N], search only the live rows where it is True (the class docstring).
        ``k`` goes up to 64; ``search_deep`` answers k up to 4096.
        ``row_masks``: one mask per query (``search_deep``); the deep call then answers any k with the same results, and
        ``return_status=True`` with it is a ValueError."""
        q2, squeezed = _as_2d(queries)
        if row_masks is not None:
            if q2.shape[1] == self.gallery.shape[1]:
                _check_row_masks(row_masks, q2.shape[0], self.num_rows, self.gallery.shape[1], self.gallery.device, return_status)
            return self.search_deep(queries, k, scale, return_dot64, row_mask, lane=lane, row_masks=row_masks)
        q = q2.to(device=self.gallery.device, dtype=self.gallery.dtype).contiguous()
        words = self._mask_words(row_mask, lane)
        idx, score, dot64, status, self._ws_lanes[lane] = _local_topk(q, self.gallery, int(k), scale, self.norm_bound,
                                                                      return_dot64, return_status, self._ws_lanes.get(lane),
                                                                      self.norm_bound_dev, self._split, words)
        idx = idx.to(torch.int64)
        if squeezed:
            idx, score = idx[0], score[0]
            dot64 = dot64[0] if dot64 is not None else None
        out = (score, idx)
        if return_dot64:
            out = out + (dot64,)
        if return_status:
            out = out + (status,)
        return out

    def search_deep(self, queries: torch.Tensor, k: int, scale: float = 1.0, return_dot64: bool = False,
                    row_mask: Optional[torch.Tensor] = None, *, max_pairs: int = _RANGE_MAX_PAIRS,
                    tile_cap: Optional[int] = None, surv_cap: Optional[int] = None, lane: int = 0, row_masks=None):
        """``cosine_topk_deep`` over this index (k up to 4096): reuses the measured norm bound, for a pre-split fp32 gallery
        its ``hi`` half and residual bound, the live mask (AND ``row_mask``) and a workspace per ``lane``.  Identical
        results; ``(values, indices int64[, dot64])``.  ``self.deep_counts``: the (listed tiles, surviving rows) of the
        last call, the capacities a repeat of it needs.
        ``row_masks``: one mask per query -- bool [Q, N] or ``DecisionMasks`` (``index.decide(...)``: rank with these
        queries among the rows another tower accepted; ``leave_out_masks``) -- AND-ed with the live rows and ``row_mask``.
        An fp32 index without a split builds and keeps one for these calls."""
        q2, squeezed = _as_2d(queries)
        _check_deep_args(q2, self.gallery, k, row_mask, row_masks)
        q = q2.to(device=self.gallery.device, dtype=self.gallery.dtype).contiguous()
        words = self._mask_words(row_mask, ("deep", lane))
        qmasks, split = None, self._split
        if row_masks is not None:
            qmasks = _row_masks_words(row_masks, self.num_rows)
            if self.gallery.dtype == torch.float32 and split is None and self.num_rows > 0:
                if self._qsplit is None:
                    self._qsplit = _split_fp32(self.gallery)
                split = self._qsplit
        idx, score, dot64, self._ws_lanes[("deep", lane)], self.deep_counts = _deep_call(
            q, self.gallery, int(k), scale, self.norm_bound, self.norm_bound_dev, split, words, max_pairs, tile_cap,
            surv_cap, return_dot64, self._ws_lanes.get(("deep", lane)), qmasks=qmasks)
        return _deep_out(squeezed, idx, score, dot64, return_dot64)

    def search_packed(self, queries2d: torch.Tensor, k: int, scale: float, row_offset: int, lane: int = 0,
                      row_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """This shard's all-gather message for [Q,E] queries: [Q,k,2] int64 = (global row id or -1, fp64 dot bits),
        written by one kernel straight from the search outputs (mmr_topk_pack)."""
        q = queries2d.to(device=self.gallery.device, dtype=self.gallery.dtype).contiguous()
        words = self._mask_words(row_mask, lane)
        idx, _, dot64, _, self._ws_lanes[lane] = _local_topk(q, self.gallery, int(k), scale, self.norm_bound, True, False,
                                                             self._ws_lanes.get(lane), self.norm_bound_dev, self._split,
                                                             words)
        packed = torch.empty(q.shape[0], int(k), 2, dtype=torch.int64, device=q.device)
        L = _lib.lib()
        _lib.check(L.mmr_topk_pack(idx.data_ptr(), dot64.data_ptr(), q.shape[0], int(k), int(row_offset), packed.data_ptr(),
                                   _lib.stream_ptr(q.device)))
        return packed

    def range_search(self, queries: torch.Tensor, threshold: float, scale: float = 1.0, return_dot64: bool = False, *,
                     max_pairs: int = _RANGE_MAX_PAIRS, cap: Optional[int] = None, cand_cap: Optional[int] = None,
                     row_mask: Optional[torch.Tensor] = None):
        """``cosine_range`` over this index: reuses the measured norm bound and, for a pre-split fp32 gallery, its ``hi`` half
        and residual bound.  Identical results.  Deleted rows and rows where ``row_mask`` is False never match."""
        q2, squeezed = _as_2d(queries)
        q = q2.to(device=self.gallery.device, dtype=self.gallery.dtype).contiguous()
        if q.shape[1] != self.gallery.shape[1]:
            raise ValueError(f"query dim {q.shape[1]} != gallery dim {self.gallery.shape[1]}")
        words = self._mask_words(row_mask, "range")
        Q = q.shape[0]
        if Q == 0:
            e = torch.empty(0, dtype=torch.int64, device=q.device)
            return _range_out(0, squeezed, e, e, e.float(), e.double(), return_dot64)
        qi, rows, score, dot64 = _range_call(q, self.gallery, threshold, scale, self.norm_bound, self.norm_bound_dev,
                                             self._split, cap, cand_cap, max_pairs, words)
        return _range_out(Q, squeezed, qi, rows, score, dot64, return_dot64)

    def threshold_sweep(self, queries: torch.Tensor, labels: torch.Tensor, targets: torch.Tensor, thresholds, *,
                        row_mask: Optional[torch.Tensor] = None, cand_cap: Optional[int] = None,
                        max_pairs: int = _RANGE_MAX_PAIRS, row_masks=None) -> ThresholdSweep:
        """``threshold_sweep`` over this index: reuses the measured norm bound and, for a pre-split fp32 gallery, its ``hi``
        half and residual bound.  Identical results.  Deleted rows and rows where ``row_mask`` is False are counted nowhere;
        ``row_masks`` gives every query a mask of its own on top of both."""
        q2, squeezed = _as_2d(queries)
        q = q2.to(device=self.gallery.device, dtype=self.gallery.dtype).contiguous()
        N, E = self.gallery.shape
        tg = torch.as_tensor(targets).reshape(-1) if squeezed else targets
        thr = _check_sweep_args(q, N, E, labels, tg, thresholds, self.gallery.device)
        _check_row_masks(row_masks, q.shape[0], N, E, self.gallery.device)
        words = self._mask_words(row_mask, "range")
        qmasks = None if row_masks is None else _row_masks_words(row_masks, N)
        return _sweep_call(q, self.gallery, _i32(labels, "labels", q.device), _i32(tg, "targets", q.device), thr,
                           self.norm_bound, self.norm_bound_dev, self._split, cand_cap, max_pairs, words, squeezed, qmasks)

    def decide(self, queries: torch.Tensor, thresholds, *, row_mask: Optional[torch.Tensor] = None,
               cand_cap: Optional[int] = None, max_pairs: int = _RANGE_MAX_PAIRS, lane: int = 0) -> DecisionMasks:
        """``cosine_decide`` over this index: reuses the measured norm bound, for a pre-split fp32 gallery its ``hi`` half and
        residual bound, the live mask (AND ``row_mask``) and a workspace per ``lane``.  Identical results.  Deleted rows
        and rows where ``row_mask`` is False never pass."""
        q2, _ = _as_2d(queries)
        q = q2.to(device=self.gallery.device, dtype=self.gallery.dtype).contiguous()
        thr = _check_decide_args(q, self.gallery.shape[1], thresholds)
        words = self._mask_words(row_mask, ("decide", lane))
        res, self._ws_lanes[("decide", lane)] = _decide_call(q, self.gallery, thr.to(q.device), self.norm_bound,
                                                             self.norm_bound_dev, self._split, cand_cap, max_pairs, words,
                                                             self._ws_lanes.get(("decide", lane)))
        return res

    def assign(self, centroids: torch.Tensor, bias: Optional[torch.Tensor] = None, *, row_mask: Optional[torch.Tensor] = None,
               return_score: bool = False, amb_cap: Optional[int] = None, max_ambiguous: int = _ASSIGN_MAX_AMBIGUOUS,
               lane: int = 0):
        """``cosine_assign`` over this index: reuses the measured norm bound, the live mask (AND ``row_mask``) and a
        workspace per ``lane``.  Identical results; deleted rows and rows where ``row_mask`` is False get -1."""
        c, b = _check_assign_args(self.gallery, centroids, bias)
        words = self._mask_words(row_mask, ("assign", lane))
        labels, best64, _, self._ws_lanes[("assign", lane)] = _assign_call(
            self.gallery, c, b, self.norm_bound, self.norm_bound_dev, words, return_score, amb_cap, max_ambiguous,
            self._ws_lanes.get(("assign", lane)))
        return (labels, best64) if return_score else labels

    def score_extent(self, queries: torch.Tensor, row_mask: Optional[torch.Tensor] = None):
        """Exact fp64 ``(min, max)`` dot of each query over the live rows, [Q] each: the ``min_val`` / ``max_val`` of the
        reference's ``find_thresholds`` (code/search_image.py:85-87).  Two k = 1 searches, of ``q`` and of ``-q`` (the
        fixed-order dot of ``-q`` is the exact negative), so ``np.linspace(lo, hi, 200)`` then ``threshold_sweep`` is the
        reference's sweep end to end.  No live row (or only NaN dots): ``(+inf, -inf)``."""
        q2, squeezed = _as_2d(queries)
        hi = self.search(q2, k=1, return_dot64=True, row_mask=row_mask)[2][:, 0]
        lo = -self.search(-q2, k=1, return_dot64=True, row_mask=row_mask)[2][:, 0]
        return (lo[0], hi[0]) if squeezed else (lo, hi)

    def near_duplicates(self, threshold: float, scale: float = 1.0, *, max_pairs: int = _RANGE_MAX_PAIRS,
                        cap: Optional[int] = None, cand_cap: Optional[int] = None, row_mask: Optional[torch.Tensor] = None):
        """``gallery_self_join`` over this index (the data-governance pass): ``(i, j, scores, dot64)``, ``i < j``, sorted.
        Only pairs of two live rows (both True in ``row_mask`` when given) qualify."""
        words = self._mask_words(row_mask, "range")
        a, b, score, dot64 = _range_call(None, self.gallery, threshold, scale, self.norm_bound, self.norm_bound_dev,
                                         self._split, cap, cand_cap, max_pairs, words)
        return a.to(torch.int64), b.to(torch.int64), score, dot64

    def scores(self, ref_feature: torch.Tensor, scale: float = 100.0) -> torch.Tensor:
        """``get_similarity``'s first line for this gallery (reference code/search_image.py:107)."""
        return similarity(self.gallery, ref_feature, scale)


class _PendingSearch:
    """One query batch of a ShardedGalleryIndex whose all-gather is in flight."""

    def __init__(self, owner, gathered, work, scale, squeezed):
        self.owner, self.gathered, self.work, self.scale, self.squeezed = owner, gathered, work, scale, squeezed

    def result(self, return_dot64: bool = False):
        """(values fp32 [Q,k], global int64 ids [Q,k] [, exact fp64 dots]); stream-ordered behind the collective."""
        if self.work is not None:
            self.work.wait()          # nccl: the CURRENT STREAM waits for the collective, the host does not
            self.work = None
        if self.owner._merge is None:                                    # HIP path: rank the gathered messages as they are
            out = merge_topk_packed(self.gathered, self.scale)
        else:
            idx_parts = self.gathered[..., 0].contiguous()
            dot_parts = self.gathered[..., 1].contiguous().view(torch.float64)
            out = self.owner._merge(idx_parts, dot_parts, self.scale)   # (score, idx, dot64)
        if self.squeezed:
            out = tuple(t[0] for t in out)
        return out if return_dot64 else out[:2]


class ShardedGalleryIndex:
    """Row-sharded gallery: rank r holds rows [offset_r, offset_r + n_r) and searches them locally;
    ONE all-gather (RCCL over xGMI with the nccl backend) of the packed per-shard top-k, then an
    exact merge.  Global top-k is a subset of the union of local top-k lists, so the merged result
    equals the single-GPU result bit for bit.

    ``search`` is one batch, start to finish.  ``search_async`` returns as soon as the batch's collective
    is issued (``all_gather_into_tensor(async_op=True)``: it runs on the backend's own stream), so the next
    batch's gallery scan -- or the caller's next encode -- overlaps it; ``.result()`` makes the current
    stream wait for the collective and merges.  ``search_pipelined`` does that over a list of batches.

    ``local_search`` / ``merge`` exist so the collective and offset logic can be exercised on a
    CPU ``gloo`` group in tests; the defaults are the HIP kernels.
    """

    def __init__(self, local_gallery: torch.Tensor, group=None, norm_bound: Optional[float] = None,
                 local_search: Optional[Callable] = None, merge: Optional[Callable] = None):
        import torch.distributed as dist

        self.dist = dist
        self.group = group
        self.use_dist = dist.is_available() and dist.is_initialized()   # collectives run even for a 1-rank group
        self.world = dist.get_world_size(group) if self.use_dist else 1
        self.rank = dist.get_rank(group) if self.use_dist else 0
        self.local = local_gallery
        self._index = GalleryIndex(local_gallery, norm_bound) if local_search is None else None
        self._local_search = local_search
        self._merge = merge if merge is not None else (None if local_search is None else merge_topk)
        n_local = torch.tensor([local_gallery.shape[0]], dtype=torch.int64, device=local_gallery.device)
        if self.use_dist:
            counts = torch.empty(self.world, dtype=torch.int64, device=local_gallery.device)
            dist.all_gather_into_tensor(counts, n_local, group=group)
        else:
            counts = n_local
        self.counts = counts.cpu()
        self.offsets = torch.cumsum(self.counts, 0) - self.counts
        self.offset = int(self.offsets[self.rank])
        self.total_rows = int(self.counts.sum())

    def local_topk(self, queries: torch.Tensor, k: int = 10, scale: float = 1.0):
        """This rank's (global int64 ids [Q,k], fp64 dots [Q,k]) -- the payload of the collective."""
        q2, _ = _as_2d(queries)
        if self._local_search is None:
            _, lidx, ldot = self._index.search(q2, k, scale, return_dot64=True)
        else:
            lidx, ldot = self._local_search(q2, self.local, k)
        gidx = torch.where(lidx >= 0, lidx.to(torch.int64) + self.offset, lidx.to(torch.int64))
        return gidx, ldot

    def search_async(self, queries: torch.Tensor, k: int = 10, scale: float = 1.0, lane: int = 0) -> _PendingSearch:
        squeezed = queries.dim() == 1
        if self._local_search is None:
            q2, _ = _as_2d(queries)
            packed = self._index.search_packed(q2, k, scale, self.offset, lane)     # one kernel after the search
        else:
            gidx, ldot = self.local_topk(queries, k, scale)
            # one packed message per rank: [Q,k,2] int64 = (global id, fp64 dot bits)
            packed = torch.stack([gidx, ldot.view(torch.int64)], dim=-1).contiguous()
        if self.use_dist:
            # output = the ranks' messages concatenated along dim 0 (the layout both nccl and gloo accept)
            flat = torch.empty((self.world * packed.shape[0],) + tuple(packed.shape[1:]), dtype=packed.dtype,
                               device=packed.device)
            work = self.dist.all_gather_into_tensor(flat, packed, group=self.group, async_op=True)   # THE collective
            gathered = flat.view((self.world,) + tuple(packed.shape))
        else:
            gathered, work = packed.unsqueeze(0), None
        return _PendingSearch(self, gathered, work, scale, squeezed)

    def search(self, queries: torch.Tensor, k: int = 10, scale: float = 1.0):
        """Every rank passes the same queries; every rank gets the same global (values, int64 ids)."""
        return self.search_async(queries, k, scale).result()

    def search_pipelined(self, batches, k: int = 10, scale: float = 1.0):
        """[(values, ids)] for a sequence of query batches: batch i's all-gather overlaps batch i+1's scan."""
        out, pending = [], None
        for qb in batches:
            nxt = self.search_async(qb, k, scale)
            if pending is not None:
                out.append(pending.result())
            pending = nxt
        if pending is not None:
            out.append(pending.result())
        return out


def verify_exact_topk(index, gallery: torch.Tensor, queries: torch.Tensor, k: int = 10):
    """Proof that ``index`` (a ``GalleryIndex`` or a ``ShardedGalleryIndex`` over this rank's ``gallery`` rows) returns
    the exact global top-k for ``queries`` -- four checks that together leave no room for a wrong list:

      (a) every returned global id is re-scored in fp64 by the ONE rank that owns the row and must reproduce the merged
          dot product (sum over ranks of the owners' re-scores == merged dot64, owner count == 1);
      (b) the list is in (-dot, +id) order (so ids are unique and ties go to the lowest id);
      (c) exactly k-1 rows precede the merged k-th entry: every rank counts the entries of its local top-(k+1) list
          that rank before it, the counts are summed (all-reduce) and must equal k-1 -- a row that beats the merged
          k-th but is missing from the list (dropped by the merge, or outside a shard's candidates) breaks the count;
      (d) all ranks hold the same answer (MIN / MAX all-reduce of position-weighted checksums).

    Collectives run on the index's process group (gloo on CPU in tests, RCCL on the GPUs); with no group it checks the
    single-shard result the same way.  Returns ``("ok" | "FAILED: ...", detail dict)``.  Diagnostic: outside any timed
    region (bench.py calls it after the clock stops).
    """
    sharded = isinstance(index, ShardedGalleryIndex)
    use_dist = sharded and index.use_dist
    dist = index.dist if sharded else None
    group = index.group if sharded else None
    q2, _ = _as_2d(queries)
    qd = q2.double()
    if sharded:
        _, gidx, d64 = index.search_async(q2, k, 1.0).result(return_dot64=True)
        offset = index.offset
        lidx, ld = index.local_topk(q2, k + 1, 1.0)
    else:
        _, gidx, d64 = index.search(q2, k, 1.0, return_dot64=True)
        offset = 0
        _, lidx, ld = index.search(q2, k + 1, 1.0, return_dot64=True)
    n_local = gallery.shape[0]
    Q = q2.shape[0]
    problems = []
    # (a) owner re-score
    mine = (gidx >= offset) & (gidx < offset + n_local)
    rows = gallery[(gidx - offset).clamp(0, max(n_local - 1, 0)).reshape(-1)].double().reshape(Q, k, -1)
    re = (rows * qd.unsqueeze(1)).sum(-1)
    re = torch.where(mine, re, torch.zeros_like(re))
    owners = mine.to(torch.int32)
    if use_dist:
        dist.all_reduce(re, group=group)
        dist.all_reduce(owners, group=group)
    if not bool((owners == 1).all()):
        problems.append("an id is owned by no rank or by several")
    err = float((re - d64).abs().max()) if re.numel() else 0.0
    if not err < 1e-12:
        problems.append(f"re-scored dot differs from the merged dot64 by {err:.3e}")
    # (b) order and uniqueness
    if k > 1 and not bool(((d64[:, :-1] > d64[:, 1:]) | ((d64[:, :-1] == d64[:, 1:]) & (gidx[:, :-1] < gidx[:, 1:]))).all()):
        problems.append("merged list is not in (-dot, +id) order")
    # (c) exactly k-1 candidates rank before the merged k-th.  Each rank counts the entries of its local top-(k+1) list
    # that precede the merged k-th entry in (-dot, +id) order; the counts are summed over ranks.  If any row of any
    # shard beat the merged k-th without being in the merged list, its shard would count it (or, were it outside that
    # shard's top-(k+1), count k+1 better ones): the sum equals k-1 only for the exact global top-k.
    lval = lidx >= 0
    kd, ki = d64[:, k - 1:k], gidx[:, k - 1:k]
    before = lval & ((ld > kd) | ((ld == kd) & (lidx < ki)))
    full = gidx[:, k - 1] >= 0                                  # fewer than k rows in total: every candidate is in the list
    cnt = torch.where(full, before.sum(1), lval.sum(1)).to(torch.int64)
    if use_dist:
        dist.all_reduce(cnt, group=group)
    want = torch.where(full, torch.full_like(cnt, k - 1), (gidx >= 0).sum(1).to(torch.int64))
    if not bool((cnt == want).all()):
        problems.append("a candidate that beats the merged k-th is missing from the merged list")
    # (d) all ranks hold the same answer (position-weighted checksums: a permuted list differs)
    if use_dist:
        wq = torch.arange(1, Q + 1, dtype=torch.float64, device=gidx.device).unsqueeze(1)
        wk = torch.arange(1, k + 1, dtype=torch.float64, device=gidx.device).unsqueeze(0)
        chk = torch.stack([(gidx.double() * wq * wk).sum(), (d64 * wq * wk).sum()])
        lo, hi = chk.clone(), chk.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
        if not bool((lo == hi).all()):
            problems.append("ranks disagree on the merged result")
    detail = {"rescored_max_abs_err": err, "queries": Q, "k": k, "ranks": index.world if sharded else 1,
              "checks": "owner re-score == merged dot64; (-dot,+id) order; exactly k-1 candidates precede the merged k-th; ranks agree"}
    return ("ok" if not problems else "FAILED: " + "; ".join(problems)), detail
