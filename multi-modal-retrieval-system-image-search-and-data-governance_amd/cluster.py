"""Clustering a device-resident gallery: the reference's ``KMeans`` step (``get_cluster_features`` /
``get_text_cluster_features``, code/search_image.py:185-292) for N rows instead of 10-50 shots.

    cluster_sums(gallery, labels, K)                 per-cluster fp64 sums and sizes, bit-for-bit reproducible
    kmeans_plusplus(gallery, K)                      sklearn's greedy k-means++ seeding on the device, exact and reproducible
    kmeans(gallery, K, init=...)                     Lloyd iterations: exact assignment -> sums -> new centroids
    reference_vector_by_clustering(features, shots)  the reference's rule on top of kmeans(K = 2)
    silhouette_sums / silhouette_samples / silhouette_score   sklearn's silhouette of a labelling, one pairwise scan on the GPU
    select_k(gallery, ks=(2, 3, 4))                  the reference's loop: kmeans for each K, the best silhouette wins
    rank_in_clusters(gallery, labels, K)             each row's exact distance to its own centre, each cluster's rows nearest first
    percentile_trim / trimmed_centers / outlier_filter   the reference's outlier-trimmed class centre (search_image.py:295-318)

Both halves of an iteration are HIP kernels (csrc/assign.hip, csrc/cluster.hip), and so is the silhouette's N x N scan
(csrc/silhouette.hip); only the [K, E] centroid update and the mean of the samples run in torch.  Labels are exact (``search.cosine_assign``), so a run is deterministic and "the labels repeat" is a sound
stopping rule.
"""
import math
from typing import Dict, NamedTuple, Optional, Sequence, Union

import torch

from . import _lib
from . import search as _search

_SCAN_DTYPES = (torch.bfloat16, torch.float16)


def cluster_sums(gallery: torch.Tensor, labels: torch.Tensor, K: int, workspace: Optional[torch.Tensor] = None):
    """-> (sums fp64 [K, E], sizes int64 [K]): the sum and the number of the rows carrying each label.  Labels outside
    ``[0, K)`` (-1 included) are skipped; an empty cluster gets zeros.  ``gallery``: fp32, bf16 or fp16 [N, E] on the GPU;
    ``labels``: integer [N].  No floating-point atomics: the additions' order depends on the labels, N and K alone, so two
    runs agree bit for bit (include/mmr.h: mmr_cluster_sums)."""
    if not gallery.is_cuda:
        raise RuntimeError("gallery must live on the GPU (there is no CPU path)")
    if gallery.dim() != 2:
        raise ValueError(f"gallery must be [N, E], got shape {tuple(gallery.shape)}")
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1")
    g = gallery.contiguous() if gallery.dtype in _search._NATIVE_DTYPES else gallery.float().contiguous()
    N, E = g.shape
    if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != (N,) or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"labels must be an integer tensor [{N}]")
    lab = labels.to(device=g.device, dtype=torch.int32).contiguous()
    L = _lib.lib()
    need = L.mmr_cluster_sums_workspace_bytes(N, E, K)
    if need == 0:
        raise ValueError(f"cluster_sums: unsupported sizes N={N} E={E} K={K} (K <= 65535, E <= 65536)")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=g.device)
    sums = torch.empty(K, E, dtype=torch.float64, device=g.device)
    sizes = torch.empty(K, dtype=torch.int64, device=g.device)
    _lib.check(L.mmr_cluster_sums(g.data_ptr(), _lib.dtype_code(g.dtype), N, E, lab.data_ptr(), K, sums.data_ptr(),
                                  sizes.data_ptr(), workspace.data_ptr(), workspace.numel(), _lib.stream_ptr(g.device)))
    return sums, sizes


class KMeansResult(NamedTuple):
    centroids: torch.Tensor      # [K, E] in the gallery's dtype: the centroids ``labels`` was assigned against
    labels: torch.Tensor         # int32 [N]; -1 for a row outside row_mask (or one whose scores are all NaN)
    sizes: torch.Tensor          # int64 [K]
    inertia: float               # euclidean: sum |x - c|^2 over the labelled rows; cosine: sum (1 - x.c); fp64, from best64
    n_iter: int                  # assignments made
    converged: bool              # the labels repeated


def new_centroids(sums: torch.Tensor, sizes: torch.Tensor, previous: torch.Tensor, metric: str) -> torch.Tensor:
    """The centroid update, and its definition: in torch fp64 on the [K, E] sums, ``sums / sizes`` (euclidean) or
    ``sums / sqrt(sum(sums^2))`` (cosine), cast ``.to(float32).to(previous.dtype)``.  An empty cluster -- or, for the cosine
    metric, one whose sum is zero -- keeps its previous centroid."""
    if metric == "euclidean":
        keep = sizes == 0
        new = sums / sizes.clamp(min=1).to(torch.float64)[:, None]
    else:
        norm = sums.square().sum(1, keepdim=True).sqrt()
        keep = (sizes == 0) | (norm[:, 0] == 0)
        new = sums / torch.where(norm == 0, torch.ones_like(norm), norm)
    new = new.to(torch.float32).to(previous.dtype)
    return torch.where(keep[:, None], previous, new)


def centroid_bias(centroids: torch.Tensor, metric: str) -> Optional[torch.Tensor]:
    """``-0.5 * |c|^2`` in torch fp64 of the ROUNDED centroids for the euclidean metric (arg-max of ``x.c - |c|^2 / 2`` is
    arg-min of ``|x - c|``); None for cosine."""
    if metric != "euclidean":
        return None
    return -0.5 * centroids.to(torch.float64).square().sum(1)


def _row_norms2(g: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """fp64 sum of |g[r]|^2 over ``rows``, in slices (no [N, E] fp64 copy)"""
    total = torch.zeros((), dtype=torch.float64, device=g.device)
    for i in range(0, rows.numel(), 1 << 16):
        total += g[rows[i:i + (1 << 16)]].to(torch.float64).square().sum()
    return total


# ---------------------------------------------------------------------------------------------------- k-means++ seeding
KMEANSPP_TRIALS_MAX = _lib.HEADER.constants["MMR_KMEANSPP_TRIALS_MAX"]
KMEANSPP_BLOCK_ROWS = _lib.HEADER.constants["MMR_KMEANSPP_BLOCK_ROWS"]     # rows per block of the two-level sampling
KMEANSPP_K_MAX = 65535
KMEANSPP_N_MAX = 1 << 24
_KMEANSPP_E = (128, 256, 512, 768)
_INITS = ("sample", "k-means++")


def kmeanspp_trials(K: int) -> int:
    """sklearn's default number of candidates per step, ``2 + int(ln K)``, capped at ``KMEANSPP_TRIALS_MAX``."""
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1")
    return min(2 + int(math.log(K)), KMEANSPP_TRIALS_MAX)


def kmeanspp_variates(K: int, L: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The seeding's randomness, drawn once on the host: int64 [K, L], each uniform in ``[0, 2^53)`` --
    ``torch.randint(0, 2**53, (K, L), generator=generator)`` on the CPU.  Row c feeds step c; step 0 uses only ``[0, 0]``."""
    K, L = int(K), int(L)
    if K < 1 or not 1 <= L <= KMEANSPP_TRIALS_MAX:
        raise ValueError(f"K must be >= 1 and L in [1, {KMEANSPP_TRIALS_MAX}], got K={K} L={L}")
    if generator is not None and generator.device.type != "cpu":
        raise ValueError("kmeanspp_variates draws on the CPU: pass a CPU generator")
    return torch.randint(0, 2 ** 53, (K, L), generator=generator, dtype=torch.int64)


def _kmeanspp_call(g: torch.Tensor, K: int, L: int, metric: str, words: Optional[torch.Tensor], variates: torch.Tensor,
                   norm_bound_dev: torch.Tensor):
    """mmr_kmeanspp_seed on checked arguments -> (centers [K, E], indices int32 [K], potentials int64 [K], shift int32 [1])"""
    N, E = g.shape
    dev = g.device
    lib = _lib.lib()
    need = lib.mmr_kmeanspp_workspace_bytes(N, E, K, L)
    if need == 0:
        raise ValueError(f"kmeans_plusplus: unsupported sizes N={N} E={E} K={K} L={L}")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    var_dev = variates.to(dev).contiguous()
    indices = torch.empty(K, dtype=torch.int32, device=dev)
    potentials = torch.empty(K, dtype=torch.int64, device=dev)
    shift = torch.empty(1, dtype=torch.int32, device=dev)
    centers = torch.empty(K, E, dtype=g.dtype, device=dev)
    _lib.check(lib.mmr_kmeanspp_seed(g.data_ptr(), _lib.dtype_code(g.dtype), N, E, K, L, _METRICS[metric], _lib.ptr(words),
                                     var_dev.data_ptr(), 0.0, _lib.ptr(norm_bound_dev), indices.data_ptr(), potentials.data_ptr(),
                                     shift.data_ptr(), centers.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
    return centers, indices, potentials, shift


def kmeans_plusplus(gallery: torch.Tensor, K: int, *, metric: str = "euclidean", row_mask: Optional[torch.Tensor] = None,
                    generator: Optional[torch.Generator] = None, variates: Optional[torch.Tensor] = None,
                    n_local_trials: Optional[int] = None, return_potentials: bool = False):
    """-> (centers [K, E] in the gallery's dtype, indices int64 [K]): greedy k-means++ seeds of a bf16 / fp16 gallery [N, E]
    on the GPU, the shape of ``sklearn.cluster.kmeans_plusplus``'s result.  ``return_potentials``: also (potentials int64
    [K], shift int).  Exact and reproducible: the result EQUALS a restatement in integers, and two runs agree bit for bit.

    The definition (include/mmr.h: mmr_kmeanspp_seed).  Greedy k-means++ as in ``sklearn.cluster._kmeans._kmeans_plusplus``
    (sample_weight = 1) with integer weights.  E in (128, 256, 512, 768), 1 <= N <= 2^24, 1 <= K <= 65535 and K <= the live
    rows; rows where ``row_mask`` (bool [N]) is False are never chosen and have weight 0.  Trials per step
    L = ``n_local_trials``, default ``kmeanspp_trials(K)`` = 2 + int(ln K), 1 <= L <= 16.  ``variates``: int64 [K, L], each
    in [0, 2^53); default ``kmeanspp_variates(K, L, generator)``.  ``metric``: ``"euclidean"`` or ``"cosine"`` (the spherical
    rule of ``kmeans``).
    Scale: G = ``gallery_norm_bound(gallery)`` widened to fp64; Dmax = 4 G G (euclidean) or 1 + G G (cosine);
    shift = 37 - ilogb(Dmax) (0 when Dmax == 0); S = 2^shift.
    Distance of row i to centre c, with dot the fixed-order exact fp64 dot of ``cosine_topk`` and n_i = dot(x_i, x_i):
    d = (n_i + n_c) - 2 dot(x_i, x_c) (euclidean) or 1 - dot(x_i, x_c) (cosine);
    w = min(int64(trunc(max(d, 0) S)), 2^38 - 1), and 0 where d is NaN.  All sums of weights are int64.
    Sampling from weights w with total T and a variate b: r = (b T) >> 53; the sample is the smallest row whose inclusive
    prefix sum exceeds r; the lowest live row when T == 0.
    Step 0: w = 1 on live rows, one sample with variates[0, 0] gives indices[0]; closest = the weights to that row;
    potentials[0] = sum(closest).  Step c >= 1: L samples from closest with variates[c]; trial_t = min(closest, weights to
    candidate t), pot_t = sum(trial_t); the smallest pot_t wins, ties to the lowest t; indices[c] = its row,
    closest = trial_winner, potentials[c] = pot_winner.
    A chosen row has weight 0 and is not drawn again while T > 0; when the distinct rows run out the remaining seeds repeat
    the lowest live row (``kmeans`` tolerates the empty clusters).  Rows with non-finite elements: weight 0 where d is NaN,
    the result otherwise unspecified but in range.

    One C call enqueues the whole seeding (a gallery pass, a sampling launch and a pick per step); the only host read is
    the count of ``row_mask``'s live rows."""
    if metric not in _METRICS:
        raise ValueError(f"metric must be 'euclidean' or 'cosine', got {metric!r}")
    if not isinstance(gallery, torch.Tensor) or gallery.dim() != 2 or gallery.dtype not in _SCAN_DTYPES:
        raise ValueError(f"kmeans_plusplus needs a bf16 or fp16 gallery [N, E], got {getattr(gallery, 'dtype', None)} "
                         f"{tuple(getattr(gallery, 'shape', ()))}")
    N, E = gallery.shape
    K = int(K)
    if E not in _KMEANSPP_E or not 1 <= N <= KMEANSPP_N_MAX:
        raise ValueError(f"kmeans_plusplus: unsupported sizes N={N} E={E} (E in {_KMEANSPP_E}, 1 <= N <= 2^24)")
    if not 1 <= K <= KMEANSPP_K_MAX:
        raise ValueError(f"K must be in [1, {KMEANSPP_K_MAX}], got {K}")
    if K > N:
        raise ValueError(f"kmeans_plusplus needs {K} live rows, the gallery has {N}")
    L = kmeanspp_trials(K) if n_local_trials is None else int(n_local_trials)
    if not 1 <= L <= KMEANSPP_TRIALS_MAX:
        raise ValueError(f"n_local_trials must be in [1, {KMEANSPP_TRIALS_MAX}], got {L}")
    if variates is None:
        variates = kmeanspp_variates(K, L, generator)
    else:
        if not isinstance(variates, torch.Tensor) or variates.dtype != torch.int64 or tuple(variates.shape) != (K, L):
            raise ValueError(f"variates must be an int64 tensor [{K}, {L}], got {getattr(variates, 'dtype', None)} "
                             f"{tuple(getattr(variates, 'shape', ()))}")
        if int(variates.min()) < 0 or int(variates.max()) >= 2 ** 53:
            raise ValueError("variates must lie in [0, 2^53)")
    if not gallery.is_cuda:
        raise RuntimeError("gallery must live on the GPU (there is no CPU path)")
    g = gallery.contiguous()
    _search._check_row_mask(row_mask, N, g.device)
    words = None
    if row_mask is not None:
        live = int(row_mask.sum())
        if live < K:
            raise ValueError(f"kmeans_plusplus needs {K} live rows, the gallery has {live}")
        words = _search._pack_row_mask(row_mask, None, N)
    centers, indices, potentials, shift = _kmeanspp_call(g, K, L, metric, words, variates, _search.gallery_norm_bound(g))
    if return_potentials:
        return centers, indices.to(torch.int64), potentials, int(shift)
    return centers, indices.to(torch.int64)


def kmeans(gallery: torch.Tensor, K: int, *, init: Union[str, torch.Tensor], metric: str = "euclidean", max_iter: int = 100,
           row_mask: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
           max_ambiguous: int = _search._ASSIGN_MAX_AMBIGUOUS) -> KMeansResult:
    """Lloyd's k-means over a bf16 / fp16 gallery [N, E] on the GPU, every assignment exact.

    ``init``: a [K, E] tensor (cast to the gallery's dtype); ``"sample"``: K distinct live rows, the first K of
    ``torch.randperm(live rows, generator=generator)``; or ``"k-means++"``: the seeds of ``kmeans_plusplus(gallery, K,
    metric=metric, row_mask=row_mask, generator=generator)``, sklearn's default start -- its variates are drawn on the host,
    so ``generator`` must then be a CPU generator (``"sample"`` also takes a device one).  Each iteration is
    ``cosine_assign`` (bias ``centroid_bias``) -> ``cluster_sums`` -> ``new_centroids``; those three docstrings are the
    definition, so a run can be reproduced bit for bit.  ``metric="cosine"`` is spherical k-means (no bias, centroids
    re-normalised).  ``row_mask`` (bool [N]): rows where it is False take no part and get -1.  Stops when the labels
    repeat -- deterministic, since labels are exact -- or after ``max_iter`` assignments: centroids are rounded to 16
    bits after every update, which can make Lloyd cycle between a few label sets instead of converging, and ``max_iter``
    bounds that (``converged`` is then False).  The returned labels are the assignment against the returned centroids."""
    if metric not in ("euclidean", "cosine"):
        raise ValueError(f"metric must be 'euclidean' or 'cosine', got {metric!r}")
    if not gallery.is_cuda:
        raise RuntimeError("gallery must live on the GPU (there is no CPU path)")
    if gallery.dim() != 2 or gallery.dtype not in _SCAN_DTYPES:
        raise ValueError(f"kmeans needs a bf16 or fp16 gallery [N, E], got {gallery.dtype} {tuple(gallery.shape)}")
    K, max_iter = int(K), int(max_iter)
    if K < 1 or max_iter < 1:
        raise ValueError("K and max_iter must be >= 1")
    g = gallery.contiguous()
    N, E = g.shape
    _search._check_row_mask(row_mask, N, g.device)
    if isinstance(init, str):
        if init not in _INITS:
            raise ValueError(f"init must be a [K, E] tensor, 'sample' or 'k-means++', got {init!r}")
        if init == "k-means++":
            c = kmeans_plusplus(g, K, metric=metric, row_mask=row_mask, generator=generator)[0]
        else:
            live = torch.arange(N, device=g.device) if row_mask is None else torch.nonzero(row_mask).reshape(-1)
            if live.numel() < K:
                raise ValueError(f"init='sample' needs {K} live rows, the gallery has {live.numel()}")
            perm = torch.randperm(live.numel(), generator=generator, device=generator.device if generator is not None else "cpu")
            c = g[live[perm[:K].to(g.device)]].contiguous()
    else:
        if not isinstance(init, torch.Tensor) or tuple(init.shape) != (K, E):
            raise ValueError(f"init must be a [{K}, {E}] tensor, 'sample' or 'k-means++'")
        c = init.to(device=g.device, dtype=g.dtype).contiguous()
    words = None if row_mask is None else _search._pack_row_mask(row_mask, None, N)
    nb_dev = _search.gallery_norm_bound(g)
    ws_a = ws_s = None
    prev = None
    converged = False
    for it in range(max_iter):
        bias = centroid_bias(c, metric)
        labels, best64, _, ws_a = _search._assign_call(g, c, bias, None, nb_dev, words, True, None, max_ambiguous, ws_a)
        n_iter = it + 1
        if prev is not None and torch.equal(labels, prev):
            converged = True
            break
        if n_iter == max_iter:
            break
        prev = labels
        if ws_s is None:
            ws_s = torch.empty(max(_lib.lib().mmr_cluster_sums_workspace_bytes(N, E, K), 256), dtype=torch.uint8, device=g.device)
        sums, sizes = cluster_sums(g, labels, K, ws_s)
        c = new_centroids(sums, sizes, c, metric)
    rows = torch.nonzero(labels >= 0).reshape(-1)
    sizes = torch.bincount(labels[rows].to(torch.int64), minlength=K)
    score = best64[rows].sum()
    if metric == "euclidean":
        inertia = float(_row_norms2(g, rows) - 2.0 * score)
    else:
        inertia = float(rows.numel() - score)
    return KMeansResult(c, labels, sizes, inertia, n_iter, converged)


def reference_vector_by_clustering(features: torch.Tensor, shots: int, *, init: Union[str, torch.Tensor] = "sample",
                                   generator: Optional[torch.Generator] = None, max_iter: int = 100,
                                   return_indices: bool = False):
    """The reference's ``get_cluster_features`` rule (code/search_image.py:185-232) on ``kmeans(K=2)``: cluster the encoded
    samples [n, E] in two; when the clusters are balanced (``|n0 - n1| / n < 0.2``) take the ``shots`` rows nearest the
    mean of the two centres, otherwise the ``shots`` rows of the majority cluster nearest its centre
    (``np.argsort(distances)[:shots]``, stable); return their mean, NOT re-normalised, as fp32 [E].

    The clustering runs on the features' 16-bit form (fp16 unless they are bf16); the centres (the means of the final
    clusters, ``cluster_sums / sizes``), the distances and the mean are fp64 torch on the caller's own values.  ``init``:
    ``"k-means++"`` (sklearn's default seeding, ``kmeans_plusplus`` with ``generator``), ``"sample"`` with ``generator``
    (the default here), or two explicit centres.  E must then be one ``kmeans_plusplus`` takes.
    ``return_indices``: also the chosen row ids (int64, nearest first)."""
    if features.dim() != 2:
        raise ValueError(f"features must be [n, E], got shape {tuple(features.shape)}")
    shots = int(shots)
    if shots < 1:
        raise ValueError("shots must be >= 1")
    g = features if features.dtype in _SCAN_DTYPES else features.to(torch.float16)
    res = kmeans(g, 2, init=init, metric="euclidean", max_iter=max_iter, generator=generator)
    f64 = features.to(torch.float64)
    n = f64.shape[0]
    sums, sizes = cluster_sums(g, res.labels, 2)
    n0, n1 = (int(x) for x in sizes.tolist())
    if n0 == 0 or n1 == 0:       # one cluster took everything: its centre is the only one
        centres = (sums.sum(0) / max(n0 + n1, 1))[None, :].expand(2, -1)
    else:
        centres = sums / sizes.to(torch.float64)[:, None]
    if abs(n0 - n1) / n < 0.2:
        d = (f64 - centres.mean(0)).square().sum(1).sqrt()
        idx = torch.argsort(d, stable=True)[:shots]
    else:
        major = 0 if n0 >= n1 else 1
        rows = torch.nonzero(res.labels == major).reshape(-1)
        d = (f64[rows] - centres[major]).square().sum(1).sqrt()
        idx = rows[torch.argsort(d, stable=True)[:shots]]
    vec = f64[idx].mean(0).to(torch.float32)
    return (vec, idx) if return_indices else vec


# ---------------------------------------------------------------------------------------------------- silhouette
SILHOUETTE_K_MAX = _lib.HEADER.constants["MMR_SILHOUETTE_K_MAX"]
_METRICS = {"euclidean": 0, "cosine": 1}


def _silhouette_args(gallery: torch.Tensor, labels: torch.Tensor, K, metric: str):
    if metric not in _METRICS:
        raise ValueError(f"metric must be 'euclidean' or 'cosine', got {metric!r}")
    if not gallery.is_cuda:
        raise RuntimeError("gallery must live on the GPU (there is no CPU path)")
    if gallery.dim() != 2 or gallery.dtype not in _SCAN_DTYPES:
        raise ValueError(f"silhouette needs a bf16 or fp16 gallery [N, E], got {gallery.dtype} {tuple(gallery.shape)}")
    g = gallery.contiguous()
    N, E = g.shape
    if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != (N,) or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"labels must be an integer tensor [{N}]")
    lab = labels.to(device=g.device, dtype=torch.int32).contiguous()
    if K is None:
        K = int(lab.max()) + 1 if N else 1
    K = int(K)
    if K < 1 or K > SILHOUETTE_K_MAX:
        raise ValueError(f"K must be in [1, {SILHOUETTE_K_MAX}], got {K}")
    return g, lab, K


def _silhouette_sums(g: torch.Tensor, lab: torch.Tensor, K: int, metric: str, workspace: Optional[torch.Tensor]):
    N, E = g.shape
    L = _lib.lib()
    need = L.mmr_silhouette_workspace_bytes(N, E, K, _lib.dtype_code(g.dtype))
    if need == 0:
        raise ValueError(f"silhouette_sums: unsupported sizes N={N} E={E} K={K} (E in 128, 256, 512, 768; K <= {SILHOUETTE_K_MAX})")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=g.device)
    sums = torch.empty(N, K, dtype=torch.float64, device=g.device)
    sizes = torch.empty(K, dtype=torch.int64, device=g.device)
    _lib.check(L.mmr_silhouette_sums(g.data_ptr(), _lib.dtype_code(g.dtype), N, E, lab.data_ptr(), K, _METRICS[metric],
                                     sums.data_ptr(), sizes.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                     _lib.stream_ptr(g.device)))
    return sums, sizes


def _silhouette_samples(sums: torch.Tensor, lab: torch.Tensor, sizes: torch.Tensor) -> torch.Tensor:
    N, K = sums.shape
    samples = torch.empty(N, dtype=torch.float64, device=sums.device)
    _lib.check(_lib.lib().mmr_silhouette_samples(sums.data_ptr(), lab.data_ptr(), sizes.data_ptr(), N, K, samples.data_ptr(),
                                                 _lib.stream_ptr(sums.device)))
    return samples


def silhouette_sums(gallery: torch.Tensor, labels: torch.Tensor, K: int, metric: str = "euclidean",
                    workspace: Optional[torch.Tensor] = None):
    """-> (sums fp64 [N, K], sizes int64 [K]): ``sums[i, c]`` = the sum of the distances from row i to the rows carrying
    label c, ``sizes[c]`` their number.  Labels outside ``[0, K)`` (-1 included, what ``kmeans`` gives masked rows) are
    skipped as columns, but EVERY row gets its sums: ``sums / sizes`` is the mean distance of any row to any cluster.
    ``metric``: ``"euclidean"`` (sklearn's default, the reference's) or ``"cosine"`` (``1 - cos``); a row's distance to
    itself is exactly 0.  ``gallery``: bf16 or fp16 [N, E] on the GPU, E in (128, 256, 512, 768); K <= 1024.

    One N x N scan on the matrix cores, approximate within a stated bound (include/mmr.h: mmr_silhouette_sums; DESIGN.md
    section 3, "Silhouette"): about 2e-4 relative on unit rows.  Near-duplicate rows are where it is loosest: exact
    duplicates measure about ``sqrt(1e-7 |x|^2)`` apart instead of 0, which moves a sample by up to about 5e-5.  A row with
    a non-finite element makes its cluster's column and its own row of ``sums`` non-finite.  No floating-point atomics:
    two runs agree bit for bit."""
    g, lab, K = _silhouette_args(gallery, labels, K, metric)
    return _silhouette_sums(g, lab, K, metric, workspace)


def silhouette_samples(gallery: torch.Tensor, labels: torch.Tensor, K: Optional[int] = None, metric: str = "euclidean") -> torch.Tensor:
    """-> fp64 [N]: ``sklearn.metrics.silhouette_samples`` on the rows whose label is in ``[0, K)``, NaN for every other row.
    ``K=None``: ``labels.max() + 1``.  With ``a`` = the mean distance to the row's own cluster (itself excluded) and ``b`` =
    the smallest mean distance to another non-empty cluster: ``(b - a) / max(a, b)``; 0 for a row alone in its cluster.
    The samples are the exact fp64 rule applied to ``silhouette_sums`` (whose docstring states the accuracy)."""
    g, lab, K = _silhouette_args(gallery, labels, K, metric)
    sums, sizes = _silhouette_sums(g, lab, K, metric, None)
    return _silhouette_samples(sums, lab, sizes)


def silhouette_score(gallery: torch.Tensor, labels: torch.Tensor, K: Optional[int] = None, metric: str = "euclidean") -> float:
    """``sklearn.metrics.silhouette_score``: the mean of ``silhouette_samples`` over the labelled rows, taken in torch fp64 on
    the device.  ValueError, as sklearn, unless 2 <= non-empty clusters <= labelled rows - 1."""
    g, lab, K = _silhouette_args(gallery, labels, K, metric)
    sums, sizes = _silhouette_sums(g, lab, K, metric, None)
    n_clusters, n_rows = int((sizes > 0).sum()), int(sizes.sum())
    if not 2 <= n_clusters <= n_rows - 1:
        raise ValueError(f"silhouette_score needs 2 <= non-empty clusters <= labelled rows - 1, got {n_clusters} clusters over {n_rows} rows")
    samples = _silhouette_samples(sums, lab, sizes)
    live = (lab >= 0) & (lab < K)
    return float(samples[live].mean())


class SelectKResult(NamedTuple):
    best_k: int                          # the K with the largest score; ties go to the smallest K
    scores: Dict[int, float]             # K -> silhouette_score of kmeans(K)'s labels
    results: Dict[int, KMeansResult]     # K -> that run


def best_k_of(scores: Dict[int, float]) -> int:
    """The selection rule: the largest score, ties to the smallest K; a NaN score never wins."""
    best = None
    for k in sorted(scores):
        s = scores[k]
        if s == s and (best is None or s > scores[best]):
            best = k
    if best is None:
        raise ValueError("no K has a score")
    return best


def select_k(gallery: torch.Tensor, ks: Sequence[int] = (2, 3, 4), *, init: str = "sample",
             generator: Optional[torch.Generator] = None, metric: str = "euclidean", max_iter: int = 100) -> SelectKResult:
    """The reference's K-selection loop (code/search_image.py:256-259) on the GPU: ``kmeans(gallery, K, init=init,
    generator=generator, metric=metric, max_iter=max_iter)`` for each K of ``ks`` in the order given, each scored with
    ``silhouette_score(gallery, labels, K, metric)``.  ``init``: ``"sample"`` or ``"k-means++"`` (``kmeans``).  ``generator``
    is consumed run after run, so a seeded generator makes the whole selection reproducible."""
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 2 or len(set(ks)) != len(ks):
        raise ValueError(f"ks must be distinct integers >= 2, got {ks}")
    scores, results = {}, {}
    for k in ks:
        results[k] = kmeans(gallery, k, init=init, metric=metric, max_iter=max_iter, generator=generator)
        scores[k] = silhouette_score(gallery, results[k].labels, k, metric)
    return SelectKResult(best_k_of(scores), scores, results)


# ---------------------------------------------------------------------------------------------------- ranking and trim
RANK_K_MAX = 65535
_RANK_E = (128, 256, 512, 768)


class ClusterRanking(NamedTuple):
    dist: torch.Tensor           # fp64 [N]: each row's distance to its own cluster's centre; NaN for a row that is not live
    order: torch.Tensor          # int64 [N]: cluster k's rows at [start[k], start[k + 1]), nearest first; then the other rows
    start: torch.Tensor          # int64 [K + 1]
    centers: torch.Tensor        # fp32 [K, E]: the centres the distances were taken to

    def members(self, k: int) -> torch.Tensor:
        """Cluster k's rows (int64), nearest first, ties to the lower row id."""
        k = int(k)
        if not 0 <= k < self.start.numel() - 1:
            raise IndexError(f"cluster {k} outside [0, {self.start.numel() - 1})")
        lo, hi = (int(x) for x in self.start[k:k + 2].tolist())
        return self.order[lo:hi]

    def nearest(self, shots: int) -> torch.Tensor:
        """int64 [K, shots]: the ``shots`` rows nearest each cluster's centre, nearest first -- the reference's
        ``np.argsort(distances)[:shots]`` for every cluster at once -- padded with -1 where a cluster is shorter."""
        shots = int(shots)
        if shots < 1:
            raise ValueError("shots must be >= 1")
        N = self.order.numel()
        pos = self.start[:-1, None] + torch.arange(shots, device=self.start.device)[None, :]
        inside = pos < self.start[1:, None]
        if N == 0:
            return torch.full_like(pos, -1)
        return torch.where(inside, self.order[pos.clamp(max=N - 1)], torch.full_like(pos, -1))


class TrimmedCenters(NamedTuple):
    centers: torch.Tensor        # fp64 [K, E]: the mean of each cluster's kept rows, NOT re-normalised; NaN where none is kept
    keep: torch.Tensor           # bool [N]: the rows that went into the centres
    thresholds: torch.Tensor     # fp64 [K]: the percentile of each cluster's distances (NaN: empty, or a NaN distance)
    sizes: torch.Tensor          # int64 [K]: the rows each cluster had
    kept: torch.Tensor           # int64 [K]: the rows each cluster kept


def _rank_args(gallery: torch.Tensor, labels: torch.Tensor, K, metric: str):
    """The checks ``rank_in_clusters`` and ``trimmed_centers`` share, ValueErrors before the device is asked for
    -> (gallery, int32 labels, K)"""
    if metric not in _METRICS:
        raise ValueError(f"metric must be 'euclidean' or 'cosine', got {metric!r}")
    if not isinstance(gallery, torch.Tensor) or gallery.dim() != 2 or gallery.dtype not in _search._NATIVE_DTYPES:
        raise ValueError(f"gallery must be an fp32, bf16 or fp16 tensor [N, E], got {getattr(gallery, 'dtype', None)} "
                         f"{tuple(getattr(gallery, 'shape', ()))}")
    N, E = gallery.shape
    if E not in _RANK_E or N >= 2 ** 31 - 1:
        raise ValueError(f"unsupported sizes N={N} E={E} (E in {_RANK_E}, N < 2^31 - 1)")
    K = int(K)
    if not 1 <= K <= RANK_K_MAX:
        raise ValueError(f"K must be in [1, {RANK_K_MAX}], got {K}")
    if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != (N,) or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"labels must be an integer tensor [{N}]")
    if not gallery.is_cuda:
        raise RuntimeError("gallery must live on the GPU (there is no CPU path)")
    return gallery.contiguous(), labels.to(device=gallery.device, dtype=torch.int32).contiguous(), K


def rank_in_clusters(gallery: torch.Tensor, labels: torch.Tensor, K: int, *, centers: Optional[torch.Tensor] = None,
                     metric: str = "cosine", workspace: Optional[torch.Tensor] = None) -> ClusterRanking:
    """Every row's exact distance to its own cluster's centre and each cluster's rows in order of it, in one gallery pass
    plus sorts of row ids (include/mmr.h: mmr_cluster_rank is the definition).  ``gallery``: fp32, bf16 or fp16 [N, E] on
    the GPU, E in (128, 256, 512, 768); ``labels``: integer [N], a row outside ``[0, K)`` (-1 included) is not live and
    gets NaN.  ``centers``: [K, E], rounded to fp32 once; None: the clusters' means, ``cluster_sums``'s fp64 sums / sizes
    rounded to fp32 (NaN for an empty cluster).  ``metric="cosine"``: ``1 - x.c``, the reference's ``outlier_filter`` rule,
    the centre not normalised; ``"euclidean"``: the SQUARED distance ``(|x|^2 + |c|^2) - 2 x.c``, clamped at 0.  The dots
    are the fixed-order exact fp64 dots of ``cosine_topk``.  Order: (distance, row id) ascending, NaN after +inf."""
    g, lab, K = _rank_args(gallery, labels, K, metric)
    N, E = g.shape
    dev = g.device
    if centers is None:
        sums, sizes = cluster_sums(g, lab, K)
        c = (sums / sizes.to(torch.float64)[:, None]).to(torch.float32)
    else:
        if not isinstance(centers, torch.Tensor) or tuple(centers.shape) != (K, E) or not centers.is_floating_point():
            raise ValueError(f"centers must be a floating-point tensor [{K}, {E}]")
        c = centers.to(device=dev, dtype=torch.float32).contiguous()
    L = _lib.lib()
    need = L.mmr_cluster_rank_workspace_bytes(N, E, K)
    if need == 0:
        raise ValueError(f"rank_in_clusters: unsupported sizes N={N} E={E} K={K}")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    dist = torch.empty(N, dtype=torch.float64, device=dev)
    order = torch.empty(N, dtype=torch.int32, device=dev)
    start = torch.empty(K + 1, dtype=torch.int64, device=dev)
    _lib.check(L.mmr_cluster_rank(g.data_ptr(), _lib.dtype_code(g.dtype), N, E, lab.data_ptr(), K, c.data_ptr(), _METRICS[metric],
                                  dist.data_ptr(), order.data_ptr(), start.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                  _lib.stream_ptr(dev)))
    return ClusterRanking(dist, order.to(torch.int64), start, c)


def percentile_trim(ranking: ClusterRanking, labels: torch.Tensor, q: float = 95.0):
    """-> (thresholds fp64 [K], trimmed_labels int32 [N], kept int64 [K]): ``thresholds[k] = np.percentile(cluster k's
    distances, q)`` bit for bit (linear interpolation; NaN for an empty cluster or one holding a NaN distance);
    ``trimmed_labels`` keeps a row's label where its distance is ``<=`` its cluster's threshold and is -1 elsewhere;
    ``kept`` counts the rows kept.  ``labels``: the ones ``ranking`` was made with (include/mmr.h:
    mmr_cluster_percentile_trim)."""
    q = float(q)
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"q must be in [0, 100], got {q}")
    N, K = ranking.dist.numel(), ranking.start.numel() - 1
    dev = ranking.dist.device
    if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != (N,) or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"labels must be an integer tensor [{N}]")
    if not ranking.dist.is_cuda:
        raise RuntimeError("the ranking must live on the GPU (there is no CPU path)")
    lab = labels.to(device=dev, dtype=torch.int32).contiguous()
    order = ranking.order.to(torch.int32).contiguous()
    thresholds = torch.empty(K, dtype=torch.float64, device=dev)
    trimmed = torch.empty(N, dtype=torch.int32, device=dev)
    kept = torch.empty(K, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().mmr_cluster_percentile_trim(ranking.dist.data_ptr(), order.data_ptr(), ranking.start.data_ptr(),
                                                      lab.data_ptr(), N, K, q, thresholds.data_ptr(), trimmed.data_ptr(),
                                                      kept.data_ptr(), _lib.stream_ptr(dev)))
    return thresholds, trimmed, kept


def trimmed_centers(gallery: torch.Tensor, labels: torch.Tensor, K: int, *, percentile: float = 95.0, metric: str = "cosine",
                    centers: Optional[torch.Tensor] = None, row_mask: Optional[torch.Tensor] = None) -> TrimmedCenters:
    """The reference's outlier-trimmed class centre (``outlier_filter``, code/search_image.py:295-318) for every class of
    a labelled gallery at once: ``rank_in_clusters`` (distances to ``centers``, default the classes' means) ->
    ``percentile_trim`` -> ``cluster_sums`` over the rows kept -> ``sums / kept`` in torch fp64.  A class that keeps
    nothing gets NaN; the centres are NOT re-normalised, as in the reference.  ``row_mask`` (bool [N]): rows where it is
    False take no part, their labels count as -1.  ``~keep & (labels in [0, K))`` is the per-class outlier list."""
    percentile = float(percentile)
    if not 0.0 <= percentile <= 100.0:
        raise ValueError(f"percentile must be in [0, 100], got {percentile}")
    g, lab, K = _rank_args(gallery, labels, K, metric)
    _search._check_row_mask(row_mask, g.shape[0], g.device)
    if row_mask is not None:
        lab = torch.where(row_mask, lab, torch.full_like(lab, -1))
    ranking = rank_in_clusters(g, lab, K, centers=centers, metric=metric)
    thresholds, trimmed, kept = percentile_trim(ranking, lab, percentile)
    sums, _ = cluster_sums(g, trimmed, K)
    return TrimmedCenters(sums / kept.to(torch.float64)[:, None], trimmed >= 0, thresholds,
                          ranking.start[1:] - ranking.start[:-1], kept)


def outlier_filter(features: torch.Tensor, percentile: float = 95.0, return_keep: bool = False):
    """The reference's ``outlier_filter`` (code/search_image.py:295-318) for one class: the mean of the rows, the cosine
    distances ``1 - rows @ mean``, the rows within ``np.percentile(distances, percentile)``, and the mean of those, NOT
    re-normalised -> fp32 [E].  ``trimmed_centers`` with K = 1 and every label 0.  ``features``: fp16, bf16 or fp32
    [n, E] on the GPU, n >= 1.  ``return_keep``: also the rows kept (bool [n])."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1:
        raise ValueError(f"features must be [n, E] with n >= 1, got shape {tuple(getattr(features, 'shape', ()))}")
    labels = torch.zeros(features.shape[0], dtype=torch.int32, device=features.device)
    res = trimmed_centers(features, labels, 1, percentile=percentile, metric="cosine")
    vec = res.centers[0].to(torch.float32)
    return (vec, res.keep) if return_keep else vec
