"""Brute-force fp64 oracle and fixtures for the nearest-centroid and k-means tests (not a test module).

Oracle, in the style of decide_helpers.oracle_bits: the numpy fp64 score matrix ``g @ c.T + bias`` decides every row whose
maximum stands alone; every (row, centroid) within ``slack = 1e-6 * |c| * G`` of the row's maximum (the slack of the
row's best centroid added), and every product that is not finite, is re-decided with search_helpers.dot64
(oracle/search_ref.c's mmr_ref_dot64, the fixed-order dot the library decides on).  The rule: largest score wins, ties go
to the lowest centroid, a NaN score never wins, a row without a non-NaN score (or outside ``mask``) gets -1.
"""
import functools

import numpy as np
import torch

from search_helpers import dot64
from mmr_amd import synth

# (E, K, N) of the parity tests: one centroid; a tile-short gallery; N not a multiple of 32; two passes with a short
# one; a pass with exactly one live centroid (257 at E <= 512, 129 at E = 768); two full passes (E = 128, K = 300 is
# 256 + 44; 512 / 256 and 768 / 128 are one full pass each)
PARITY_SHAPES = [(128, 1, 70), (256, 40, 31), (128, 33, 1000), (128, 300, 4099), (512, 256, 4099), (512, 257, 4099),
                 (768, 128, 2051), (768, 129, 2051)]
R_EPS_REL = 8e-5        # csrc/range_common.h


def f32(x: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(x.detach().float().cpu().numpy())


@functools.lru_cache(maxsize=None)
def unit_rows(n, E, seed):
    return synth.synth_unit_rows(n, E, seed=seed)


def parity_fixture(E, K, N, dtype):
    """-> (gallery [N, E], centroids [K, E]) in ``dtype``: random unit rows, distinct seeds"""
    return unit_rows(N, E, 7000 + N + E).to(dtype), unit_rows(K, E, 9000 + K + E).to(dtype)


def euclid_bias(c: np.ndarray) -> np.ndarray:
    """-|c|^2 / 2 in fp64 of the values the library sees"""
    return -0.5 * (c.astype(np.float64) ** 2).sum(1)


def exact_score(ref, grow: np.ndarray, crow: np.ndarray, b) -> float:
    d = dot64(ref, grow, crow)
    return d if b is None else float(np.float64(d) + np.float64(b))


def pick(scores) -> int:
    """The rule on exact scores in ascending centroid order: (centroid, score) pairs -> label"""
    best, lab = 0.0, -1
    for c, s in scores:
        if s == s and (lab < 0 or s > best):
            best, lab = s, c
    return lab


def oracle_assign(ref, g: np.ndarray, c: np.ndarray, bias=None, mask=None, want_score=True):
    """-> (labels int32 [N], best64 fp64 [N] (NaN where -1), rows re-decided with mmr_ref_dot64).  g, c: contiguous fp32
    arrays holding the values the library sees; bias: fp64 [K] or None; mask: bool [N] or None."""
    N, K = g.shape[0], c.shape[0]
    g64, c64 = g.astype(np.float64), c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = g64 @ c64.T
        if bias is not None:
            s = s + np.asarray(bias, dtype=np.float64)[None, :]
        G = np.sqrt((g64 ** 2).sum(1)).max() if N else 0.0
        slack = 1e-6 * np.sqrt((c64 ** 2).sum(1)) * G
        if bias is not None:
            slack = slack + 1e-9 * np.abs(np.asarray(bias, dtype=np.float64))
        bad = ~np.isfinite(s)
        sm = np.where(bad, -np.inf, s)
        top = sm.argmax(1)
        m = sm[np.arange(N), top]
        near = bad | (sm >= (m - slack[top])[:, None] - slack[None, :])
    if not np.all(np.isfinite(slack)):
        near[:] = True
    labels = top.astype(np.int32)
    live = np.ones(N, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    redo = np.flatnonzero((near.sum(1) > 1) | bad.any(1))
    redone = 0
    for r in redo:
        if not live[r]:
            continue
        cs = np.flatnonzero(near[r])
        labels[r] = pick((int(k), exact_score(ref, g[r], c[k], None if bias is None else bias[k])) for k in cs)
        redone += 1
    labels[~live] = -1
    best = np.full(N, np.nan, dtype=np.float64)
    if want_score:
        for r in np.flatnonzero(labels >= 0):
            k = labels[r]
            best[r] = exact_score(ref, g[r], c[k], None if bias is None else bias[k])
    return labels, best, redone


def margin_eps(c: np.ndarray, bias, G: float) -> np.ndarray:
    """The kernel's per-centroid margin (csrc/assign.hip: assign_prep_kernel) in fp64: scan_margin's
    8e-5 * 1.0001 |c| G + 2^-137 plus the roundings of the fp32 bias add"""
    cn = np.sqrt((c.astype(np.float64) ** 2).sum(1)) * 1.0001
    beta = np.zeros(c.shape[0]) if bias is None else np.abs(np.asarray(bias, dtype=np.float64))
    reach = (cn * G + beta) * 1.01
    return (R_EPS_REL * cn * G + 2.0 ** -137 + 2.0 ** -23 * reach + 2.0 ** -140) * (1 + 2.0 ** -20)


def ambiguous_rows(g: np.ndarray, c: np.ndarray, bias=None, factor: float = 1.0, doc: bool = False) -> np.ndarray:
    """bool [N]: the rows a scan whose margin is ``factor`` times margin_eps cannot decide: the winner's lower bound is
    not strictly above every other centroid's upper bound, i.e. winner minus runner-up <= factor * (eps_a + eps_b).
    doc: the margin is the documented 8e-5 |c| G alone, without the kernel's upward roundings and bias terms (a floor
    for the candidate count needs the smallest sound value).  From numpy fp64 scores (the margin is 1e11 times their
    error)."""
    g64, c64 = g.astype(np.float64), c.astype(np.float64)
    s = g64 @ c64.T
    if bias is not None:
        s = s + np.asarray(bias)[None, :]
    if c.shape[0] < 2:
        return np.zeros(g.shape[0], dtype=bool)
    if doc:
        eps = R_EPS_REL * np.sqrt((c64 ** 2).sum(1)) * np.sqrt((g64 ** 2).sum(1)).max()
    else:
        G = float(np.float32(np.sqrt((g64 ** 2).sum(1)).max()) * np.float32(1.0001))
        eps = margin_eps(c, bias, G)
    eps = factor * eps
    top = s.argmax(1)
    rows = np.arange(g.shape[0])
    lo = s[rows, top] - eps[top]
    hi = s + eps[None, :]
    hi[rows, top] = -np.inf
    return lo <= hi.max(1)


def ambiguous_share(g: np.ndarray, c: np.ndarray, bias=None, factor: float = 1.0) -> float:
    """Share of rows a scan with ``factor`` times that margin cannot decide (ambiguous_rows)."""
    return float(ambiguous_rows(g, c, bias, factor).mean()) if c.shape[0] > 1 else 0.0


# ------------------------------------------------------------------ k-means
def planted_clusters(N, E, K, seed, dtype, spread=2.5, init_noise=1.5):
    """-> (gallery [N, E] in ``dtype``, true labels int64 [N], init [K, E] in ``dtype``): K unit centres, each row its centre
    plus noise, normalised; elements below 2^-30 in magnitude are zeroed so that fp64 sums of the rows are exact in any
    order (sum_is_exact checks it).  init: one row of each planted cluster, perturbed -- not the centres.  The defaults
    overlap the clusters enough that Lloyd needs 8 to 16 iterations from that init."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    centres = synth.synth_unit_rows(K, E, seed=seed + 1)
    truth = torch.randint(0, K, (N,), generator=gen)
    x = centres[truth] + spread * torch.randn(N, E, generator=gen) / E ** 0.5
    x = (x / x.norm(dim=-1, keepdim=True)).to(dtype)
    x = torch.where(x.float().abs() < 2.0 ** -30, torch.zeros_like(x), x)
    first = torch.stack([x[int(torch.nonzero(truth == k)[0])] for k in range(K)])
    init = (first.float() + init_noise * torch.randn(K, E, generator=gen) / E ** 0.5).to(dtype)
    return x, truth, init


def sum_is_exact(x: np.ndarray, unit: float) -> bool:
    """True when fp64 addition of any subset of the rows of x, in any order, is exact: every element is a multiple of
    ``unit`` (a power of two) and sum |x| over all rows stays below 2^52 units in every column, so every partial sum is
    an integer below 2^52 times ``unit``."""
    a = np.abs(x.astype(np.float64))
    q = a / unit
    return bool(np.all(q == np.floor(q)) and a.sum(0).max() < unit * 2.0 ** 52)


def lloyd_reference(ref, g_t: torch.Tensor, init: torch.Tensor, metric: str, max_iter: int, mask=None):
    """Lloyd from the definition in mmr_amd.cluster's docstrings, with the oracle's labels and torch fp64 sums (index_add_:
    exact in any order on fixtures that pass sum_is_exact).  g_t, init: CPU tensors in the gallery's dtype.
    -> (centroids, labels int32 numpy, sizes int64 numpy, n_iter, converged)"""
    K, E = init.shape
    g = f32(g_t)
    g64 = g_t.to(torch.float64)
    c = init.clone()
    prev = None
    converged = False
    for it in range(max_iter):
        cf = f32(c)
        bias = (-0.5 * c.to(torch.float64).square().sum(1)).numpy() if metric == "euclidean" else None
        labels, _, _ = oracle_assign(ref, g, cf, bias, mask, want_score=False)
        n_iter = it + 1
        if prev is not None and np.array_equal(labels, prev):
            converged = True
            break
        if n_iter == max_iter:
            break
        prev = labels
        rows = torch.from_numpy(np.flatnonzero(labels >= 0))
        idx = torch.from_numpy(labels[labels >= 0].astype(np.int64))
        sums = torch.zeros(K, E, dtype=torch.float64).index_add_(0, idx, g64[rows])
        sizes = torch.bincount(idx, minlength=K)
        if metric == "euclidean":
            keep = sizes == 0
            new = sums / sizes.clamp(min=1).to(torch.float64)[:, None]
        else:
            norm = sums.square().sum(1, keepdim=True).sqrt()
            keep = (sizes == 0) | (norm[:, 0] == 0)
            new = sums / torch.where(norm == 0, torch.ones_like(norm), norm)
        new = new.to(torch.float32).to(c.dtype)
        c = torch.where(keep[:, None], c, new)
    sizes = np.bincount(labels[labels >= 0], minlength=K).astype(np.int64)
    return c, labels, sizes, n_iter, converged
