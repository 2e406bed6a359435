"""The definition of mmr_cluster_rank / mmr_cluster_percentile_trim (include/mmr.h) restated in numpy, and the fixtures of
their tests (not a test module).  Distances come from kmeanspp_helpers.fixed_dot / fixed_norms -- mmr_ref_dot64 in
vectorised numpy, held to the C oracle bit for bit by test_kmeanspp_host and, on these fixtures' rows, by
test_cluster_trim_host -- in the definition's own expression order; the order from ``np.lexsort((rows, key, labels))``
with ``key`` the sortable image of the distance; the thresholds from ``np.percentile`` itself.

NaN.  A NaN's payload is not a value: x86 and the GPU make different ones from inf - inf.  The library stores the quiet
NaN 0x7ff8000000000000, and ``bits`` maps every NaN of either side to it before comparing bit patterns.

``mut=`` plants one mistake (MUTATIONS); the failing controls show that each changes the result on the GPU tests' own
fixtures, so a device kernel with that mistake could not pass them.
"""
import functools

import numpy as np
import torch

import assign_helpers as A
import kmeanspp_helpers as H

# (E, K, N): one row; two; 10, 12 and 21 rows in one cluster hit t >= 0.5, t < 0.5 and t == 0 at q = 95; less than a pass
# of 16 rows per group with several clusters; less than a workgroup; several workgroups with a short last one, at every E
PARITY_SHAPES = [(128, 1, 1), (128, 1, 2), (128, 1, 10), (128, 1, 12), (128, 1, 21), (128, 3, 31), (256, 8, 70),
                 (512, 17, 4099), (768, 33, 2051)]
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
METRICS = ("cosine", "euclidean")
QS = (0.0, 50.0, 95.0, 100.0)
MUTATIONS = ("lt", "by_rank", "nearest_rank", "center_fp64", "center_normalised", "tie_high", "nan_first", "noclamp")


def bits(x) -> np.ndarray:
    """int64 bit patterns of fp64 values, every NaN as the quiet NaN the library stores"""
    x = np.array(x, dtype=np.float64, copy=True)
    x[np.isnan(x)] = np.float64("nan")
    return x.view(np.int64)


def sort_key(d: np.ndarray, mut=None) -> np.ndarray:
    """uint64: ascending in the distance (sign-flipped bits), NaN above +inf"""
    b = np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)
    key = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(d), np.uint64(0) if mut == "nan_first" else ~np.uint64(0), key)


def live_of(labels: np.ndarray, K: int) -> np.ndarray:
    return (labels >= 0) & (labels < K)


def distances(g: np.ndarray, labels: np.ndarray, K: int, centers64: np.ndarray, metric: str, mut=None) -> np.ndarray:
    """fp64 [N]: the distance of every live row to its own centre, NaN elsewhere.  g: fp32 [N, E] holding the values the
    library sees; centers64: fp64 [K, E], rounded to fp32 ONCE here as the Python layer does"""
    N = g.shape[0]
    d = np.full(N, np.nan, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        norms = H.fixed_norms(g) if metric == "euclidean" and N else None
        for k in range(K):
            rows = np.flatnonzero(labels == k)
            if not rows.size:
                continue
            c = centers64[k]
            if mut == "center_normalised":
                c = c / np.sqrt((c * c).sum())
            if mut != "center_fp64":
                c = c.astype(np.float32)
            s = H.fixed_dot(np.ascontiguousarray(g[rows]), c)
            if metric == "cosine":
                dk = 1.0 - s
            else:
                nc = H.fixed_norms(c[None, :])[0]
                dk = (norms[rows] + nc) - 2.0 * s
                if mut != "noclamp":
                    dk = np.where(dk < 0.0, 0.0, dk)
            d[rows] = dk + 0.0                       # -0.0 counts as +0.0
    return d


def ranking(d: np.ndarray, labels: np.ndarray, K: int, mut=None):
    """-> (order int64 [N], start int64 [K + 1])"""
    N = d.shape[0]
    labkey = np.where(live_of(labels, K), labels, K).astype(np.int64)
    rows = np.arange(N, dtype=np.int64)
    order = np.lexsort((-rows if mut == "tie_high" else rows, sort_key(d, mut), labkey)).astype(np.int64)
    start = np.searchsorted(labkey[order], np.arange(K + 1), side="left").astype(np.int64)
    return order, start


def thresholds_of(d, order, start, K, q, mut=None) -> np.ndarray:
    thr = np.full(K, np.nan, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for k in range(K):
            seg = d[order[start[k]:start[k + 1]]]
            if seg.size:
                thr[k] = np.percentile(seg, q, method="nearest") if mut == "nearest_rank" else np.percentile(seg, q)
    return thr


def trim(d, order, start, labels, K, q, thr, mut=None):
    """-> (trimmed_labels int32 [N], kept int64 [K])"""
    live = live_of(labels, K)
    lab = np.where(live, labels, 0)
    with np.errstate(invalid="ignore"):
        if mut == "by_rank":            # the first floor(v) + 1 sorted rows of a cluster, whatever their values
            keep = np.zeros(d.shape[0], dtype=bool)
            for k in range(K):
                n = int(start[k + 1] - start[k])
                if n and thr[k] == thr[k]:
                    keep[order[start[k]:start[k] + int(np.floor((q / 100.0) * (n - 1))) + 1]] = True
        elif mut == "lt":
            keep = live & (d < thr[lab])
        else:
            keep = live & (d <= thr[lab])
    trimmed = np.where(keep, labels, -1).astype(np.int32)
    return trimmed, np.bincount(trimmed[keep], minlength=K).astype(np.int64)


class Restated:
    pass


def restate(g, labels, K, centers64, metric, qs=QS, mut=None) -> Restated:
    r = Restated()
    r.dist = distances(g, labels, K, centers64, metric, mut)
    r.order, r.start = ranking(r.dist, labels, K, mut)
    r.thresholds, r.trimmed, r.kept = {}, {}, {}
    for q in qs:
        r.thresholds[q] = thresholds_of(r.dist, r.order, r.start, K, q, mut)
        r.trimmed[q], r.kept[q] = trim(r.dist, r.order, r.start, labels, K, q, r.thresholds[q], mut)
    return r


def same(a: Restated, b: Restated) -> bool:
    return (np.array_equal(bits(a.dist), bits(b.dist)) and np.array_equal(a.order, b.order) and np.array_equal(a.start, b.start)
            and all(np.array_equal(bits(a.thresholds[q]), bits(b.thresholds[q])) and np.array_equal(a.trimmed[q], b.trimmed[q])
                    and np.array_equal(a.kept[q], b.kept[q]) for q in a.thresholds))


# ------------------------------------------------------------------ fixtures
def plant_negative(row: np.ndarray):
    """-> (centre fp32 [E], found): the row's own values with ONE element moved by one fp32 ulp, chosen so that the
    euclidean expression (n_r + n_c) - 2 s comes out NEGATIVE before the clamp (the true squared distance, about 1e-16,
    is below the rounding of the sums).  found is False when no single nudge does it; the centre is then the row itself.
    Only an fp32 gallery gives one: the sums over a unit row of 16-bit elements are exact, so their expression is 0."""
    E = row.shape[0]
    cands = np.repeat(row[None, :], 2 * E, axis=0)
    j = np.arange(E)
    cands[j, j] = np.nextafter(row, np.float32(np.inf), dtype=np.float32)
    cands[E + j, j] = np.nextafter(row, np.float32(-np.inf), dtype=np.float32)
    nr = H.fixed_norms(row[None, :])[0]
    d = (nr + H.fixed_norms(cands)) - 2.0 * H.fixed_dot(cands, row)
    ok = np.flatnonzero((d < 0.0) & (np.repeat(row[None, :], 2, axis=0).reshape(-1) != 0.0))
    return (cands[ok[0]].copy(), True) if ok.size else (row.copy(), False)


class Fixture:
    def __init__(self, gallery, labels, centers64, notes):
        self.gallery = gallery                  # CPU tensor [N, E] in the case's dtype
        self.g32 = A.f32(gallery)
        self.labels = labels                    # int32 numpy [N]
        self.centers64 = centers64              # fp64 numpy [K, E]; the library gets .astype(float32)
        self.notes = notes                      # what was planted where


@functools.lru_cache(maxsize=None)
def fixture(E, K, N, dtype) -> Fixture:
    """K == 1: every row live (N is the cluster's size), row 1 an exact duplicate of row 0.
    K >= 3: random labels; cluster K - 1 empty; labels -1, K and K + 5; in cluster 0 an exact duplicate pair and three
    identical rows far from everything (the negated first row); a row with a NaN element and a row with an inf element
    (cluster 1 at K == 3, clusters 2 and 3 otherwise); cluster 1's centre is plant_negative of one of its rows.
    Centres: the fp64 means of each cluster's finite rows, the three far rows left out (not fp32 values, so rounding them
    once matters)."""
    rng = np.random.default_rng(5200 + E + K + N)
    g = H.planted(N, E, K, dtype).clone()
    notes = {}
    if K == 1:
        labels = np.zeros(N, dtype=np.int32)
        if N >= 2:
            g[1] = g[0]
            notes["dup"] = (0, 1)
    else:
        assert K >= 3 and N >= 10 * (K - 1) // 2
        labels = rng.integers(0, K - 1, N).astype(np.int32)
        labels[:3 * (K - 1)] = np.arange(3 * (K - 1)) % (K - 1)           # every other cluster has at least three rows
        first = np.flatnonzero(labels == 0)
        if first.size < 6:
            labels[N - 6:N] = 0
            first = np.flatnonzero(labels == 0)
        g[first[2]] = g[first[0]]
        notes["dup"] = (int(first[0]), int(first[2]))
        for r in first[[1, 3, 4]]:
            g[r] = -g[first[0]]
        notes["far"] = tuple(int(r) for r in first[[1, 3, 4]])
        nan_k, inf_k = (2, 3) if K >= 8 else (1, 1)
        nan_row = int(np.flatnonzero(labels == nan_k)[-1])
        inf_row = int(np.flatnonzero(labels == inf_k)[0])
        g[nan_row, 7] = float("nan")
        g[inf_row, 9] = float("inf")
        notes.update(nan=nan_row, inf=inf_row, empty=K - 1)
        taken = {nan_row, inf_row, *first[:5].tolist()}
        dead = []
        for r0, step in ((3 * (K - 1), 1), (N // 2, 1), (N - 3, -1)):       # past the rows that give every cluster three
            r = r0
            while r in taken:
                r += step
            taken.add(r)
            dead.append(r)
        for r, l in zip(dead, (-1, K, K + 5)):
            labels[r] = l
        notes["dead"] = tuple(dead)
    g32 = A.f32(g)
    centers = np.zeros((K, E), dtype=np.float64)
    finite = np.isfinite(g32).all(1)
    finite[list(notes.get("far", ()))] = False          # the far rows stay out of their centre, so that they are its farthest
    for k in range(K):
        rows = np.flatnonzero((labels == k) & finite)
        if rows.size:
            centers[k] = g32[rows].astype(np.float64).mean(0)
    if K >= 3:
        rows = np.flatnonzero((labels == 1) & finite)
        c, found = plant_negative(g32[rows[1]])
        centers[1] = c.astype(np.float64)
        notes["negative"] = (int(rows[1]), found)
    return Fixture(g.contiguous(), labels, centers, notes)


@functools.lru_cache(maxsize=None)
def restated(E, K, N, dtype, metric) -> Restated:
    """The restatement of a parity fixture, computed once and shared"""
    f = fixture(E, K, N, dtype)
    return restate(f.g32, f.labels, K, f.centers64, metric)


def case_id(E, K, N, dtype, metric) -> str:
    return f"E{E}-K{K}-N{N}-{str(dtype).split('.')[-1]}-{metric}"


# ------------------------------------------------------------------ the reference flow
def reference_rows(seed: int, n: int = 10, E: int = 128, planted: int = 6) -> torch.Tensor:
    """fp16 [n, E]: unit rows around a prototype, row ``planted`` around another direction"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    proto, other = torch.nn.functional.normalize(torch.randn(2, E, generator=gen), dim=-1)
    x = proto[None, :] + 0.3 * torch.randn(n, E, generator=gen) / E ** 0.5
    x[planted] = other + 0.3 * torch.randn(E, generator=gen) / E ** 0.5
    return torch.nn.functional.normalize(x, dim=-1).to(torch.float16)


def reference_outlier_filter(f: np.ndarray, percentile: float = 95.0):
    """The reference's expression (code/search_image.py:295-318) on float32 numpy rows -> (centre fp32 [E], kept bool [n], d)"""
    c = f.mean(0)
    d = 1 - f @ c
    keep = d <= np.percentile(d, percentile)
    return f[keep].mean(0), keep, d
