"""What the silhouette tests share (no test functions): the fp64 restatement of the definition in include/mmr.h, the error
bound B[i, c] of mmr_silhouette_sums, the samples rule in numpy, and the fixture builder.

Distances come from direct differences in row chunks -- no Gram-matrix cancellation -- so the restatement is good to a few
ulps of fp64 and can stand in for the exact value next to a bound of 1e-4.
"""
import functools

import numpy as np
import torch

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
METRICS = {"euclidean": 0, "cosine": 1}
# the shapes of test_silhouette_gpu.py's bound test; test_silhouette_host.py's failing control runs on the same ones
#   name: (N, E, K, forced cluster sizes)
SHAPES = {
    "1200x128x6": (1200, 128, 6, (1, 2, 33, 257)),      # a ragged last resident block, cluster boundaries inside tiles
    "700x512x3": (700, 512, 3, (1, 33)),
    "700x768x3": (700, 768, 3, (2, 257)),               # the 128-row resident block
    "3000x128x2": (3000, 128, 2, (2100,)),              # one cluster longer than a 2048-row chunk: two partials
}

R_EPS_REL = 8e-5                      # csrc/range_common.h, tests/margin_helpers.py
ETA_P, ETA_N = 1.7e-4, 2.0 ** -21     # eta = ETA_P |x_i||x_j| + ETA_N (|x_i|^2 + |x_j|^2)
SQRT_ULP = 2.0 ** -22
COS_DELTA = 1.7e-4 + 2.0 ** -21
CHAIN = 1.001 * 2.0 ** -13            # an fp32 chain of at most 2048 additions


def make_fixture(N, E, K, dtype, forced, seed=0, duplicates=5, strength=0.5):
    """-> (x: torch [N, E] of `dtype` on the CPU, labels: int32 numpy [N]).  K planted clusters on unit rows (row =
    normalised(strength * centre + unit noise), rounded to the dtype); clusters 0.. take the `forced` sizes, the rest
    share what is left; `duplicates` identical rows inside the last cluster; 7 random rows relabelled -1 and one relabelled
    K (both skipped) -- taken from the last cluster so the forced sizes stand; rows shuffled."""
    rng = np.random.default_rng(seed)
    forced = list(forced)
    free = K - len(forced)
    assert free >= 1
    rest = N - sum(forced)
    sizes = forced + [rest // free + (1 if i < rest % free else 0) for i in range(free)]
    assert min(sizes) >= 1 and sum(sizes) == N and sizes[-1] >= duplicates + 8 + 2
    lab = np.repeat(np.arange(K, dtype=np.int32), sizes)
    centres = rng.standard_normal((K, E))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    noise = rng.standard_normal((N, E))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    x = strength * centres[lab] + noise
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    last = np.nonzero(lab == K - 1)[0]
    if duplicates:
        x[last[1:duplicates]] = x[last[0]]
    skipped = rng.choice(last[duplicates:], 8, replace=False)
    lab[skipped[:7]] = -1
    lab[skipped[7]] = K
    perm = rng.permutation(N)
    xt = torch.from_numpy(x[perm]).to(torch.float32).to(dtype)
    return xt, lab[perm].copy()


def without_duplicates(x, lab):
    """The fixture with every row that repeats an earlier row taken out."""
    _, first = np.unique(x.to(torch.float64).numpy(), axis=0, return_index=True)
    keep = np.sort(first)
    return x[torch.from_numpy(keep)], lab[keep].copy()


def pair_distances(x64, rows, metric):
    """fp64 d(i, j) for i in `rows` (a slice) against every j: [len(rows), N]; d(i, i) = 0 exactly"""
    xi = x64[rows]
    if metric == "euclidean":
        with np.errstate(invalid="ignore", over="ignore"):         # a non-finite row: inf - inf
            d = np.sqrt(np.square(xi[:, None, :] - x64[None, :, :]).sum(-1))
    else:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            nrm = np.sqrt(np.square(x64).sum(1))
            d = 1.0 - (xi @ x64.T) / (nrm[rows, None] * nrm[None, :])
    idx = np.arange(rows.start, rows.stop)
    d[idx - rows.start, idx] = 0.0
    return d


def pair_delta(x64, rows, d, metric):
    """The per-pair error allowance delta(i, j) next to d = pair_distances(...); delta(i, i) = 0"""
    if metric == "euclidean":
        nrm = np.sqrt(np.square(x64).sum(1))
        p = nrm[rows, None] * nrm[None, :]
        n = np.square(nrm)[rows, None] + np.square(nrm)[None, :]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            eta = ETA_P * p + ETA_N * n
            delta = np.minimum(np.sqrt(eta), np.where(d > 0, eta / d, np.inf)) + SQRT_ULP * d
    else:
        delta = np.full_like(d, COS_DELTA)
    idx = np.arange(rows.start, rows.stop)
    delta[idx - rows.start, idx] = 0.0
    return delta


def sums_and_bound(x, lab, K, metric, chunk=32):
    """-> (S64 [N, K], B [N, K], sizes [K]) for a torch gallery of 16-bit rows: the definition, and the bound
    B[i, c] = sum_j delta(i, j) + CHAIN * sum_j (d(i, j) + delta(i, j)), j over the live rows with label c."""
    x64 = x.to(torch.float64).numpy()
    N = x64.shape[0]
    live = (lab >= 0) & (lab < K)
    onehot = np.zeros((N, K))
    onehot[np.nonzero(live)[0], lab[live]] = 1.0
    S, B = np.empty((N, K)), np.empty((N, K))
    for i0 in range(0, N, chunk):
        rows = slice(i0, min(N, i0 + chunk))
        d = pair_distances(x64, rows, metric)
        delta = pair_delta(x64, rows, d, metric)
        # a masked sum per cluster, not a matmul: a non-finite d of another cluster must not leak in as inf * 0
        for c in range(K):
            m = onehot[:, c] > 0
            S[rows, c] = d[:, m].sum(1)
            B[rows, c] = delta[:, m].sum(1) + CHAIN * (d[:, m] + delta[:, m]).sum(1)
    return S, B, onehot.sum(0).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(shape, dtype, metric):
    """The bound test's case, computed once a session: (x, labels, K, S64, B, sizes)"""
    N, E, K, forced = SHAPES[shape]
    x, lab = make_fixture(N, E, K, DTYPES[dtype], forced, seed=N + E + K)
    S, B, sizes = sums_and_bound(x, lab, K, metric)
    return x, lab, K, S, B, sizes


def samples_rule(sums, lab, sizes):
    """The samples rule of include/mmr.h in numpy fp64, operation for operation: [N], NaN for rows that are not live"""
    N, K = sums.shape
    out = np.full(N, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(N):
            own = int(lab[i])
            if not 0 <= own < K:
                continue
            if sizes[own] == 1:
                out[i] = 0.0
                continue
            a = sums[i, own] / np.float64(sizes[own] - 1)
            b, nan = np.float64(np.inf), bool(np.isnan(a))
            for c in range(K):
                if c == own or sizes[c] <= 0:
                    continue
                v = sums[i, c] / np.float64(sizes[c])
                nan = nan or bool(np.isnan(v))
                if v < b:
                    b = v
            mx = a if a > b else b
            out[i] = np.nan if nan else (0.0 if mx == 0.0 else (b - a) / mx)
    return out
