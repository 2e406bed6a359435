"""The k-means++ seeding's definition restated in numpy and Python integers, and the fixtures of its tests (not a test
module).  The definition is the comment above mmr_kmeanspp_seed in include/mmr.h; ``restate`` follows it line by line, and
the device result must EQUAL it.

Weights.  assign_helpers.oracle_assign lets a numpy fp64 matrix decide what stands clear of a slack and re-decides the
rest with the C oracle's mmr_ref_dot64.  Here the slack that pattern asks for, ``1e-9 * Dmax * S``, is 137 to 275 weight
units (Dmax * S lies in [2^37, 2^38)): no weight stands clear of it, every one has to be decided in the fixed order.  So
``fixed_dot`` restates mmr_ref_dot64 in vectorised numpy -- exact products, each of 64 lanes summed left to right, the xor
butterfly 32, 16, ..., 1 -- and decides EVERY weight with it in the definition's own expression order; test_kmeanspp_host
holds it to ``search_helpers.dot64`` bit for bit, on random rows of every scale and on the GPU fixtures' own rows.  ``dots="blas"`` swaps in the plain fp64 matrix product: for the
statistical comparison with sklearn only, where the last bit does not matter and 200 runs have to stay cheap.

``mut=`` plants one mistake (MUTATIONS); the failing controls show that each changes the result on the GPU tests' own
fixtures, so a device kernel with that mistake could not pass them.
"""
import functools
import math

import numpy as np
import torch

import assign_helpers as A
from mmr_amd import _header

WMAX = 2 ** 38 - 1
BLOCK_ROWS = _header.load().constants["MMR_KMEANSPP_BLOCK_ROWS"]      # rows per block of the sampling and of the pass
MUTATIONS = ("ge", "argmax", "nomin", "mask_weighted", "tie_high", "round", "shift1", "step0_all")
METRICS = {"euclidean": 0, "cosine": 1}

# (E, K, N) of the parity tests: one row; less than a pass of 16 rows; less than a block; several blocks with a short
# last one, at every E and so every chunk width of the exact dot
PARITY_SHAPES = [(128, 1, 1), (128, 3, 31), (256, 8, 70), (128, 8, 4099), (512, 17, 4099), (768, 33, 2051)]


def trials(K: int) -> int:
    return 2 + int(math.log(K))


def fixed_dot(g: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fp64 [N]: mmr_ref_dot64(g[i], c) for every row, bit for bit.  g: fp32 [N, E], c: fp32 [E], E a multiple of 64."""
    N, E = g.shape
    assert E % 64 == 0 and c.shape == (E,)
    per = E // 64
    p = g.astype(np.float64).reshape(N, 64, per) * c.astype(np.float64).reshape(1, 64, per)      # exact products
    acc = np.zeros((N, 64), dtype=np.float64)
    for j in range(per):
        acc = acc + p[:, :, j]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off]
    return np.ascontiguousarray(acc[:, 0])


def fixed_norms(g: np.ndarray) -> np.ndarray:
    """fp64 [N]: n_i = dot(x_i, x_i) in the fixed order"""
    N, E = g.shape
    per = E // 64
    g64 = g.astype(np.float64).reshape(N, 64, per)
    p = g64 * g64
    acc = np.zeros((N, 64), dtype=np.float64)
    for j in range(per):
        acc = acc + p[:, :, j]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off]
    return np.ascontiguousarray(acc[:, 0])


def host_norm_bound(g: np.ndarray) -> float:
    """A norm bound for tests without a device: fp32(sqrt(max n_i)) * fp32(1.000001).  The GPU tests read the library's own."""
    n = fixed_norms(g).max() if g.shape[0] else 0.0
    return float(np.float32(np.sqrt(n)) * np.float32(1.000001))


def scale_of(G: float, metric: str, mut=None):
    """-> (shift, Dmax) from the fp32 norm bound G"""
    g = float(np.float32(G))
    dmax = (4.0 * g) * g if metric == "euclidean" else 1.0 + g * g
    shift = 0 if dmax == 0.0 else 37 - (math.frexp(dmax)[1] - 1)
    if mut == "shift1":
        shift += 1
    return shift, dmax


def weights_from(d: np.ndarray, shift: int, mut=None) -> np.ndarray:
    """int64 weights of the distances d: min(int64(trunc(max(d, 0) * 2^shift)), 2^38 - 1), 0 for NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.ldexp(np.where(d > 0.0, d, 0.0), shift)          # NaN > 0 is False: weight 0
        x = np.rint(x) if mut == "round" else np.trunc(x)
    return np.minimum(x, float(WMAX)).astype(np.int64)


def sample(w: np.ndarray, b: int, first_live: int, mut=None) -> int:
    """The sampling rule on a weight vector (int64) and a variate"""
    T = int(w.sum())
    if T == 0:
        return first_live
    r = (int(b) * T) >> 53
    cum = np.cumsum(w)
    i = int(np.searchsorted(cum, r, side="left" if mut == "ge" else "right"))
    return min(i, w.shape[0] - 1)


def variate_for(target: int, T: int) -> int:
    """The smallest variate b with (b * T) >> 53 == target (T <= 2^53, 0 <= target < T)"""
    b = -((-(target << 53)) // T)
    assert 0 <= b < 2 ** 53 and (b * T) >> 53 == target
    return b


def pick(pots, mut=None) -> int:
    """The winner among the trials' potentials (Python ints): the smallest, ties to the lowest trial"""
    if mut == "argmax":
        return max(range(len(pots)), key=lambda t: (pots[t], -t))
    best = min(pots)
    hits = [t for t, p in enumerate(pots) if p == best]
    return hits[-1] if mut == "tie_high" else hits[0]


class Restated:
    def __init__(self, indices, potentials, shift, closest, cands):
        self.indices = np.asarray(indices, dtype=np.int64)
        self.cands = cands                          # per step, the rows its trials drew
        self.potentials = np.asarray(potentials, dtype=np.int64)
        self.shift = shift
        self.closest = closest                      # int64 [N] after the last step


def restate(g: np.ndarray, K: int, L: int, variates, G: float, metric: str = "euclidean", mask=None, mut=None,
            dots: str = "fixed", gram=None) -> Restated:
    """The definition.  g: contiguous fp32 [N, E] holding the values the library sees; variates: int [K, L] (numpy / nested
    lists), or a callable ``variates(c, closest, L) -> L ints`` that sees the weight vector step c samples from (how the
    crafted-target tests place their draws); G: the fp32 norm bound; mask: bool [N] or None.  dots="blas": plain fp64
    products, from ``gram`` = g64 @ g64.T when the caller has it."""
    N, E = g.shape
    live = np.ones(N, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    first_live = int(np.argmax(live))
    shift, _ = scale_of(G, metric, mut)
    if dots == "fixed":
        norms = fixed_norms(g)
    else:
        g64 = g.astype(np.float64)
        norms = (g64 * g64).sum(1)

    def weights_to(c: int) -> np.ndarray:
        with np.errstate(invalid="ignore", over="ignore"):
            dot = fixed_dot(g, g[c]) if dots == "fixed" else (gram[:, c] if gram is not None else g64 @ g64[c])
            d = (norms + norms[c]) - 2.0 * dot if metric == "euclidean" else 1.0 - dot
        w = weights_from(d, shift, mut)
        if mut != "mask_weighted":
            w[~live] = 0
        return w

    def draws(c, closest, n):
        row = variates(c, closest, n) if callable(variates) else [int(v) for v in np.asarray(variates)[c][:n]]
        assert len(row) == n and all(0 <= int(b) < 2 ** 53 for b in row)
        return [int(b) for b in row]

    w0 = np.ones(N, dtype=np.int64) if mut == "step0_all" else live.astype(np.int64)
    indices = [sample(w0, draws(0, w0, 1)[0], first_live, mut)]
    drawn = [[indices[0]]]
    closest = weights_to(indices[0])
    potentials = [int(closest.sum())]
    for c in range(1, K):
        cands = [sample(closest, b, first_live, mut) for b in draws(c, closest, L)]
        trial = [weights_to(r) if mut == "nomin" else np.minimum(closest, weights_to(r)) for r in cands]
        pots = [int(t.sum()) for t in trial]
        win = pick(pots, mut)
        drawn.append(cands)
        indices.append(cands[win])
        closest = trial[win]
        potentials.append(pots[win])
    return Restated(indices, potentials, shift, closest, drawn)


# ------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def planted(N, E, K, dtype, seed=None):
    """A planted fixture in ``dtype`` (assign_helpers.planted_clusters with min(K, 8) clusters, at least 1) -> gallery [N, E]"""
    kc = max(1, min(K, 8, N))
    while True:       # every planted cluster needs a row
        try:
            return A.planted_clusters(N, E, kc, (seed if seed is not None else 4100 + N + E + K), dtype)[0].contiguous()
        except IndexError:
            kc -= 1


def parity_mask(N: int) -> np.ndarray:
    """Clears row 0, row N - 1 and a run of 20 rows across the first block boundary of the pass and of the sampling
    (BLOCK_ROWS - 6 .. BLOCK_ROWS + 13, where the gallery has them)"""
    m = np.ones(N, dtype=bool)
    m[0] = False
    m[N - 1] = False
    m[BLOCK_ROWS - 6:BLOCK_ROWS + 14] = False
    return m


def variates_of(K: int, L: int, seed: int) -> np.ndarray:
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 2 ** 53, (K, L), generator=g, dtype=torch.int64).numpy()


# ------------------------------------------------------------------ the cases the GPU tests and the failing controls share
class Case:
    def __init__(self, name, gallery, K, L, variates, metric, mask, craft=None):
        self.name, self.gallery, self.K, self.L, self.metric = name, gallery, K, L, metric
        self.variates = variates                  # int64 numpy [K, L], or None: placed against the restatement by ``craft``
        self.craft = craft                        # crafted_variates or edge_variates: (case, G) -> (variates, Restated)
        self.mask = mask                          # bool numpy [N] or None
        self.g32 = A.f32(gallery)


def parity_case(E, K, N, dtype, metric, masked, L=None) -> Case:
    L = trials(K) if L is None else L
    name = f"E{E}-K{K}-N{N}-{str(dtype).split('.')[-1]}-{metric}-{'masked' if masked else 'all'}-L{L}"
    return Case(name, planted(N, E, K, dtype), K, L, variates_of(K, L, 1000 + E + K + N), metric, parity_mask(N) if masked else None)


def crafted_variates(case: Case, G: float):
    """-> (variates int64 [K, L], Restated): every step's draws are placed from the restatement's own prefix sums -- the
    first positive-weight row (b = 0, with leading zero weights when row 0 is masked or chosen), the last positive-weight
    row (b = 2^53 - 1), r one below the prefix sum at the end of the sampling's block 0 and r equal to it; further trials
    repeat these.  Step 0 draws r equal to that prefix sum.  The last two are the boundary of the sampling's FIRST level;
    which rows they give depends on the weights there: under parity_mask, which clears the rows on both sides of the
    boundary, they are the last live row below the cleared run and the first above it (zero weights at the boundary).
    The rows BLOCK_ROWS - 1 and BLOCK_ROWS themselves are edge_variates' business."""
    B = BLOCK_ROWS
    out = np.zeros((case.K, case.L), dtype=np.int64)

    def place(c, closest, n):
        cum = np.cumsum(closest)
        T = int(cum[-1])
        if T == 0:
            row = [0, 2 ** 53 - 1, 1, 2 ** 52][:n]
        else:
            edge = int(cum[min(B, closest.shape[0]) - 1])        # prefix sum at the end of block 0
            marks = [0, 2 ** 53 - 1]
            marks.append(variate_for(edge - 1, T) if edge >= 1 else 0)
            marks.append(variate_for(edge, T) if edge < T else 2 ** 53 - 1)
            row = [marks[3]] if c == 0 else [marks[t % 4] for t in range(n)]
        out[c, :len(row)] = row
        return row

    res = restate(case.g32, case.K, case.L, place, G, case.metric, case.mask)
    return out, res


def crafted_case(dtype=torch.bfloat16) -> Case:
    return Case("crafted-E128-K6-N700", planted(700, 128, 6, dtype), 6, 4, None, "euclidean", parity_mask(700), crafted_variates)


def edge_targets(N: int, L: int):
    """Per step c >= 1 the L rows its trials are to draw: the last row of a block of the sampling and the first row of the
    next block, for every block boundary the gallery has, one boundary a step when L == 2 and one row a step when L == 1"""
    rows = [r for b in range(BLOCK_ROWS, N, BLOCK_ROWS) for r in (b - 1, b)]
    return [rows[i:i + L] for i in range(0, len(rows), L)]


def edge_variates(case: Case, G: float):
    """-> (variates int64 [K, L], Restated) for an UNMASKED case with K = 1 + len(edge_targets): step 0 draws the last row
    of the gallery (b = 2^53 - 1); step c draws edge_targets' rows, whose weights are positive -- a last row of a block by
    the largest r that gives it (one below its inclusive prefix sum: the last thread of the block's scan), a first row by
    the smallest (r equal to the prefix sum of the block before: the first thread of the next)."""
    targets = edge_targets(case.g32.shape[0], case.L)
    assert case.mask is None and case.K == 1 + len(targets)
    out = np.zeros((case.K, case.L), dtype=np.int64)

    def place(c, closest, n):
        if c == 0:
            row = [2 ** 53 - 1]
        else:
            cum = np.cumsum(closest)
            T = int(cum[-1])
            assert all(closest[r] > 0 for r in targets[c - 1])
            row = [variate_for(int(cum[r]) - 1 if (r + 1) % BLOCK_ROWS == 0 else int(cum[r - 1]), T) for r in targets[c - 1]]
        out[c, :len(row)] = row
        return row

    res = restate(case.g32, case.K, case.L, place, G, case.metric, None)
    return out, res


def edge_case(L: int, dtype=torch.bfloat16, metric="euclidean") -> Case:
    N = 2 * BLOCK_ROWS + 188                      # two boundaries and a short last block
    K = 1 + len(edge_targets(N, L))
    return Case(f"edges-E128-K{K}-N{N}-L{L}", planted(N, 128, 6, dtype), K, L, None, metric, None, edge_variates)


def duplicates_case() -> Case:
    """Three distinct rows, each four times (row i holds value i % 3); K = 5 with 16 trials a step, so that trials tie"""
    base = planted(3, 128, 3, torch.bfloat16, seed=77)
    g = base[torch.arange(12) % 3].contiguous()
    return Case("duplicates-E128-K5-N12", g, 5, 16, variates_of(5, 16, 4242), "euclidean", None)


def control_cases():
    """What the failing controls run each mutation on: a masked parity case of each metric, the crafted targets, the block
    edges and the duplicates -- all of them cases of test_kmeanspp_gpu"""
    return [parity_case(256, 8, 70, torch.bfloat16, "euclidean", True), parity_case(128, 8, 4099, torch.float16, "cosine", True),
            crafted_case(), edge_case(1), edge_case(2), duplicates_case()]
