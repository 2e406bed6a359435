"""Fixtures that pin the search certificates' margins from below (not a test module).

Every exact search call decides a pair from an approximate MFMA dot ``acc`` only when it lies more than ``eps`` from its
threshold (or from the k-th score) and rechecks the rest in fp64, so it is exact only if |acc - dot64| <= eps.  The
fixtures here put |acc - dot64| at 94 % of the smallest sound ``eps`` (``doc_margin``), or crowd pairs just inside it, so
that a margin term that is halved or dropped changes a result or a candidate count.  All constructions are exact: every
product and sum they rely on is a multiple of a power of two small enough to be exact in fp32 and fp64 in any order.

test_margin_fixtures_host.py asserts the properties the GPU tests rely on; read it for the arithmetic.
"""
import math

import numpy as np
import torch

R_EPS_REL = 8e-5                      # csrc/range_common.h: the MFMA accumulation term of every margin
QMAG = 2.0 ** -4                      # magnitude of the constant-magnitude operand
DELTA = 31.0 / 64.0 * 2.0 ** -13      # planted residual per element: just under half a bf16 ulp of [2^-5, 2^-4)
ULP = 2.0 ** -12                      # one bf16 ulp in [2^-5, 2^-4)
STEP = QMAG * ULP                     # 2^-16: what one element moved by one ulp adds to the dot
KS_MAX = 32                           # candidate tiles the first tier of the split top-k keeps (csrc/topk_scan.h)
TILE = 32
NDECOY = 48


def f32(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().float().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32)


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 array -> nearest-even bf16, widened back to fp32"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().float().numpy()


def exact_norm2(rows) -> np.ndarray:
    """Per-row sum of squares, exact up to one final rounding: the fp64 squares of fp32 / bf16 / fp16 values are exact
    and math.fsum adds them without intermediate rounding.  -> fp64 [N]"""
    x = f32(rows).astype(np.float64)
    if x.ndim == 1:
        x = x[None, :]
    sq = x * x
    return np.array([math.fsum(r) for r in sq.tolist()], dtype=np.float64)


def row_norms(rows) -> np.ndarray:
    """Row norms from numpy fp64 sums (relative error near 1e-15): for comparisons with room to spare -> fp64 [N]"""
    x = f32(rows).astype(np.float64)
    return np.sqrt((x * x).sum(1))


def max_norm(rows) -> float:
    """sqrt of the largest exact_norm2 (the rows near the numpy maximum are the only ones summed exactly)"""
    x = f32(rows)
    n2 = row_norms(x) ** 2
    near = np.flatnonzero(n2 >= n2.max() * (1 - 1e-12))
    return math.sqrt(float(exact_norm2(x[near]).max())) if near.size else 0.0


def doc_margin(form: str, q, g, R=None, qr=None) -> np.ndarray:
    """The margin of DESIGN.md section 3 in fp64, without the kernels' upward roundings: the smallest sound value.
    q: the rows the scan multiplied ([Q, E]; for the split routes the bf16-rounded queries qh); g: the gallery, or its
    largest row norm G as a float.  form "plain": 8e-5 |q| G.  form "split": 8e-5 |qh| G (1 + 2^-8) + qr G + |qh| R with
    R = max_row |g - hi(g)| and qr[Q] = |q - qh|.  -> fp64 [Q]"""
    G = float(g) if np.isscalar(g) else max_norm(g)
    qn = np.sqrt(exact_norm2(q))
    if form == "plain":
        return R_EPS_REL * qn * G
    assert form == "split" and R is not None and qr is not None
    return R_EPS_REL * qn * G * (1 + 2.0 ** -8) + np.asarray(qr, dtype=np.float64) * G + qn * float(R)


def resid_norm(x) -> np.ndarray:
    """|x - bf16(x)| per row, exact up to the final rounding -> fp64 [N]"""
    x = f32(x)
    if x.ndim == 1:
        x = x[None, :]
    return np.sqrt(exact_norm2(x - bf16_round(x)))          # the residual of a rounding is exact in fp32


def decoy_steps(E: int) -> np.ndarray:
    """Elements each of the 48 decoys moves, descending.  In units of D / 31 (D = the planted error, 31 * E / 128 steps):
    twelve decoys at 30 .. 25, thirty-six at 18 .. 1, each value twice.  So the 10th largest is 0.84 D and the 33rd --
    the best tile the first tier leaves out -- 0.26 D.  E = 128 keeps the repeats (D is only 31 steps there); wider rows
    take one step off every second decoy, so all 48 differ."""
    u = E // 128
    v = np.array([30 - i // 2 for i in range(12)] + [18 - i // 2 for i in range(36)], dtype=np.int64)
    j = u * v
    if u > 1:
        j = j - (np.arange(NDECOY) % 2)
    return j


class Aligned:
    """What aligned_gallery_fixture / aligned_query_fixture return.
    q [Q, E], g [N, E] fp32; base = qh . gh, the scan's product for every planted pair (exact); D = the planted error
    |q| R (gallery form) or qr |g| (query form), exact; planted / anti: rows (gallery form) or query ids (query form)
    with dot64 = base + D / base - D; decoys: rows with acc = dot64 = base + decoy_j * STEP."""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _binade_row(rng, E, signs, m_lo=1):
    """bf16-exact, |x| = 2^-5 (1 + m / 128) with m_lo <= m <= 126 (an ulp up or DELTA down stays in the binade), signed"""
    m = rng.integers(m_lo, 127, E)
    return (signs * 2.0 ** -5 * (1 + m / 128.0)).astype(np.float32)


def aligned_gallery_fixture(E: int, N: int = 20011, seed: int = 0, self_join: bool = False) -> Aligned:
    """Rounding residuals of gallery rows aligned with the query.  Query 0: 2^-4 s, s random signs (bf16-exact, so
    qr = 0).  gh = s |gh|, bf16-exact in one binade.  Planted rows gh + DELTA s (hi = gh, exact in fp32): the scan sees
    base = q . gh, the exact dot is base + D with D = 2^-4 DELTA E = |q| R.  Anti-aligned rows gh - DELTA s: exact dot
    base - D.  Decoys: gh with j elements one ulp further from zero, bf16-exact, dot base + j 2^-16 for the scan and
    exactly.  Fillers: uniform in (-2^-6, 2^-6), so their residuals (<= 2^-15 per element), norms and dots stay
    strictly below the planted rows'.  Each special row has a 32-row tile of its own; planted rows sit at row 0, at the
    last row of tile 1, above row 16384 and at row N - 1 (N % 32 != 0).
    self_join: the query also sits in the gallery, as row ``partner`` = (2^-4 + DELTA) s, whose own residual DELTA s is
    aligned with every gh-like row too: the pair (partner, planted) is off by |r_a| |g_p| + |a_h| |r_p| nearly in full.
    |gh| then stays in the top quarter of the binade so that the first product is close to its Cauchy-Schwarz bound."""
    assert E % 128 == 0 and N % TILE != 0 and N > 16384 + 20 * TILE
    rng = np.random.default_rng(1000 * E + seed)
    s = rng.choice(np.array([-1.0, 1.0]), E)
    q = (QMAG * s).astype(np.float32)[None, :]
    gh = _binade_row(rng, E, s, 96 if self_join else 1)
    g = rng.uniform(-2.0 ** -6, 2.0 ** -6, (N, E)).astype(np.float32)
    planted = np.array([0, 2 * TILE - 1, 16384 + 9 * TILE + 5, N - 1])
    anti = np.array([400 * TILE + 3, 600 * TILE + 31])
    g[planted] = gh + np.float32(DELTA) * s.astype(np.float32)
    g[anti] = gh - np.float32(DELTA) * s.astype(np.float32)
    js = decoy_steps(E)
    order = rng.permutation(NDECOY)                              # rank in the ladder is unrelated to the row id
    decoys = np.array([(10 + 7 * int(t)) * TILE + int(rng.integers(0, TILE)) for t in order])
    for row, j in zip(decoys, js):
        d = gh.copy()
        pick = rng.choice(E, int(j), replace=False)
        d[pick] += np.float32(ULP) * s[pick].astype(np.float32)
        g[row] = d
    partner = 300 * TILE + 17
    if self_join:
        g[partner] = ((QMAG + DELTA) * s).astype(np.float32)
    base = float(q[0].astype(np.float64) @ gh.astype(np.float64))
    D = QMAG * DELTA * E
    return Aligned(q=q, g=g, gh=gh, s=s, base=base, D=D, planted=planted, anti=anti, decoys=decoys, decoy_j=js, step=STEP,
                   partner=partner if self_join else None, E=E, N=N)


QC = 2.0 ** -5 * 1.5                  # |qh_i| of the query form: mid-binade, bf16-exact
QSTEP = QC * 2.0 ** -13               # what one decoy element of the query form adds to the dot


def query_decoy_steps(E: int) -> np.ndarray:
    """Elements (an even number: half where the query's signs agree with the planted row's, half where they differ) of
    the 48 decoys of the query form, descending: decoy_steps' ladder in units of D / 31, D = 31 E / 48 of these steps."""
    v = np.array([30 - i // 2 for i in range(12)] + [18 - i // 2 for i in range(36)], dtype=np.float64)
    return (2 * np.floor(v * E / 96.0)).astype(np.int64)


def aligned_query_fixture(E: int, N: int = 20011, seed: int = 0) -> Aligned:
    """The mirror: the query's rounding residual aligned with a row.  Planted rows g0 = 2^-4 s.  qh = QC t with t = s on
    half of the elements and -s on the other half, so base = qh . g0 = 0 exactly.  Query 0 = qh + DELTA s (hi = qh; the
    scan sees 0, the exact dot is D = 2^-4 DELTA E = qr |g0|), query 1 = qh - DELTA s (exact dot -D).  Decoys: 2^-13 t on j / 2
    elements of either half and 0 elsewhere, so s . d = 0 and the scan's product j QSTEP is also the exact dot.  Fillers:
    -t |u|, u uniform in (0, 2^-6), rounded to bf16: every dot negative.  Every row is bf16-exact (R = 0) and none is longer
    than g0, so qr G is the whole split part of the margin."""
    assert E % 128 == 0 and N % TILE != 0 and N > 16384 + 20 * TILE
    rng = np.random.default_rng(2000 * E + seed)
    s = rng.choice(np.array([-1.0, 1.0]), E)
    agree = rng.permutation(E)[:E // 2]
    t = -s.copy()
    t[agree] = s[agree]
    differ = np.setdiff1d(np.arange(E), agree)
    qh = (QC * t).astype(np.float32)
    ds = np.float32(DELTA) * s.astype(np.float32)
    q = np.stack([qh + ds, qh - ds])
    g = bf16_round((-t * rng.uniform(2.0 ** -9, 2.0 ** -6, (N, E))).astype(np.float32))
    planted = np.array([0, 2 * TILE - 1, 16384 + 9 * TILE + 5, N - 1])
    g[planted] = (QMAG * s).astype(np.float32)
    js = query_decoy_steps(E)
    order = rng.permutation(NDECOY)
    decoys = np.array([(10 + 7 * int(k)) * TILE + int(rng.integers(0, TILE)) for k in order])
    for row, j in zip(decoys, js):
        d = np.zeros(E, dtype=np.float32)
        for half in (agree, differ):
            pick = rng.choice(half, int(j) // 2, replace=False)
            d[pick] = np.float32(2.0 ** -13) * t[pick].astype(np.float32)
        g[row] = d
    return Aligned(q=q, g=g, qh=qh, s=s, t=t, base=0.0, D=QMAG * DELTA * E, planted=planted, anti=np.array([], dtype=np.int64),
                   decoys=decoys, decoy_j=js, step=QSTEP, E=E, N=N)


def crowd_fixture(dtype, E: int, N: int, Q: int, tau: float, seed: int = 0):
    """Unit rows crowded round a threshold.  Row r belongs to query r % Q: g_r = a u + sqrt(1 - a^2) w with u the
    (rounded) query's direction, w a random unit vector orthogonal to it and a spread evenly over tau +- 3 eps,
    eps = 8e-5; then rounded to ``dtype`` (bf16 / fp16).  -> (q [Q, E], g [N, E] in dtype, dots fp64 [Q, N] of the rounded
    values -- numpy fp64 products, within 1e-15 of the oracle's dot64: test_margin_fixtures_host.py checks it)."""
    gen = torch.Generator().manual_seed(7000 + E + seed)
    q = torch.randn(Q, E, generator=gen, dtype=torch.float64)
    q = (q / q.norm(dim=1, keepdim=True)).to(dtype)
    u = q.double()
    u = u / u.norm(dim=1, keepdim=True)
    own = torch.arange(N) % Q
    w = torch.randn(N, E, generator=gen, dtype=torch.float64)
    w = w - (w * u[own]).sum(1, keepdim=True) * u[own]
    w = w / w.norm(dim=1, keepdim=True)
    a = tau + 3 * R_EPS_REL * (2 * torch.rand(N, generator=gen, dtype=torch.float64) - 1)
    # the dot that counts is taken with the rounded query, whose norm is not exactly 1
    a = (a / q.double().norm(dim=1)[own]).unsqueeze(1)
    g = (a * u[own] + (1 - a * a).sqrt() * w).to(dtype)
    dots = q.double().numpy() @ g.double().numpy().T
    return q, g, dots


def assign_crowd_fixture(dtype, E: int, N: int, K: int, seed: int = 0):
    """Rows between two centroids.  Row r lies along c_a + c_b (a = r % K, b = (r + 1) % K) plus g (c_a - c_b) with g
    chosen so that score(a) - score(b) is spread evenly over +-6 eps (eps = 8e-5, so +-3 (eps_a + eps_b)), then rounded
    to ``dtype``.  -> (gallery [N, E], centroids [K, E] in dtype, scores fp64 [N, K] of the rounded values)"""
    gen = torch.Generator().manual_seed(9000 + E + seed)
    c = torch.randn(K, E, generator=gen, dtype=torch.float64)
    c = (c / c.norm(dim=1, keepdim=True)).to(dtype)
    c64 = c.double()
    a = torch.arange(N) % K
    b = (a + 1) % K
    mid, dif = c64[a] + c64[b], c64[a] - c64[b]
    scale = 1.0 / mid.norm(dim=1, keepdim=True)
    gap = 6 * R_EPS_REL * (2 * torch.rand(N, 1, generator=gen, dtype=torch.float64) - 1)
    # (x mid + y dif) . dif = x (|c_a|^2 - |c_b|^2) + y |dif|^2 = gap
    y = (gap - scale * (c64[a].square().sum(1, keepdim=True) - c64[b].square().sum(1, keepdim=True))) / dif.square().sum(1, keepdim=True)
    g = (scale * mid + y * dif).to(dtype)
    return g, c, g.double().numpy() @ c64.numpy().T
