"""Brute-force fp64 oracle and data builders for the threshold-sweep tests.

Oracle, in the style of test_range_gpu._oracle_range: numpy fp64 `q @ g.T` bins every pair
(`np.searchsorted(thresholds, s, side="right")`); every pair whose product lies within a window of ANY threshold, or
is not finite, is re-decided with oracle/search_ref.c's mmr_ref_dot64, the fixed-order dot the library ranks on.  The
window is 1e-6 for rows of norm about 1 (numpy's own fp64 error there is near 1e-15) and scales with the product of the
largest finite row norms for un-normalised and power-of-two-scaled inputs.
"""
import ctypes

import numpy as np
import torch

from mmr_amd import synth

F32P = ctypes.POINTER(ctypes.c_float)
NCLASS = 7


def f32(x: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(x.detach().float().cpu().numpy())


def dot64(ref, a: np.ndarray, b: np.ndarray) -> float:
    return ref.mmr_ref_dot64(a.ctypes.data_as(F32P), b.ctypes.data_as(F32P), a.shape[0])


def _max_finite_norm(x: np.ndarray) -> float:
    with np.errstate(over="ignore", invalid="ignore"):
        n = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
    n = n[np.isfinite(n)]
    return float(n.max()) if n.size else 0.0


def oracle_sweep(ref, q: np.ndarray, g: np.ndarray, labels: np.ndarray, targets: np.ndarray, thresholds: np.ndarray,
                 mask: np.ndarray = None):
    """-> (ge int64 [Q,2,T], total int64 [Q,2], pairs re-decided with mmr_ref_dot64).  q, g: fp32 arrays holding the
    values the library sees (a bf16 gallery widened to fp32); mask: bool [N], rows that count (None: all)."""
    thr = np.asarray(thresholds, dtype=np.float64)
    Q, N, T = q.shape[0], g.shape[0], thr.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        s = q.astype(np.float64) @ g.astype(np.float64).T
    window = 1e-6 * max(_max_finite_norm(q) * _max_finite_norm(g), np.finfo(np.float64).tiny)
    live = np.ones(N, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    hist = np.zeros((Q, 2, T + 1), dtype=np.int64)
    redecided = 0
    for a in range(Q):
        sa = s[a]
        fin = np.isfinite(sa)
        b = np.searchsorted(thr, np.where(fin, sa, 0.0), side="right")
        below = np.abs(sa - thr[np.clip(b - 1, 0, T - 1)])
        above = np.abs(thr[np.clip(b, 0, T - 1)] - sa)
        with np.errstate(invalid="ignore"):
            near = ~fin | (np.minimum(below, above) <= window)
        keep = live.copy()
        for r in np.nonzero(near & live)[0]:
            d = dot64(ref, q[a], g[r])
            redecided += 1
            if d != d:
                keep[r] = False            # a NaN dot is absent
            else:
                b[r] = np.searchsorted(thr, d, side="right")
        pos = labels == targets[a]
        hist[a, 1] = np.bincount(b[keep & pos], minlength=T + 1)
        hist[a, 0] = np.bincount(b[keep & ~pos], minlength=T + 1)
    # ge[..., i] = rows in the bins above i (bin = number of thresholds <= dot)
    ge = np.flip(np.cumsum(np.flip(hist, -1), -1), -1)[..., 1:]
    return np.ascontiguousarray(ge), hist.sum(-1), redecided


def labelled_gallery(N: int, E: int, seed: int, dtype=torch.float32):
    """Unit rows with class structure: g = normalize(0.12 * centre[label] + unit noise), 7 centres, labels uniform.
    -> (gallery [N,E], labels int32 [N], centres fp32 [7,E])"""
    centres = synth.synth_unit_rows(NCLASS, E, seed=seed)
    labels = torch.from_numpy(np.random.default_rng(seed + 1).integers(0, NCLASS, N).astype(np.int32))
    g = 0.12 * centres[labels.long()] + synth.synth_unit_rows(N, E, seed=seed + 2)
    g = g / g.norm(dim=-1, keepdim=True)
    return g.to(dtype), labels, centres


def labelled_queries(Q: int, E: int, centres: torch.Tensor, seed: int, dtype=torch.float32):
    """Query i is centre i with target i for i < 7; further queries are unit noise rows with targets i % 7, the last
    one (when Q > 7) with the target -5 that no row carries.  -> (queries [Q,E], targets int32 [Q])"""
    q = synth.synth_unit_rows(Q, E, seed=seed)
    n = min(Q, NCLASS)
    q[:n] = centres[:n]
    targets = torch.arange(Q, dtype=torch.int32) % NCLASS
    if Q > NCLASS:
        targets[-1] = -5
    return q.to(dtype), targets


def check_sweep(res, want_ge, want_total):
    """A ThresholdSweep of a 2-D query against the oracle's (ge, total), exactly."""
    assert np.array_equal(res.tp.cpu().numpy(), want_ge[:, 1]), "tp differs from the oracle"
    assert np.array_equal(res.fp.cpu().numpy(), want_ge[:, 0]), "fp differs from the oracle"
    assert np.array_equal(res.pos.cpu().numpy(), want_total[:, 1]), "pos differs from the oracle"
    assert np.array_equal(res.neg.cpu().numpy(), want_total[:, 0]), "neg differs from the oracle"
