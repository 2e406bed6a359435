"""Brute-force fp64 oracle and fixtures for the decision-mask tests (not a test module).

Oracle, in the style of search_helpers.oracle_range: numpy fp64 ``q @ g.T`` decides every pair farther than ``slack``
from its query's threshold; search_helpers.dot64 (oracle/search_ref.c's mmr_ref_dot64, the fixed-order dot the library
decides on) decides the rest, and every pair whose product is not finite.  ``slack`` is absolute (1e-6 suits unit rows;
numpy's own fp64 error there is near 1e-15); for scaled data pass 1e-6 * |q| * G.  The result is packed with numpy into the
library's word format: bit r & 31 of word r >> 5, bits at or past N clear.
"""
import numpy as np
import torch

from search_helpers import dot64
from mmr_amd import synth


def f32(x: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(x.detach().float().cpu().numpy())


def pack_bits(bits: np.ndarray) -> np.ndarray:
    """bool [Q, N] -> uint32 [Q, ceil(N/32)]"""
    Q, N = bits.shape
    W = (N + 31) // 32
    padded = np.zeros((Q, W * 32), dtype=bool)
    padded[:, :N] = bits
    out = np.zeros((Q, W), dtype=np.uint32)
    for b in range(32):
        out |= padded[:, b::32].astype(np.uint32) << np.uint32(b)
    return out


def unpack_words(words: np.ndarray, N: int) -> np.ndarray:
    """uint32 / int32 [Q, W] -> bool [Q, N] (pad bits dropped)"""
    w = np.ascontiguousarray(words).view(np.uint32)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(w.shape[0], -1)[:, :N].astype(bool)


def oracle_bits(ref, q: np.ndarray, g: np.ndarray, thr, mask=None, slack=1e-6):
    """-> (bool [Q, N], pairs re-decided with mmr_ref_dot64).  q, g: contiguous fp32 arrays holding the values the
    library sees; thr: fp64 [Q]; mask: bool [N], rows that can pass (None: all)."""
    thr = np.asarray(thr, dtype=np.float64).reshape(-1)
    assert thr.shape[0] == q.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        s = q.astype(np.float64) @ g.astype(np.float64).T
        bits = s >= thr[:, None]
        near = ~np.isfinite(s) | (np.abs(s - thr[:, None]) <= slack)
    if mask is not None:
        near &= np.asarray(mask, dtype=bool)[None, :]
    qs, rs = np.nonzero(near)
    for a, b in zip(qs, rs):
        bits[a, b] = dot64(ref, q[a], g[b]) >= thr[a]          # NaN >= t is False: a NaN dot sets no bit
    if mask is not None:
        bits &= np.asarray(mask, dtype=bool)[None, :]
    return bits, len(qs)


def oracle_decide(ref, q, g, thr, mask=None, slack=1e-6) -> np.ndarray:
    """-> uint32 [Q, ceil(N/32)], the words mmr_cosine_decide must write"""
    return pack_bits(oracle_bits(ref, q, g, thr, mask, slack)[0])


def words_np(res) -> np.ndarray:
    """DecisionMasks (or an int32 device tensor [Q, W]) -> uint32 numpy words"""
    w = res.words if hasattr(res, "words") else res
    return np.ascontiguousarray(w.cpu().numpy()).view(np.uint32)


def boundary_fixture(ref, N: int, E: int, K: int, seed: int, dtype=torch.float32):
    """Unit rows with K planted (query, row) pairs whose thresholds sit ON the exact dot.

    -> (queries [2K, E], gallery [N, E] in ``dtype``, thr fp64 [2K], rows int [K]).  Query 2k and 2k+1 are the same
    vector; r = rows[k] is its planted row.  thr[2k] = dot64(q, r): the pair must pass (the rule is inclusive);
    thr[2k+1] = nextafter(dot64, +inf): it must fail.  So at least 2K pairs lie inside every margin, and a rule that
    decides from an approximate dot gets one twin of every pair wrong unless it reproduces dot64 to the last bit."""
    g = synth.synth_unit_rows(N, E, seed=seed).to(dtype)
    base = synth.synth_unit_rows(K, E, seed=seed + 1).to(dtype)
    q = base.repeat_interleave(2, dim=0).contiguous()
    rows = np.random.default_rng(seed + 2).choice(N, K, replace=False)
    gf, qf = f32(g), f32(q)
    thr = np.empty(2 * K, dtype=np.float64)
    for k in range(K):
        d = dot64(ref, qf[2 * k], gf[rows[k]])
        thr[2 * k] = d
        thr[2 * k + 1] = np.nextafter(d, np.inf)
    return q, g, thr, rows


def check_twins(bits: np.ndarray, rows) -> None:
    """Every planted pair passes under its own dot and fails under the next fp64 above it."""
    for k, r in enumerate(rows):
        assert bits[2 * k, r], f"pair {k}: a dot that ties its threshold must pass"
        assert not bits[2 * k + 1, r], f"pair {k}: a dot one ulp under its threshold must fail"
