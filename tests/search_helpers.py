"""Oracles the GPU search tests share (not a test module).

Top-k: the C oracle over the compacted gallery gallery[mask], ids mapped back -- idx, score and dot64 are compared bit
for bit.  Range search / self-join: numpy fp64 products find every pair within ``slack`` of the threshold or above it;
oracle/search_ref.c's mmr_ref_dot64 then makes the exact decision on those pairs and gives the exact bits.  ``slack``
is absolute (1e-6 suits unit rows); for scaled data pass 1e-6 * |q| * G.  A pair whose dot is NaN never matches
(``NaN >= t`` is false on both sides of the comparison)."""
import ctypes

import numpy as np
import torch

F32P = ctypes.POINTER(ctypes.c_float)


def to_np(x):
    return x.detach().float().cpu().numpy()


def plan_tpt(N, dtype):
    """(rows per scan tile, tiles per scan task) of the top-k scan for an [N, E] gallery of this dtype"""
    tr = 16 if dtype == torch.float32 else 32
    nt = (N + tr - 1) // tr
    if nt <= 256:
        return tr, 1
    m = (nt + 256 * 64 - 1) // (256 * 64)
    return tr, (nt + 256 * m - 1) // (256 * m)


def expect_topk(oracle, q, g, mask, k, scale=1.0):
    """oracle top-k over g[mask], ids mapped back -> (idx int64, score f32, dot64 f64)"""
    rows = np.flatnonzero(mask)
    Q = q.shape[0]
    if rows.size == 0:
        return (np.full((Q, k), -1, np.int64), np.full((Q, k), -np.inf, np.float32), np.full((Q, k), -np.inf, np.float64))
    oi, os_, od = oracle.cosine_topk(to_np(q), to_np(g)[rows], k, scale=scale)
    idx = np.where(oi >= 0, rows[np.clip(oi, 0, None)], -1)
    return idx, os_, od


def assert_topk(got, want):
    score, idx, d64 = got[:3]
    wi, ws, wd = want
    assert np.array_equal(idx.cpu().numpy(), wi), "indices differ from the oracle over gallery[mask]"
    assert np.array_equal(d64.cpu().numpy().view(np.int64), wd.view(np.int64)), "dot64 bits differ"
    assert np.array_equal(score.cpu().numpy().view(np.int32), ws.view(np.int32)), "score bits differ"


def dot64(ref, a, b):
    return ref.mmr_ref_dot64(a.ctypes.data_as(F32P), b.ctypes.data_as(F32P), a.shape[0])


def oracle_range(ref, q, g, tau, mask=None, slack=1e-6):
    """-> (qids, rows, dot64) sorted by (q, row); q, g contiguous fp32 arrays, mask bool [N] or None"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = q.astype(np.float64) @ g.astype(np.float64).T
    if mask is not None:
        s[:, ~mask] = -np.inf
    qs, rs = np.nonzero(s >= tau - slack)
    d = np.array([dot64(ref, q[a], g[b]) for a, b in zip(qs, rs)], dtype=np.float64)
    keep = d >= tau
    return qs[keep], rs[keep], d[keep]


def oracle_join(ref, g, tau, mask=None, slack=1e-6):
    """-> (i, j, dot64), i < j, sorted by (i, j)"""
    g64 = g.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = g64 @ g64.T
    if mask is not None:
        s[~mask, :] = -np.inf
        s[:, ~mask] = -np.inf
    a, b = np.nonzero(np.triu(s >= tau - slack, 1))
    o = np.lexsort((b, a))
    a, b = a[o], b[o]
    d = np.array([dot64(ref, g[x], g[y]) for x, y in zip(a, b)], dtype=np.float64)
    keep = d >= tau
    return a[keep], b[keep], d[keep]
