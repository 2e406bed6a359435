"""CPU: the threshold sweep's host side.  Argument validation of the C ABI returns before any launch; the workspace does
not grow with N; ThresholdSweep.metrics() / best() against a direct evaluation of the reference's formulas
(CLIP/lab3.py:39-65: precision = TP / (TP + FP), recall = TP / (TP + FN), F1 = 2PR / (P + R), each 0 where its
denominator is 0; the best threshold is the first one with the largest F1); the Python wrappers' argument errors."""
import ctypes
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def _grid(values):
    return (ctypes.c_double * len(values))(*values)


def _call(L, *, q=16, gallery=16, hi=None, dtype=1, Q=4, N=100, E=512, labels=16, targets=16, thr=(0.1, 0.2, 0.3), T=None,
          bound=1.0, mask=None, cand_cap=8, ge=16, total=16, counts=16, ws=16, ws_bytes=1 << 30):
    """Device pointers are fake (16): every call here must return from the host checks, which never dereference them."""
    grid = None if thr is None else _grid(thr)
    T = (0 if thr is None else len(thr)) if T is None else T
    return L.mmr_threshold_sweep(q, gallery, hi, dtype, Q, N, E, labels, targets, grid, T, bound, None, None, mask, cand_cap,
                                 ge, total, counts, ws, ws_bytes, 0)


def test_argument_validation_happens_before_any_launch(lib):
    L = lib.lib()
    err = lambda: L.mmr_last_error()
    for null in ("q", "targets", "ge", "total", "counts", "ws", "gallery", "labels"):
        assert _call(L, **{null: None}) == -22 and b"null pointer" in err(), null
    assert _call(L, thr=None, T=3) == -22 and b"thresholds_host" in err()
    assert _call(L, thr=(0.1,), T=0) == -22 and b"T=0" in err()
    assert _call(L, thr=tuple(np.linspace(0, 1, 1025))) == -22 and b"T=1025" in err()
    assert _call(L, thr=tuple(np.linspace(0, 1, 1024)), ws_bytes=8) == -28                   # T = 1024 itself is accepted
    assert _call(L, thr=(0.3, 0.2)) == -22 and b"ascending" in err()
    assert _call(L, thr=(0.1, 0.2, 0.2)) == -22 and b"ascending" in err()
    assert _call(L, thr=(0.1, float("nan"), 0.3)) == -22 and b"finite" in err()
    assert _call(L, thr=(0.1, float("inf"))) == -22 and b"finite" in err()
    assert _call(L, E=100) == -95 and b"E=100" in err()
    assert _call(L, dtype=7) == -22 and b"dtype" in err()
    assert _call(L, Q=0) == -22 and b"Q=0" in err()
    assert _call(L, N=-1) == -22
    assert _call(L, cand_cap=0) == -22 and b"cand_cap" in err()
    assert _call(L, bound=float("inf")) == -22 and b"gallery_norm_bound" in err()
    assert _call(L, ws_bytes=8) == -28 and b"workspace" in err()
    assert _call(L, mask=18) == -22 and b"row_mask" in err()
    assert _call(L, q=24) == -22 and b"16-byte" in err()
    assert _call(L, labels=18) == -22 and b"4-byte" in err()
    assert L.mmr_version() == 1


def test_workspace_is_independent_of_n_for_bf16(lib):
    L = lib.lib()
    f = L.mmr_sweep_workspace_bytes
    base = f(1000, 512, 10, 200, 1 << 16, 1, 0)
    assert base > 0
    assert f(1_000_000, 512, 10, 200, 1 << 16, 1, 0) == base == f(0, 512, 10, 200, 1 << 16, 1, 1)
    # O(Q*T + cand_cap): the histogram and the candidate list, plus fixed scalars
    assert base <= 10 * 2 * 201 * 8 + (1 << 16) * 8 + 200 * 16 + 4096
    assert f(1000, 512, 20, 200, 1 << 16, 1, 0) > base and f(1000, 512, 10, 400, 1 << 16, 1, 0) > base
    assert f(1000, 512, 10, 200, 1 << 17, 1, 0) > base
    # fp32: a pre-split hi half keeps it independent of N, the split in the call adds the hi copy
    given = f(1000, 512, 10, 200, 1 << 16, 0, 1)
    assert f(1_000_000, 512, 10, 200, 1 << 16, 0, 1) == given
    assert f(1000, 512, 10, 200, 1 << 16, 0, 0) == given + 1000 * 512 * 2
    for bad in ((-1, 512, 10, 200, 8, 1, 0), (10, 512, 10, 0, 8, 1, 0), (10, 512, 10, 1025, 8, 1, 0), (10, 512, 10, 5, 0, 1, 0),
                (10, 512, 10, 5, 8, 3, 0)):
        assert f(*bad) == 0, bad


def _direct(tp, fp, pos):
    """The reference's rule, one (query, grid point) at a time."""
    Q, T = tp.shape
    P, R, F = np.zeros((Q, T)), np.zeros((Q, T)), np.zeros((Q, T))
    best = []
    for a in range(Q):
        best_f1, best_i = -1.0, 0
        for i in range(T):
            TP, FP = int(tp[a, i]), int(fp[a, i])
            FN = int(pos[a]) - TP
            p = TP / (TP + FP) if TP + FP > 0 else 0
            r = TP / (TP + FN) if TP + FN > 0 else 0
            f = 2 * p * r / (p + r) if p + r > 0 else 0
            P[a, i], R[a, i], F[a, i] = p, r, f
            if f > best_f1:
                best_f1, best_i = f, i
        best.append(best_i)
    return P, R, F, np.array(best)


def test_metrics_and_best_follow_the_reference_formulas():
    from mmr_amd.search import ThresholdSweep

    thr = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5], dtype=torch.float64)
    #            ordinary curve      tied best F1 (first wins)   no positives        nothing clears      all-zero columns
    tp = np.array([[50, 40, 30, 10, 0], [10, 10, 10, 10, 5], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [7, 7, 0, 0, 0]])
    fp = np.array([[900, 100, 10, 0, 0], [5, 5, 5, 5, 0], [30, 20, 10, 5, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
    pos = np.array([50, 10, 0, 12, 7])
    neg = np.array([950, 90, 100, 88, 93])
    ge = torch.from_numpy(np.stack([fp, tp], axis=1))
    total = torch.from_numpy(np.stack([neg, pos], axis=1))
    res = ThresholdSweep(thr, ge, total)
    assert torch.equal(res.tp, torch.from_numpy(tp)) and torch.equal(res.fp, torch.from_numpy(fp))
    assert torch.equal(res.fn, torch.from_numpy(pos[:, None] - tp)) and torch.equal(res.tn, torch.from_numpy(neg[:, None] - fp))
    P, R, F, best = _direct(tp, fp, pos)
    p, r, f1 = res.metrics()
    assert p.dtype == r.dtype == f1.dtype == np.float64
    assert np.array_equal(p, P) and np.array_equal(r, R) and np.array_equal(f1, F)
    b = res.best()
    assert np.array_equal(b["index"], best) and best.tolist() == [2, 0, 0, 0, 0]
    assert np.array_equal(b["threshold"], thr.numpy()[best])
    for key, m in (("f1", F), ("precision", P), ("recall", R)):
        assert np.array_equal(b[key], m[np.arange(5), best]), key
    # a 1-D query: every field loses the query axis
    one = ThresholdSweep(thr, ge[1:2], total[1:2], squeezed=True)
    assert tuple(one.tp.shape) == (5,) and one.pos.dim() == 0 and tuple(one.fn.shape) == (5,)
    assert np.array_equal(one.metrics()[2], F[1]) and int(one.best()["index"]) == 0 and one.best()["f1"] == F[1, 0]


def test_python_argument_errors_raise_before_any_launch():
    """The gallery is a meta tensor: nothing could be launched even if a check were missing."""
    from mmr_amd import search

    dev = torch.device("meta")
    q = torch.empty(3, 512, dtype=torch.bfloat16, device=dev)
    labels = torch.empty(100, dtype=torch.int32, device=dev)
    targets = torch.zeros(3, dtype=torch.int32)
    ok = [0.1, 0.2]
    check = lambda **kw: search._check_sweep_args(kw.get("q", q), 100, 512, kw.get("labels", labels), kw.get("targets", targets),
                                                  kw.get("thr", ok), dev)
    assert check().dtype == torch.float64 and check().tolist() == ok
    assert check(thr=np.linspace(0, 1, 1024)).shape[0] == 1024
    bad = [dict(q=torch.empty(3, 256, device=dev)), dict(labels=torch.empty(99, dtype=torch.int32, device=dev)),
           dict(labels=torch.empty(100, dtype=torch.float32, device=dev)), dict(labels=torch.empty(100, 1, dtype=torch.int32, device=dev)),
           dict(labels=torch.empty(100, dtype=torch.int32)), dict(labels=[0] * 100), dict(targets=torch.zeros(4, dtype=torch.int32)),
           dict(targets=torch.zeros(3)), dict(thr=[]), dict(thr=[[0.1, 0.2]]), dict(thr=[0.2, 0.1]), dict(thr=[0.1, 0.1]),
           dict(thr=[0.1, float("nan")]), dict(thr=[float("-inf"), 0.1]), dict(thr=np.linspace(0, 1, 1025)), dict(thr=[True, False])]
    for kw in bad:
        with pytest.raises(ValueError):
            check(**kw)
    with pytest.raises(ValueError):
        search._i32(torch.tensor([0, 2 ** 31]), "labels", "cpu")
    with pytest.raises(RuntimeError):                       # a CPU gallery: there is no CPU path
        search.threshold_sweep(torch.zeros(1, 512), torch.zeros(10, 512), torch.zeros(10, dtype=torch.int32),
                               torch.zeros(1, dtype=torch.int32), ok)
    import mmr_amd
    assert mmr_amd.threshold_sweep is search.threshold_sweep and mmr_amd.ThresholdSweep is search.ThresholdSweep
    assert hasattr(search.GalleryIndex, "threshold_sweep") and hasattr(search.GalleryIndex, "score_extent")
