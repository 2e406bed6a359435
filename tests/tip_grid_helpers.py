"""Shared by test_tip_grid_host.py and test_tip_grid_gpu.py (not a test module): the reference's threshold search
(`get_similarity` + `find_thresholds` + `eval_threshold`, code/main_custom.py:27-105), its confusion matrix, `cls_f1` and
`cls_acc` (code/utils.py:15-76) and the pick of `search_hp` (code/utils.py:159-206), restated in numpy on fp64 values.

The contract (include/mmr.h, mmr_tip_adapter_grid): the logits of a grid point are fp32, widened to fp64 before anything
is compared; thresholds are np.linspace in fp64; an F1 of 0/0 is NaN and never wins; the first threshold whose F1 is
strictly above every earlier one (from 0.0) wins.  Degenerate classes -- pos or neg empty (num_vals = -1), hi < lo, or
num_vals == 0 -- have f1 = threshold = 0 and zero counts, where the reference raises or returns 0.
"""
import warnings

import numpy as np
import torch

import tip_train_helpers as T

GRID_BETAS = [0.01, 2.34, 7.01]
GRID_ALPHAS = [0.01, 0.76, 1.51, 3.01]
RULE_CFG = dict(search_hp=True, search_scale=[7, 3], search_step=[5, 4], init_beta=1.0, init_alpha=2.0)
# (N, S, C, E, dtype) of the non-degenerate cases: 26 classes in all
CASES = [(257, 96, 6, 512, torch.bfloat16), (257, 96, 6, 512, torch.float16), (257, 96, 6, 512, torch.float32),
         (33, 33, 5, 128, torch.float16), (300, 130, 3, 256, torch.float32)]


def make_inputs(N, S, C, E, dtype=torch.bfloat16, seed=1):
    """tip_train_helpers.make_inputs under the grid's names."""
    inp = T.make_inputs(N, S, C, E, dtype=dtype, seed=seed)
    return dict(features=inp["features"], labels=inp["targets"], clip_weights=inp["clip_weights"],
                cache_keys=inp["cache_keys"].to(dtype), cache_values=inp["cache_values"])


def rule_lists(cfg):
    """code/utils.py:163-164."""
    return ([i * (cfg["search_scale"][0] - 0) / cfg["search_step"][0] + 0.01 for i in range(cfg["search_step"][0])],
            [i * (cfg["search_scale"][1] - 0) / cfg["search_step"][1] + 0.01 for i in range(cfg["search_step"][1])])


def f32(values):
    return torch.tensor(values, dtype=torch.float64).to(torch.float32)


# ------------------------------------------------------------------ stage 1 on the CPU, in a dtype of choice
def stage1(inp, betas, dtype, keys_t=None):
    """-> L0 [N,C], cache [nb,N,C] in `dtype` (fp64: the truth; fp32: what sizes the allowance)."""
    F = inp["features"].to(dtype)
    Wc = inp["clip_weights"].to(dtype)
    K = (inp["cache_keys"].to(dtype) if keys_t is None else keys_t.to(dtype).t())
    V = inp["cache_values"].to(dtype)
    L0 = 100.0 * (F @ Wc)
    A = F @ K
    cache = torch.stack([torch.exp(float(b) * A - float(b)) @ V * 10.0 for b in betas.to(dtype)])
    return L0, cache


def grid_logits(L0, cache, alphas, b, a):
    """The contract's logits of point (b, a) from the two returned fp32 tensors: one rounded multiply, one rounded add."""
    assert L0.dtype == torch.float32 and cache.dtype == torch.float32 and alphas.dtype == torch.float32
    return L0 + cache[b] * alphas[a]


# ------------------------------------------------------------------ the threshold search, as the literal loop
def linspace_formula(lo, hi, n):
    """np.linspace(lo, hi, n) in fp64, spelled out: what the kernel evaluates."""
    lo, hi = np.float64(lo), np.float64(hi)
    if n == 1:
        return np.array([np.float64(0.0) + lo])
    step = (hi - lo) / np.float64(n - 1)
    t = np.array([np.float64(i) * step + lo for i in range(n)], dtype=np.float64)
    t[-1] = hi
    return t


def eval_threshold(pos, neg, t, ge=True):
    tp = int(np.sum(pos >= t)) if ge else int(np.sum(pos > t))
    fp = int(np.sum(neg >= t)) if ge else int(np.sum(neg > t))
    fn = len(pos) - tp
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore")
        p = np.float64(tp) / np.float64(tp + fp)
        r = np.float64(tp) / np.float64(tp + fn)
        f1 = ((np.float64(2.0) * p) * r) / (p + r)
    return f1, tp, fp, fn


def extents(pos, neg):
    """-> lo, hi, num_vals (-1: pos or neg empty)."""
    if len(pos) == 0 or len(neg) == 0:
        return 0.0, 0.0, -1
    lo = max(np.min(pos), np.min(neg))
    hi = min(np.max(pos), np.max(neg))
    return lo, hi, int((hi - lo) * 10)


def find_thresholds(pos, neg, ge=True, last_best=False):
    """-> dict(f1, threshold, tp, fp, fn, num_vals).  `pos`, `neg`: fp64 arrays.  ge / last_best: the failing controls."""
    pos, neg = np.asarray(pos, dtype=np.float64), np.asarray(neg, dtype=np.float64)
    lo, hi, nv = extents(pos, neg)
    best = dict(f1=0.0, threshold=0.0, tp=0, fp=0, fn=0, num_vals=nv)
    if nv <= 0:
        return best
    for t in np.linspace(lo, hi, nv):
        f1, tp, fp, fn = eval_threshold(pos, neg, t, ge)
        if f1 > best["f1"] or (last_best and f1 == best["f1"] and f1 > 0):
            best.update(f1=float(f1), threshold=float(t), tp=tp, fp=fp, fn=fn)
    return best


def find_thresholds_hist(pos, neg, side="right"):
    """The kernel's formulation: bin = searchsorted(t, x, "right") = #{i : t_i <= x}, a bincount and a suffix sum."""
    pos, neg = np.asarray(pos, dtype=np.float64), np.asarray(neg, dtype=np.float64)
    lo, hi, nv = extents(pos, neg)
    best = dict(f1=0.0, threshold=0.0, tp=0, fp=0, fn=0, num_vals=nv)
    if nv <= 0:
        return best
    t = np.linspace(lo, hi, nv)
    hp = np.bincount(np.searchsorted(t, pos, side), minlength=nv + 1)
    hn = np.bincount(np.searchsorted(t, neg, side), minlength=nv + 1)
    tp = np.cumsum(hp[::-1])[::-1][1:]                # tp_i = #{bin > i}
    fp = np.cumsum(hn[::-1])[::-1][1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        p = tp / (tp + fp).astype(np.float64)
        r = tp / np.float64(len(pos))
        f1 = ((2.0 * p) * r) / (p + r)
    f1 = np.where(np.isnan(f1), -np.inf, f1)
    i = int(np.argmax(f1))                            # the first index at the maximum
    if f1[i] > 0:
        best.update(f1=float(f1[i]), threshold=float(t[i]), tp=int(tp[i]), fp=int(fp[i]), fn=len(pos) - int(tp[i]))
    return best


def get_similarity(logits, labels, c, C):
    """Column c of the rows labelled c, and of the other rows with a label in [0,C); fp64."""
    x = np.asarray(logits, dtype=np.float64)[:, c]
    labels = np.asarray(labels)
    valid = (labels >= 0) & (labels < C)
    return x[valid & (labels == c)], x[valid & (labels != c)]


def threshold_table(logits, labels, find=find_thresholds):
    """find_thresholds of every class -> dict of arrays [C]."""
    C = logits.shape[1]
    rows = [find(*get_similarity(logits, labels, c, C)) for c in range(C)]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


# ------------------------------------------------------------------ confusion matrix, cls_f1, cls_acc
def confusion(logits, labels):
    """[target, pred] int64; pred = the lowest class at the row maximum; labels outside [0,C) are left out."""
    x = np.asarray(logits, dtype=np.float64)
    labels = np.asarray(labels)
    C = x.shape[1]
    pred = np.argmax(x == x.max(axis=1, keepdims=True), axis=1)
    conf = np.zeros((C, C), dtype=np.int64)
    for t, p in zip(labels, pred):
        if 0 <= t < C:
            conf[t, p] += 1
    return conf


def cls_f1(conf):
    conf = np.asarray(conf, dtype=np.float64)
    tp = np.diag(conf)
    fp, fn = conf.sum(axis=0) - tp, conf.sum(axis=1) - tp
    eps = 1e-6
    precision, recall = tp / (tp + fp + eps), tp / (tp + fn + eps)
    return float((2 * (precision * recall) / (precision + recall + eps)).mean() * 100)


def cls_acc(conf, exclude_class=None):
    conf = np.asarray(conf, dtype=np.float64)
    keep = np.array([t != exclude_class for t in range(conf.shape[0])])
    valid = conf[keep].sum()
    return 0.0 if valid == 0 else float(100 * np.diag(conf)[keep].sum() / valid)


# ------------------------------------------------------------------ search_hp's pick
def pick(scores):
    """scores [nb][na] in beta-major order -> (b, a, score): the first strictly greater than all before, from 0.0."""
    best, bb, ba = 0.0, None, None
    for b, row in enumerate(scores):
        for a, s in enumerate(row):
            if s > best:
                best, bb, ba = float(s), b, a
    return bb, ba, best


def mean_f1(f1_row, classes):
    """The reference's `f1 += ...; f1 = f1 / 5.` over the listed classes, in list order."""
    f1 = 0.0
    for c in classes:
        f1 += float(f1_row[c])
    return f1 / float(len(classes))
