"""The Tip-Adapter grid search without a GPU: the restatement of the reference's threshold search and metrics
(tip_grid_helpers) against results recorded from the reference's own functions (tests/golden/tip_grid_reference.npz,
written by tools/make_tip_grid_golden.py), the histogram formulation the kernel uses against the literal loop, with
controls that must fail, search_hp's list rule, the degenerate cases, the header and the argument checks."""
import os

import numpy as np
import pytest
import torch

import tip_grid_helpers as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tip_grid_reference.npz")


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def _cases():
    """Every (case, beta, alpha) of the GPU tests' first grid, from fp32 torch on the CPU: 5 cases x 12 points, whose
    26 classes make 312 (case, beta, alpha, class) threshold searches."""
    out = []
    for (N, S, C, E, dtype) in G.CASES:
        inp = G.make_inputs(N, S, C, E, dtype=dtype)
        betas, alphas = G.f32(G.GRID_BETAS), G.f32(G.GRID_ALPHAS)
        L0, cache = G.stage1(inp, betas, torch.float32)
        for b in range(len(betas)):
            for a in range(len(alphas)):
                out.append((G.grid_logits(L0, cache, alphas, b, a).numpy(), inp["labels"].numpy()))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def test_golden_parity_with_the_reference():
    z = np.load(GOLDEN)
    for k, (N, C, _, _) in enumerate(z["cases"].astype(int)):
        logits, labels = z[f"logits{k}"], z[f"labels{k}"]
        assert logits.dtype == np.float32 and logits.shape == (N, C)
        ours = G.threshold_table(logits, labels)
        counts = z[f"counts{k}"]
        for j, key in enumerate(("tp", "fp", "fn", "num_vals")):
            assert np.array_equal(ours[key], counts[:, j]), (k, key)
        assert np.array_equal(bits(ours["f1"]), bits(z[f"f1_{k}"])), k            # equal fp64 values
        assert np.array_equal(bits(ours["threshold"]), bits(z[f"threshold{k}"])), k
        assert (counts[:, 3] > 10).all() and (z[f"f1_{k}"] > 0).all()              # the golden cases are no degenerate ones
        conf = G.confusion(logits, labels)
        f1_ref, acc_ref, acc_ex_ref = z[f"cls{k}"]
        # cls_f1 runs in fp32 torch in the reference (tp / (tp + fp + 1e-6) and so on are fp32 operations, about six of
        # them in a row on values of order 1, then a mean and * 100): a few fp32 ulps of 100 is what fp32 allows
        assert abs(G.cls_f1(conf) - f1_ref) <= 16 * 2.0 ** -17
        assert G.cls_acc(conf) == acc_ref                                          # integer counts in Python floats: exact
        assert G.cls_acc(conf, exclude_class=C - 1) == acc_ex_ref


def test_histogram_formulation_equals_the_literal_loop(cases):
    n, lo_nv, hi_nv = 0, 10 ** 9, 0
    for logits, labels in cases:
        lit, hist = G.threshold_table(logits, labels), G.threshold_table(logits, labels, G.find_thresholds_hist)
        for key in ("tp", "fp", "fn", "num_vals"):
            assert np.array_equal(lit[key], hist[key]), key
        assert np.array_equal(bits(lit["f1"]), bits(hist["f1"]))
        assert np.array_equal(bits(lit["threshold"]), bits(hist["threshold"]))
        assert (lit["num_vals"] >= 100).all() and (lit["num_vals"] <= 400).all() and (lit["f1"] > 0).all()
        lo_nv, hi_nv = min(lo_nv, lit["num_vals"].min()), max(hi_nv, lit["num_vals"].max())
        n += logits.shape[1]
    print(f"num_vals between {lo_nv} and {hi_nv}")
    assert n == 312


def test_threshold_formula_is_numpy_linspace(cases):
    for logits, labels in cases[::5]:
        for c in range(logits.shape[1]):
            lo, hi, nv = G.extents(*G.get_similarity(logits, labels, c, logits.shape[1]))
            assert np.array_equal(bits(G.linspace_formula(lo, hi, nv)), bits(np.linspace(lo, hi, nv)))
    assert np.array_equal(bits(G.linspace_formula(-0.0, 0.15, 1)), bits(np.linspace(np.float64(-0.0), np.float64(0.15), 1)))
    t = np.linspace(np.float64(3.0), np.float64(3.0) + 1638.3, 16383)
    assert (np.diff(t) > 0).all()                                                  # non-decreasing up to the cap


def test_failing_controls(cases):
    """What the checks above would miss if they could: each wrong variant must change a result."""
    logits, labels = cases[0]
    C = logits.shape[1]
    pos, neg = G.get_similarity(logits, labels, 0, C)
    lo, hi, nv = G.extents(pos, neg)
    t0 = np.linspace(lo, hi, nv)[0]
    assert t0 == lo and (np.any(pos == lo) or np.any(neg == lo))                   # t_0 always equals an element
    f_ge, f_gt = G.eval_threshold(pos, neg, t0, ge=True), G.eval_threshold(pos, neg, t0, ge=False)
    assert f_ge[1:3] != f_gt[1:3]                                                  # `>` for `>=` changes the counts
    right = G.find_thresholds_hist(pos, neg, "right")
    changed = False
    for lg, lb in cases:
        for c in range(lg.shape[1]):
            p, n = G.get_similarity(lg, lb, c, lg.shape[1])
            a, b = G.find_thresholds_hist(p, n, "right"), G.find_thresholds_hist(p, n, "left")
            changed |= (a["tp"], a["fp"], a["f1"]) != (b["tp"], b["fp"], b["f1"])
    assert changed and right == G.find_thresholds(pos, neg)                        # side="left" changes them
    # a planted tie: 50 thresholds from 0 to 5 over pos = {0, 5, 5, 5}, neg = {0, 0, 0, 5}.  t_0 = 0 has tp 4, fp 4
    # (F1 2/3); every later one has tp 3, fp 1 and so the very same F1 0.75: the first of them must win
    pos_t, neg_t = np.array([0.0, 5.0, 5.0, 5.0]), np.array([0.0, 0.0, 0.0, 5.0])
    first, last = G.find_thresholds(pos_t, neg_t), G.find_thresholds(pos_t, neg_t, last_best=True)
    assert first["f1"] == last["f1"] and first["threshold"] < last["threshold"]    # the last best is another threshold
    assert G.find_thresholds_hist(pos_t, neg_t) == first


def test_degenerate_cases_in_the_restatement():
    zero = dict(f1=0.0, threshold=0.0, tp=0, fp=0, fn=0)
    for find in (G.find_thresholds, G.find_thresholds_hist):
        assert find([], [1.0, 2.0]) == dict(zero, num_vals=-1)                     # the reference raises: min of nothing
        assert find([1.0], []) == dict(zero, num_vals=-1)
        assert find([5.0, 6.0], [1.0, 2.0]) == dict(zero, num_vals=-30)            # hi = 2 < lo = 5: int(-3.0 * 10)
        assert find([1.0, 1.05], [1.0, 1.05]) == dict(zero, num_vals=0)            # int(0.5) == 0
        assert find([2.0, 2.0], [2.0]) == dict(zero, num_vals=0)
        one = find([0.0, 0.15], [-1.0, 0.15])                                      # num_vals == 1: the one threshold is lo
        assert one["num_vals"] == 1 and one["threshold"] == 0.0 and (one["tp"], one["fp"], one["fn"]) == (2, 1, 0)
        assert one["f1"] == ((2.0 * (2 / 3)) * 1.0) / (2 / 3 + 1.0)
    # rows with a label outside [0,C) are in neither pos nor neg nor the confusion matrix
    logits = np.array([[1.0, 0.0], [0.0, 1.0], [9.0, 9.0], [9.0, 9.0]], dtype=np.float32)
    labels = np.array([0, 1, -1, 2])
    pos, neg = G.get_similarity(logits, labels, 0, 2)
    assert pos.tolist() == [1.0] and neg.tolist() == [0.0]
    assert G.confusion(logits, labels).tolist() == [[1, 0], [0, 1]]
    assert G.confusion(np.array([[2.0, 2.0, 1.0]]), np.array([1])).tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 0]]   # lowest class


def test_search_hp_list_rule_and_pick():
    from mmr_amd import tip_adapter as ta
    cfg = G.RULE_CFG
    assert ta.search_lists(cfg) == G.rule_lists(cfg)
    betas, alphas = G.rule_lists(cfg)
    assert betas == pytest.approx([0.01, 1.41, 2.81, 4.21, 5.61], abs=1e-12) and betas[2] == 2 * 7 / 5 + 0.01 != 2.81
    assert alphas == pytest.approx([0.01, 0.76, 1.51, 2.26], abs=1e-12)
    # not on: the configured pair comes back and nothing is touched
    off = dict(cfg, search_hp=False)
    assert ta.search_hp(off, None, None, None, None, None) == (1.0, 2.0)
    # the pick: beta-major, first strictly greater, NaN never wins, (None, None, 0.0) when nothing beats 0
    table = [[0.1, 0.5, 0.5], [float("nan"), 0.5, 0.2]]
    assert G.pick(table) == (0, 1, 0.5)
    assert ta.pick_best(torch.tensor(table, dtype=torch.float64)) == (0, 1, 0.5)
    assert ta.pick_best(torch.zeros(2, 3, dtype=torch.float64)) == (None, None, 0.0) == G.pick(np.zeros((2, 3)))
    assert ta.pick_best(torch.full((1, 2), float("nan"), dtype=torch.float64)) == (None, None, 0.0)
    g = torch.Generator().manual_seed(0)
    for _ in range(20):
        s = torch.rand(4, 5, generator=g, dtype=torch.float64).round(decimals=1)   # coarse: ties are common
        assert ta.pick_best(s) == G.pick(s.tolist())


def _fake_grid(conf, f1):
    from mmr_amd import TipGrid
    conf, f1 = torch.as_tensor(conf, dtype=torch.int32), torch.as_tensor(f1, dtype=torch.float64)
    return TipGrid(None, None, None, None, conf, f1, None, None, None, None, None, 0)


def test_tipgrid_metrics_equal_the_restatement():
    rng = np.random.RandomState(3)
    conf = rng.randint(0, 40, size=(2, 3, 4, 4))
    conf[1, 2, 3] = 0                                                              # a class with no row
    f1 = rng.rand(2, 3, 4)
    grid = _fake_grid(conf, f1)
    m, acc, acc_ex, thr = grid.macro_f1(), grid.accuracy(), grid.accuracy(exclude_class=3), grid.threshold_f1([2, 0, 1])
    for b in range(2):
        for a in range(3):
            assert float(m[b, a]) == pytest.approx(G.cls_f1(conf[b, a]), rel=1e-14)
            assert float(acc[b, a]) == G.cls_acc(conf[b, a]) and float(acc_ex[b, a]) == G.cls_acc(conf[b, a], 3)
            assert float(thr[b, a]) == G.mean_f1(f1[b, a], [2, 0, 1])
    assert grid.best(classes=[2, 0, 1]) == G.pick([[G.mean_f1(f1[b, a], [2, 0, 1]) for a in range(3)] for b in range(2)])
    assert grid.best("macro_f1")[:2] == G.pick(m.tolist())[:2]
    assert float(_fake_grid(np.zeros((1, 1, 2, 2)), np.zeros((1, 1, 2))).accuracy()[0, 0]) == 0.0
    with pytest.raises(ValueError):
        grid.best("f2")
    with pytest.raises(RuntimeError, match="keep_cache"):
        grid.logits(0, 0)


def test_header_declares_the_grid_call_and_its_cap():
    import ctypes

    from mmr_amd import _header
    h = _header.load()
    p, i, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert h.constants["MMR_TIP_GRID_MAX_VALS"] == 16383           # num_vals + 1 bins of int32 = 64 KiB per histogram
    res, args, names = h.functions["mmr_tip_adapter_grid_workspace_bytes"]
    assert res is sz and args == [i64, i, i, i, i, i] and names == ["N", "E", "C", "S", "nb", "na"]
    res, args, names = h.functions["mmr_tip_adapter_grid"]
    assert res is i
    assert names == ["features", "labels", "dtype", "N", "E", "C", "S", "clip_weights_t", "keys_t", "keys_dtype",
                     "cache_values", "betas", "nb", "alphas", "na", "L0", "cache", "conf", "f1", "threshold", "tp", "fp", "fn",
                     "num_vals", "status", "workspace", "workspace_bytes", "stream"]
    assert args == [p, p, i, i64, i, i, i, p, p, i, p, p, i, p, i] + [p] * 11 + [sz, p]


def test_names_are_exported():
    import mmr_amd
    for name in ("tip_adapter_grid", "TipGrid", "search_hp"):
        assert name in mmr_amd.__all__ and getattr(mmr_amd, name) is getattr(mmr_amd.tip_adapter, name)


def test_arguments_are_checked_before_any_device_call():
    from mmr_amd import tip_adapter_grid
    E, S, C, N = 128, 12, 3, 5
    f, y = torch.zeros(N, E, dtype=torch.bfloat16), torch.zeros(N, dtype=torch.int64)
    w, k, v = torch.zeros(E, C, dtype=torch.bfloat16), torch.zeros(E, S, dtype=torch.bfloat16), torch.zeros(S, C)
    ok = dict(betas=[1.0], alphas=[1.0])
    for bad in (dict(features=f[:, :64]), dict(labels=y[:4]), dict(labels=y.int()), dict(clip_weights=w.float()),
                dict(cache_keys=k.half()), dict(cache_keys=k[:, :5]), dict(cache_values=v[:, :2]), dict(betas=[]),
                dict(alphas=[]), dict(beta_chunk=0), dict(adapter=torch.zeros(S, E, dtype=torch.bfloat16)),
                dict(adapter=torch.zeros(S + 1, E))):
        kw = dict(dict(features=f, labels=y, clip_weights=w, cache_keys=k, cache_values=v), **ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            tip_adapter_grid(kw.pop("features"), kw.pop("labels"), kw.pop("clip_weights"), kw.pop("cache_keys"),
                             kw.pop("cache_values"), kw.pop("betas"), kw.pop("alphas"), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        tip_adapter_grid(f, y, w, k, v, [1.0], [1.0])
    with pytest.raises(RuntimeError, match="GPU"):
        tip_adapter_grid(f, y, w, None, v, [1.0], [1.0], adapter=torch.zeros(S, E))
