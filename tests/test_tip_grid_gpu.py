"""mmr_tip_adapter_grid on the device (csrc/tip_grid.hip, tip_adapter.tip_adapter_grid / TipGrid / search_hp).

Stage 1 (L0, cache) is floating point and is held to the project's allowance for this arithmetic -- 8 x the deviation of
fp32 torch on the CPU from fp64, plus one fp32 ulp (tip_train_helpers.allowance).  Stage 2 is exact: every count, num_vals,
threshold and F1 must equal, as integers and as fp64 bit patterns, what the restatement of the reference's loops
(tip_grid_helpers) gives on the logits rebuilt with torch from the two returned tensors.  No case is skipped."""
import numpy as np
import pytest
import torch

import tip_grid_helpers as G
import tip_train_helpers as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = G.CASES + [(16, 16, 2, 128, torch.bfloat16), (1, 1, 1, 128, torch.bfloat16)]
GRIDS = {"grid": (G.GRID_BETAS, G.GRID_ALPHAS), "rule": G.rule_lists(G.RULE_CFG)}


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def to_dev(inp):
    return {k: v.to(DEV) for k, v in inp.items()}


def run(inp, betas, alphas, **kw):
    from mmr_amd import tip_adapter_grid
    d = to_dev(inp)
    keys = None if "adapter" in kw else d["cache_keys"]
    return tip_adapter_grid(d["features"], d["labels"], d["clip_weights"], keys, d["cache_values"], betas, alphas, **kw)


_RUNS, _WANT = {}, {}


def grid_of(case, which):
    """One device call per (case, grid), shared by the tests below and left unchanged."""
    key = (case, which)
    if key not in _RUNS:
        N, S, C, E, dtype = case
        inp = G.make_inputs(N, S, C, E, dtype=dtype)
        _RUNS[key] = (inp, run(inp, *GRIDS[which]))
    return _RUNS[key]


def want_of(case, which):
    """The restatement's results for grid_of(case, which), computed once."""
    key = (case, which)
    if key not in _WANT:
        inp, grid = grid_of(case, which)
        _WANT[key] = restated(grid, inp["labels"])
    return _WANT[key]


def restated(grid, labels):
    """The restatement on the logits torch rebuilds from the returned L0 and cache -> dict of arrays [nb,na,...]."""
    L0, cache, alphas = grid.L0.cpu(), grid.cache.cpu(), grid.alphas.cpu()
    labels = labels.numpy()
    nb, na = cache.shape[0], alphas.shape[0]
    out = {k: [] for k in ("conf", "f1", "threshold", "tp", "fp", "fn", "num_vals")}
    for b in range(nb):
        for a in range(na):
            logits = G.grid_logits(L0, cache, alphas, b, a).numpy()
            table = G.threshold_table(logits, labels)
            out["conf"].append(G.confusion(logits, labels))
            for k in table:
                out[k].append(table[k])
    C = L0.shape[1]
    return {k: np.array(v).reshape((nb, na) + ((C, C) if k == "conf" else (C,))) for k, v in out.items()}


def assert_stage2_equal(grid, want):
    for k in ("conf", "tp", "fp", "fn", "num_vals"):
        assert np.array_equal(getattr(grid, k).cpu().numpy(), want[k]), k
    assert np.array_equal(bits(grid.f1.cpu().numpy()), bits(want["f1"]))
    assert np.array_equal(bits(grid.threshold.cpu().numpy()), bits(want["threshold"]))


def assert_same_bits(g1, g2, cache=True):
    for k in ("L0", "conf", "f1", "threshold", "tp", "fp", "fn", "num_vals") + (("cache",) if cache else ()):
        a, b = getattr(g1, k).cpu().numpy(), getattr(g2, k).cpu().numpy()
        assert a.tobytes() == b.tobytes(), k
    assert g1.status == g2.status


# ------------------------------------------------------------------ 1. stage 1 against fp64
@pytest.mark.parametrize("case", G.CASES, ids=str)
def test_stage1_within_the_allowance_of_fp64(case):
    from mmr_amd import tip_adapter_logits
    inp, grid = grid_of(case, "grid")
    betas = G.f32(G.GRID_BETAS)
    L0_64, cache_64 = G.stage1(inp, betas, torch.float64)
    L0_32, cache_32 = G.stage1(inp, betas, torch.float32)
    for name, dev, r32, r64 in (("L0", grid.L0, L0_32, L0_64), ("cache", grid.cache, cache_32, cache_64)):
        err, allow = T.max_err(dev, r64), T.allowance(r32, r64)
        print(f"{case} {name}: error {err:.3e}, allowance {allow:.3e}, ratio {err / allow:.3f}")
        assert err <= allow
    assert torch.equal(grid.betas.cpu(), betas) and torch.equal(grid.alphas.cpu(), G.f32(G.GRID_ALPHAS))
    # the fused scoring call computes the same quantity its own way: the same allowance, not the same bits
    d = to_dev(inp)
    for b, a in ((0, 0), (1, 2), (2, 3)):
        beta, alpha = float(grid.betas[b]), float(grid.alphas[a])
        tip = tip_adapter_logits(d["features"], d["clip_weights"], d["cache_keys"], d["cache_values"], alpha, beta)
        t64 = L0_64 + cache_64[b] * alpha
        t32 = L0_32 + cache_32[b] * alpha
        allow = T.allowance(t32, t64)
        assert T.max_err(grid.logits(b, a), t64) <= allow and T.max_err(tip, t64) <= allow
        assert T.max_err(grid.logits(b, a), tip.double().cpu()) <= 2 * allow


# ------------------------------------------------------------------ 2. stage 2, exact
@pytest.mark.parametrize("which", sorted(GRIDS))
@pytest.mark.parametrize("case", CASES, ids=str)
def test_stage2_is_the_restatement_bit_for_bit(case, which):
    inp, grid = grid_of(case, which)
    want = want_of(case, which)
    assert_stage2_equal(grid, want)
    assert grid.status == 0
    C = case[2]
    if case in G.CASES:                                              # the recipe's classes are no degenerate ones
        nv = grid.num_vals.cpu().numpy()
        assert nv.min() >= 100 and nv.max() <= 400 and (grid.f1.cpu().numpy() > 0).all()
    # the metrics the host forms from the counts
    m, acc, acc_ex = grid.macro_f1(), grid.accuracy(), grid.accuracy(exclude_class=C - 1)
    for b in range(want["conf"].shape[0]):
        for a in range(want["conf"].shape[1]):
            assert float(m[b, a]) == pytest.approx(G.cls_f1(want["conf"][b, a]), rel=1e-14, abs=1e-300)
            assert float(acc[b, a]) == G.cls_acc(want["conf"][b, a])
            assert float(acc_ex[b, a]) == G.cls_acc(want["conf"][b, a], C - 1)


# ------------------------------------------------------------------ 3. best() and search_hp
@pytest.mark.parametrize("case", G.CASES[::2], ids=str)
def test_best_and_search_hp_equal_the_restatements_pick(case):
    from mmr_amd import search_hp
    inp, grid = grid_of(case, "rule")
    want = want_of(case, "rule")
    C = case[2]
    classes = list(range(C - 1))
    table = [[G.mean_f1(want["f1"][b, a], classes) for a in range(want["f1"].shape[1])] for b in range(want["f1"].shape[0])]
    b, a, score = G.pick(table)
    assert b is not None and grid.best(classes=classes) == (b, a, score)
    assert grid.best("macro_f1")[:2] == G.pick([[G.cls_f1(c) for c in row] for row in want["conf"]])[:2]
    d = to_dev(inp)
    betas, alphas = G.rule_lists(G.RULE_CFG)
    got = search_hp(G.RULE_CFG, d["cache_keys"], d["cache_values"], d["features"], d["labels"], d["clip_weights"])
    assert got == (betas[b], alphas[a])                              # the unrounded list values
    off = dict(G.RULE_CFG, search_hp=False)
    assert search_hp(off, d["cache_keys"], d["cache_values"], d["features"], d["labels"], d["clip_weights"]) == (1.0, 2.0)


def test_a_planted_exact_tie_goes_to_the_first_point():
    N, S, C, E, dtype = G.CASES[3]
    inp = G.make_inputs(N, S, C, E, dtype=dtype)
    betas, alphas = [2.34, 2.34, 0.01], [0.76, 1.51, 0.76]          # points (0,0), (0,2), (1,0), (1,2) are one and the same
    grid = run(inp, betas, alphas)
    scores = grid.threshold_f1()
    assert float(scores[0, 0]) == float(scores[0, 2]) == float(scores[1, 0]) == float(scores[1, 2])
    b, a, s = grid.best()
    assert (b, a, s) == G.pick(scores.tolist())
    tied = [(i, j) for i in range(3) for j in range(3) if float(scores[i, j]) == s]
    assert len(tied) >= 2 and (b, a) == tied[0]


# ------------------------------------------------------------------ 4. determinism
def test_calls_chunkings_and_prefilled_outputs_give_the_same_bits():
    from mmr_amd import _lib
    case = G.CASES[0]
    inp, first = grid_of(case, "grid")
    assert_same_bits(first, run(inp, *GRIDS["grid"]))
    assert_same_bits(first, run(inp, *GRIDS["grid"], beta_chunk=1))
    assert_same_bits(first, run(inp, *GRIDS["grid"], beta_chunk=2))
    lean = run(inp, *GRIDS["grid"], beta_chunk=1, keep_cache=False)
    assert lean.cache is None
    assert_same_bits(first, lean, cache=False)
    # the C ABI itself, its outputs and its workspace filled with zeros and then with 0xFF bytes
    N, S, C, E, dtype = case
    d = to_dev(inp)
    L = _lib.lib()
    f, y, v = d["features"], d["labels"], d["cache_values"]
    wct, kt = d["clip_weights"].t().contiguous(), d["cache_keys"].t().contiguous()
    betas, alphas = G.f32(G.GRID_BETAS).to(DEV), G.f32(G.GRID_ALPHAS).to(DEV)
    nb, na = len(betas), len(alphas)
    need = L.mmr_tip_adapter_grid_workspace_bytes(N, E, C, S, nb, na)
    results = []
    for fill in (0, 0xFF):
        ws = torch.full((max(need, 16),), fill, dtype=torch.uint8, device=DEV)
        sizes = dict(L0=N * C * 4, cache=nb * N * C * 4, conf=nb * na * C * C * 4, f1=nb * na * C * 8, threshold=nb * na * C * 8,
                     tp=nb * na * C * 4, fp=nb * na * C * 4, fn=nb * na * C * 4, num_vals=nb * na * C * 4)
        out = {k: torch.full((n,), fill, dtype=torch.uint8, device=DEV) for k, n in sizes.items()}
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        _lib.check(L.mmr_tip_adapter_grid(
            f.data_ptr(), y.data_ptr(), _lib.dtype_code(dtype), N, E, C, S, wct.data_ptr(), kt.data_ptr(), _lib.dtype_code(dtype),
            v.data_ptr(), betas.data_ptr(), nb, alphas.data_ptr(), na, *(out[k].data_ptr() for k in sizes), status.data_ptr(),
            ws.data_ptr(), ws.numel(), _lib.stream_ptr(torch.device(DEV))))
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        assert bool((ws == fill).all())                              # nothing strays into a workspace the call did not ask for
        results.append({k: t.cpu().numpy().tobytes() for k, t in out.items()})
    assert results[0] == results[1]
    for k in results[0]:
        assert results[0][k] == getattr(first, k).cpu().numpy().tobytes(), k


def test_long_caches_walk_s_in_chunks_with_the_same_chain():
    """S = 1100 > 1024 columns: two chunks of the cache kernel, the running sums resting in `cache` between them."""
    N, S, C, E = 19, 1100, 3, 128
    inp = G.make_inputs(N, S, C, E, dtype=torch.float16)
    betas = [0.01, 2.34, 7.01, 1.0, 5.5]                             # five: a full group of four betas and a tail
    alphas = [0.76, 3.01]
    grid = run(inp, betas, alphas)
    b32 = G.f32(betas)
    L0_64, cache_64 = G.stage1(inp, b32, torch.float64)
    L0_32, cache_32 = G.stage1(inp, b32, torch.float32)
    assert T.max_err(grid.L0, L0_64) <= T.allowance(L0_32, L0_64)
    assert T.max_err(grid.cache, cache_64) <= T.allowance(cache_32, cache_64)
    assert_stage2_equal(grid, restated(grid, inp["labels"]))
    assert_same_bits(grid, run(inp, betas, alphas, beta_chunk=3))


# ------------------------------------------------------------------ 5. the adapter path
def test_adapter_path_equals_its_weight_passed_as_keys():
    from mmr_amd import TipAdapterF
    N, S, C, E, dtype = G.CASES[0]
    inp = G.make_inputs(N, S, C, E, dtype=dtype)
    d = to_dev(inp)
    t = TipAdapterF(d["cache_keys"], d["cache_values"], d["clip_weights"], 1.0, 5.5, lr=1e-3, total_steps=2)
    t.step(d["features"][:64], d["labels"][:64])
    t.step(d["features"][64:128], d["labels"][64:128])
    assert not torch.equal(t.weight, d["cache_keys"].t().float())     # it did train
    by_adapter = run(inp, *GRIDS["grid"], adapter=t)
    by_weight = run(inp, *GRIDS["grid"], adapter=t.weight.clone())
    assert_same_bits(by_adapter, by_weight)
    assert_stage2_equal(by_adapter, restated(by_adapter, inp["labels"]))
    L0_64, cache_64 = G.stage1(inp, G.f32(G.GRID_BETAS), torch.float64, keys_t=t.weight.cpu())
    L0_32, cache_32 = G.stage1(inp, G.f32(G.GRID_BETAS), torch.float32, keys_t=t.weight.cpu())
    assert T.max_err(by_adapter.cache, cache_64) <= T.allowance(cache_32, cache_64)
    # fp32 keys in an fp32 problem are the same kernel either way
    inp32 = G.make_inputs(N, S, C, E, dtype=torch.float32)
    assert_same_bits(run(inp32, *GRIDS["grid"]), run(inp32, *GRIDS["grid"], adapter=inp32["cache_keys"].t().contiguous()))
    beta, alpha = t.search_hp(G.RULE_CFG, d["features"], d["labels"])
    betas, alphas = G.rule_lists(G.RULE_CFG)
    assert beta in betas and alpha in alphas


# ------------------------------------------------------------------ 6. edges
def test_a_class_without_positives_and_labels_out_of_range():
    N, S, C, E, dtype = G.CASES[3]
    inp = G.make_inputs(N, S, C, E, dtype=dtype)
    labels = inp["labels"].clone()
    labels[labels == 2] = 0                                          # class 2 has no positive row
    labels[3], labels[7] = -1, C                                     # two rows that take no part
    inp = dict(inp, labels=labels)
    grid = run(inp, *GRIDS["grid"])
    assert grid.status == 1
    nv, f1 = grid.num_vals.cpu().numpy(), grid.f1.cpu().numpy()
    assert (nv[:, :, 2] == -1).all() and (f1[:, :, 2] == 0).all() and (grid.tp.cpu().numpy()[:, :, 2] == 0).all()
    assert (nv[:, :, [0, 1, 3, 4]] > 0).all()
    conf = grid.conf.cpu().numpy()
    assert (conf.sum(axis=(2, 3)) == N - 2).all() and (conf[:, :, 2].sum(axis=-1) == 0).all()
    assert_stage2_equal(grid, restated(grid, labels))
    # without the two rows the counts are the same
    keep = torch.tensor([i for i in range(N) if i not in (3, 7)])
    sub = dict(inp, features=inp["features"][keep], labels=labels[keep])
    small = run(sub, *GRIDS["grid"])
    assert small.status == 0
    for k in ("conf", "tp", "fp", "fn", "num_vals"):
        assert torch.equal(getattr(small, k), getattr(grid, k)), k
    assert torch.equal(small.f1, grid.f1) and torch.equal(small.threshold, grid.threshold)


def test_a_constant_column_has_no_thresholds():
    N, S, C, E, dtype = G.CASES[3]
    inp = G.make_inputs(N, S, C, E, dtype=dtype)
    w = inp["clip_weights"].clone()
    w[:, 1] = 0                                                      # L0[:, 1] = 0 for every row ...
    v = inp["cache_values"].clone()
    v[:, 1] = 0                                                      # ... and so is the cache term of class 1
    w[:, 4] = w[:, 3]                                                # equal classifier rows, equal value columns: an exact
    v[:, 4] = v[:, 3]                                                # tie of classes 3 and 4 in every row
    inp = dict(inp, clip_weights=w, cache_values=v)
    grid = run(inp, *GRIDS["grid"])
    assert (grid.num_vals[:, :, 1] == 0).all() and (grid.f1[:, :, 1] == 0).all() and (grid.threshold[:, :, 1] == 0).all()
    assert (grid.conf[:, :, :, 4] == 0).all()                        # the lowest class at the maximum: 4 never beats 3
    assert_stage2_equal(grid, restated(grid, inp["labels"]))


def test_a_single_row_key_and_class():
    inp, grid = grid_of((1, 1, 1, 128, torch.bfloat16), "grid")
    assert (grid.num_vals == -1).all() and (grid.f1 == 0).all() and (grid.conf == 1).all() and grid.status == 0
    assert float(grid.accuracy()[0, 0]) == 100.0


def test_num_vals_past_the_cap_raises_and_names_the_point():
    from mmr_amd import _lib
    cap = _lib.HEADER.constants["MMR_TIP_GRID_MAX_VALS"]
    N, S, C, E, dtype = G.CASES[3]
    inp = G.make_inputs(N, S, C, E, dtype=dtype)
    big = dict(inp, cache_values=inp["cache_values"] * 100000.0)
    ok = run(big, [0.01], [0.01])                                    # alpha 0.01: the spread stays small
    assert ok.status == 0 and int(ok.num_vals.max()) <= cap
    with pytest.raises(RuntimeError, match=r"b=0, a=1.*num_vals = \d+ thresholds exceed the cap of 16383"):
        run(big, [0.01], [0.01, 3.01])
