"""GPU parity: the labelled threshold sweep (threshold_sweep / GalleryIndex.threshold_sweep / mmr_threshold_sweep)
against the brute-force fp64 oracle of tests/sweep_helpers.py.  Every count must equal the oracle's exactly."""
import numpy as np
import pytest
import torch

import sweep_helpers as H
from mmr_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S(device):
    from mmr_amd import search
    return search


@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


def _grids(s):
    """The reference's two grids: 200 points over [min score, max score] and a 1e-3 step."""
    return {"linspace200": np.linspace(float(s.min()), float(s.max()), 200), "step1e-3": np.arange(-0.2, 0.6005, 0.001)}


def _raw_sweep(device, q, g, labels, targets, thr, cand_cap, fill=0xFF, mask_words=None, hi=None, resid=None):
    """mmr_threshold_sweep through the C ABI with the workspace and outputs pre-filled with `fill` bytes.
    -> (ge, total, counts) device tensors"""
    from mmr_amd import _lib
    L = _lib.lib()
    Q, E = q.shape
    N = g.shape[0]
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    T = thr.shape[0]
    need = L.mmr_sweep_workspace_bytes(N, E, Q, T, cand_cap, _lib.dtype_code(g.dtype), int(hi is not None))
    assert need > 0
    ws = torch.full((need,), fill, dtype=torch.uint8, device=device)
    outs = [torch.full((n,), fill, dtype=torch.uint8, device=device).view(torch.int64) for n in (Q * 2 * T * 8, Q * 2 * 8, 16)]
    _lib.check(L.mmr_threshold_sweep(q.data_ptr(), g.data_ptr(), _lib.ptr(hi), _lib.dtype_code(g.dtype), Q, N, E,
                                     labels.data_ptr(), targets.data_ptr(), thr.ctypes.data, T, 0.0, None, _lib.ptr(resid),
                                     _lib.ptr(mask_words), cand_cap, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                     ws.data_ptr(), need, _lib.stream_ptr(device)))
    torch.cuda.synchronize(device)
    return outs[0].view(Q, 2, T), outs[1].view(Q, 2), outs[2]


# ------------------------------------------------------------------ 1. parity grid
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("E", [128, 512, 768])
@pytest.mark.parametrize("Q", [1, 7, 70])
@pytest.mark.parametrize("N", [1000, 10007])
def test_parity_grid(S, ref, device, N, Q, E, dtype):
    gal, labels, centres = H.labelled_gallery(N, E, seed=N + E, dtype=dtype)
    q, targets = H.labelled_queries(Q, E, centres, seed=Q + E, dtype=dtype)
    gf, qf = H.f32(gal), H.f32(q)
    s = qf.astype(np.float64) @ gf.astype(np.float64).T
    gd, qd, ld, td = gal.to(device), q.to(device), labels.to(device), targets.to(device)
    index = S.GalleryIndex(gd) if N > 1000 else None
    for name, thr in _grids(s).items():
        want_ge, want_total, redecided = H.oracle_sweep(ref, qf, gf, labels.numpy(), targets.numpy(), thr)
        res = S.threshold_sweep(qd, gd, ld, td, thr) if index is None else index.threshold_sweep(qd, ld, td, thr)
        done, cands = res.counts
        print(f"{name}: oracle re-decided {redecided} pairs; candidates {cands} of {Q * N} pairs")
        H.check_sweep(res, want_ge, want_total)
        assert np.array_equal(res.thresholds.cpu().numpy(), thr)
        assert done == cands > 0, (name, res.counts)             # the ambiguous path ran ...
        if dtype == torch.bfloat16:
            assert cands < Q * N, (name, res.counts)             # ... and so did the decided one
        if Q > H.NCLASS:                                         # the target no row carries
            assert int(res.pos[-1]) == 0 and int(res.tp[-1].sum()) == 0 and int(res.neg[-1]) == N
        assert np.array_equal((res.tp + res.fn).cpu().numpy(), np.broadcast_to(want_total[:, 1:2], (Q, len(thr))))
        assert np.array_equal((res.fp + res.tn).cpu().numpy(), np.broadcast_to(want_total[:, 0:1], (Q, len(thr))))


def test_one_dimensional_query_and_int64_labels(S, ref, device):
    gal, labels, centres = H.labelled_gallery(3000, 256, seed=9, dtype=torch.bfloat16)
    thr = np.linspace(-0.1, 0.3, 50)
    want_ge, want_total, _ = H.oracle_sweep(ref, H.f32(centres[2:3].bfloat16()), H.f32(gal), labels.numpy(), np.array([2]), thr)
    res = S.threshold_sweep(centres[2].bfloat16().to(device), gal.to(device), labels.long().to(device), [2], torch.from_numpy(thr))
    assert tuple(res.tp.shape) == (50,) and res.pos.dim() == 0
    assert np.array_equal(res.tp.cpu().numpy(), want_ge[0, 1]) and np.array_equal(res.fp.cpu().numpy(), want_ge[0, 0])
    assert int(res.pos) == want_total[0, 1] and int(res.neg) == want_total[0, 0]
    p, r, f1 = res.metrics()
    assert p.shape == r.shape == f1.shape == (50,)
    best = res.best()
    assert f1[best["index"]] == f1.max() == best["f1"] and best["threshold"] == thr[best["index"]]


# ------------------------------------------------------------------ 2. thresholds on the data
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_thresholds_that_sit_on_exact_dots(S, ref, device, dtype):
    N, Q, E = 6000, 5, 512
    gal, labels, centres = H.labelled_gallery(N, E, seed=77, dtype=dtype)
    q, targets = H.labelled_queries(Q, E, centres, seed=78, dtype=dtype)
    gd, qd = gal.to(device), q.to(device)
    _, idx, d64 = S.cosine_topk(qd, gd, k=10, return_dot64=True)
    d = d64.cpu().numpy().reshape(-1)                                        # the exact dots of 50 pairs
    thr = np.unique(np.concatenate([d, np.nextafter(d, np.inf), np.nextafter(d, -np.inf)]))
    assert 50 <= thr.shape[0] <= 150
    gf, qf = H.f32(gal), H.f32(q)
    want_ge, want_total, redecided = H.oracle_sweep(ref, qf, gf, labels.numpy(), targets.numpy(), thr)
    assert redecided >= 50
    res = S.threshold_sweep(qd, gd, labels.to(device), targets.to(device), thr)
    H.check_sweep(res, want_ge, want_total)
    # a pair that ties a threshold counts for it and not for the next one up
    both = (res.tp + res.fp).cpu().numpy()
    idx = idx.cpu().numpy()
    for a in range(Q):
        for j in range(10):
            dv = H.dot64(ref, qf[a], gf[idx[a, j]])
            i = int(np.searchsorted(thr, dv))
            assert thr[i] == dv and thr[i + 1] == np.nextafter(dv, np.inf)
            ties = int((d64[a].cpu().numpy() == dv).sum())
            assert both[a, i] - both[a, i + 1] >= ties >= 1


# ------------------------------------------------------------------ 3. agreement with range search at scale
@pytest.mark.slow
def test_agrees_with_range_search_on_a_million_rows(S, device):
    N, Q, E = 1_000_000, 10, 512
    gen = torch.Generator(device=device).manual_seed(5)
    centres = synth.synth_unit_rows(H.NCLASS, E, seed=5).to(device)
    labels = torch.randint(0, H.NCLASS, (N,), generator=gen, device=device, dtype=torch.int32)
    gal = torch.empty(N, E, dtype=torch.bfloat16, device=device)
    for s0 in range(0, N, 1 << 17):
        x = torch.randn(min(1 << 17, N - s0), E, generator=gen, device=device)
        x = 0.12 * centres[labels[s0:s0 + x.shape[0]].long()] + x / x.norm(dim=-1, keepdim=True)
        gal[s0:s0 + x.shape[0]] = (x / x.norm(dim=-1, keepdim=True)).bfloat16()
    q = torch.cat([centres, synth.synth_unit_rows(Q - H.NCLASS, E, seed=6).to(device)]).bfloat16()
    targets = (torch.arange(Q, dtype=torch.int32) % H.NCLASS).to(device)
    index = S.GalleryIndex(gal)
    lo, hi = index.score_extent(q)
    thr = np.linspace(float(lo.min()), float(hi.max()), 200)
    res = index.threshold_sweep(q, labels, targets, thr)
    again = index.threshold_sweep(q, labels, targets, thr)
    for a, b in ((res.tp, again.tp), (res.fp, again.fp), (res.pos, again.pos), (res.neg, again.neg)):
        assert torch.equal(a, b)                                             # two runs are bit-identical
    tp, fp = res.tp.cpu().numpy(), res.fp.cpu().numpy()
    assert np.all(np.diff(tp, axis=1) <= 0) and np.all(np.diff(fp, axis=1) <= 0)
    assert np.all(tp <= res.pos.cpu().numpy()[:, None]) and np.all(fp <= res.neg.cpu().numpy()[:, None])
    assert np.array_equal((res.pos + res.neg).cpu().numpy(), np.full(Q, N))
    assert int(tp[int(lo.argmin()), 0] + fp[int(lo.argmin()), 0]) == N          # the lowest point is that query's minimum: all rows
    assert int(tp[int(hi.argmax()), -1] + fp[int(hi.argmax()), -1]) >= 1        # the highest is a maximum: its row ties it
    for i in (120, 150, 199):
        offsets, rows, _ = index.range_search(q, float(thr[i]))
        offsets = offsets.cpu().numpy()
        assert np.array_equal(np.diff(offsets), tp[:, i] + fp[:, i]), i
        qid = torch.repeat_interleave(torch.arange(Q, device=device), torch.from_numpy(np.diff(offsets)).to(device))
        hit = (labels[rows] == targets[qid]).long()
        assert np.array_equal(torch.bincount(qid, weights=hit, minlength=Q).long().cpu().numpy(), tp[:, i]), i


# ------------------------------------------------------------------ 4. row masks and deletions
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_row_masks_and_deletions_equal_the_compacted_gallery(S, ref, device, dtype):
    N, Q, E = 5003, 9, 512
    gal, labels, centres = H.labelled_gallery(N, E, seed=21, dtype=dtype)
    q, targets = H.labelled_queries(Q, E, centres, seed=22, dtype=dtype)
    gf, qf = H.f32(gal), H.f32(q)
    thr = np.linspace(-0.15, 0.3, 120)
    gd, qd, ld, td = gal.to(device), q.to(device), labels.to(device), targets.to(device)
    rng = np.random.default_rng(3)
    few = np.zeros(N, dtype=bool)
    few[rng.choice(N, 19, replace=False)] = True
    masks = {"half": rng.random(N) < 0.5, "all ones": np.ones(N, dtype=bool), "fewer than 32 live rows": few}
    plain = S.threshold_sweep(qd, gd, ld, td, thr)
    for name, m in masks.items():
        want_ge, want_total, _ = H.oracle_sweep(ref, qf, gf[m], labels.numpy()[m], targets.numpy(), thr)
        md = torch.from_numpy(m).to(device)
        res = S.threshold_sweep(qd, gd, ld, td, thr, row_mask=md)
        H.check_sweep(res, want_ge, want_total)
        compact = S.threshold_sweep(qd, gd[md].contiguous(), ld[md].contiguous(), td, thr)       # the statement itself
        assert torch.equal(res.tp, compact.tp) and torch.equal(res.fp, compact.fp)
        assert torch.equal(res.pos, compact.pos) and torch.equal(res.neg, compact.neg)
        if name == "all ones":
            assert torch.equal(res.tp, plain.tp) and torch.equal(res.fp, plain.fp)
    # deletions, then deletions AND a mask
    index = S.GalleryIndex(gd)
    gone = rng.choice(N, 700, replace=False)
    index.delete_rows(torch.from_numpy(gone))
    live = np.ones(N, dtype=bool)
    live[gone] = False
    want_ge, want_total, _ = H.oracle_sweep(ref, qf, gf[live], labels.numpy()[live], targets.numpy(), thr)
    H.check_sweep(index.threshold_sweep(qd, ld, td, thr), want_ge, want_total)
    both = live & masks["half"]
    want_ge, want_total, _ = H.oracle_sweep(ref, qf, gf[both], labels.numpy()[both], targets.numpy(), thr)
    H.check_sweep(index.threshold_sweep(qd, ld, td, thr, row_mask=torch.from_numpy(masks["half"]).to(device)), want_ge, want_total)


# ------------------------------------------------------------------ 5. non-finite and extreme inputs
def _edge_data(dtype, N=2500, Q=6, E=512):
    gal, labels, centres = H.labelled_gallery(N, E, seed=31, dtype=torch.float32)
    q, targets = H.labelled_queries(Q, E, centres, seed=32, dtype=torch.float32)
    return gal, labels, q, targets


def _sweep_vs_oracle(S, ref, device, gal, labels, q, targets, thr, dtype, **kw):
    gal, q = gal.to(dtype), q.to(dtype)
    want_ge, want_total, _ = H.oracle_sweep(ref, H.f32(q), H.f32(gal), labels.numpy(), targets.numpy(), thr)
    res = S.threshold_sweep(q.to(device), gal.to(device), labels.to(device), targets.to(device), thr, **kw)
    H.check_sweep(res, want_ge, want_total)
    return res, want_ge, want_total


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_nan_rows_and_a_nan_query(S, ref, device, dtype):
    gal, labels, q, targets = _edge_data(dtype)
    N = gal.shape[0]
    thr = np.linspace(-0.15, 0.3, 64)
    nan_rows = [0, 31, 32, 1000, N - 1]
    gal[nan_rows, 5] = float("nan")
    res, _, want_total = _sweep_vs_oracle(S, ref, device, gal, labels, q, targets, thr, dtype)
    assert np.array_equal(want_total.sum(1), np.full(q.shape[0], N - len(nan_rows)))       # absent from total too
    q[2, 7] = float("nan")
    res, _, want_total = _sweep_vs_oracle(S, ref, device, gal, labels, q, targets, thr, dtype)
    assert int(res.tp[2].sum()) == 0 and int(res.fp[2].sum()) == 0 and int(res.pos[2]) == 0 and int(res.neg[2]) == 0
    assert int(res.pos[1] + res.neg[1]) == N - len(nan_rows)                              # its neighbours are unaffected


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_infinite_elements(S, ref, device, dtype):
    gal, labels, q, targets = _edge_data(dtype)
    N = gal.shape[0]
    thr = np.linspace(-0.15, 0.3, 64)
    gal[10, 3] = float("inf")
    gal[2000, 4] = float("-inf")
    res, want_ge, want_total = _sweep_vs_oracle(S, ref, device, gal, labels, q, targets, thr, dtype)
    qf = H.f32(q.to(dtype))
    assert np.all(qf[:, 3] != 0) and np.all(qf[:, 4] != 0)      # so both rows' dots are +-inf, never NaN
    assert np.array_equal(want_total.sum(1), np.full(q.shape[0], N))                       # +-inf dots count in total
    both = (res.tp + res.fp).cpu().numpy()
    plus = (qf[:, 3] > 0).astype(np.int64) + (qf[:, 4] < 0)     # rows whose dot is +inf: they clear every threshold ...
    assert np.all(both[:, -1] >= plus) and np.all(both[:, 0] <= N - (2 - plus))            # ... and -inf clears none


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_zero_query_ties_a_threshold_at_zero(S, ref, device, dtype):
    gal, labels, q, targets = _edge_data(dtype)
    N = gal.shape[0]
    q[1] = 0.0
    thr = np.array([-0.1, 0.0, np.nextafter(0.0, 1.0), 0.1])
    res, _, _ = _sweep_vs_oracle(S, ref, device, gal, labels, q, targets, thr, dtype)
    both = (res.tp + res.fp)[1].cpu().numpy()
    assert both.tolist() == [N, N, 0, 0]            # every row ties 0.0 exactly: all count there, none above


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("eg,eq", [(40, 40), (-40, -40), (60, 60), (-70, -70), (70, 0)])
def test_power_of_two_scales_give_the_same_counts(S, ref, device, dtype, eg, eq):
    gal, labels, q, targets = _edge_data(dtype)
    gal, q = gal.to(dtype).float(), q.to(dtype).float()         # the values the unscaled call sees
    thr = np.linspace(-0.15, 0.3, 64)
    base, _, _ = _sweep_vs_oracle(S, ref, device, gal, labels, q, targets, thr, dtype)
    sg, sq = 2.0 ** eg, 2.0 ** eq
    cap = {"cand_cap": q.shape[0] * gal.shape[0]} if eg == 70 else {}       # an infinite measured bound: every pair is rechecked
    res, _, _ = _sweep_vs_oracle(S, ref, device, gal * sg, labels, q * sq, targets, thr * (sg * sq), dtype, **cap)
    assert torch.equal(res.tp, base.tp) and torch.equal(res.fp, base.fp)
    assert torch.equal(res.pos, base.pos) and torch.equal(res.neg, base.neg)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_a_row_above_the_measurable_norm_sends_every_pair_to_the_recheck(S, ref, device, dtype):
    gal, labels, q, targets = _edge_data(dtype)
    N, Q = gal.shape[0], q.shape[0]
    gal[77] = gal[77] * 3e19                                     # norm above 2e19: the measured bound is +inf
    thr = np.linspace(-0.15, 0.3, 64)
    res, _, _ = _sweep_vs_oracle(S, ref, device, gal, labels, q, targets, thr, dtype, cand_cap=Q * N)
    assert res.counts == (Q * N, Q * N)


# ------------------------------------------------------------------ 6. passes and capacities
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("E,Q,T", [(128, 70, 1024), (512, 70, 1024), (768, 70, 1024), (512, 300, 1), (768, 300, 1), (512, 75, 200),
                                   (128, 150, 1), (256, 200, 1)])
def test_more_queries_than_one_pass_holds(S, ref, device, E, Q, T, dtype):
    """T = 1024 leaves room for 29 (E = 128) or 11 (E >= 512) queries per pass, T = 200 for 64, and T = 1 is bounded by
    the kernel's resident queries (64 / 128 / 256 / 128 at E = 128 / 256 / 512 / 768): each case takes at least two
    gallery passes, and the T = 1 cases fill every multiplying wave."""
    N = 3001
    gal, labels, centres = H.labelled_gallery(N, E, seed=E + T, dtype=dtype)
    q, targets = H.labelled_queries(Q, E, centres, seed=Q + T, dtype=dtype)
    thr = np.array([0.05]) if T == 1 else np.linspace(-0.2, 0.35, T)
    want_ge, want_total, _ = H.oracle_sweep(ref, H.f32(q), H.f32(gal), labels.numpy(), targets.numpy(), thr)
    res = S.threshold_sweep(q.to(device), gal.to(device), labels.to(device), targets.to(device), thr)
    H.check_sweep(res, want_ge, want_total)


def test_candidate_overflow_is_reported_and_the_wrapper_retries(S, ref, device):
    N, Q, E = 4000, 7, 512
    gal, labels, centres = H.labelled_gallery(N, E, seed=51, dtype=torch.bfloat16)
    q, targets = H.labelled_queries(Q, E, centres, seed=52, dtype=torch.bfloat16)
    thr = np.linspace(-0.15, 0.3, 200)
    gd, qd, ld, td = gal.to(device), q.to(device), labels.to(device), targets.to(device)
    want_ge, want_total, _ = H.oracle_sweep(ref, H.f32(q), H.f32(gal), labels.numpy(), targets.numpy(), thr)
    ge, total, counts = _raw_sweep(device, qd, gd, ld, td, thr, cand_cap=1)
    done, cands = counts.tolist()
    assert done == 1 and cands > 1                                # overflow: reported, outputs incomplete
    ge2, total2, counts2 = _raw_sweep(device, qd, gd, ld, td, thr, cand_cap=cands)
    assert counts2.tolist() == [cands, cands]
    assert np.array_equal(ge2.cpu().numpy(), want_ge) and np.array_equal(total2.cpu().numpy(), want_total)
    res = S.threshold_sweep(qd, gd, ld, td, thr, cand_cap=1)      # the wrapper's retry
    H.check_sweep(res, want_ge, want_total)
    assert res.counts == (cands, cands)
    with pytest.raises(MemoryError):
        S.threshold_sweep(qd, gd, ld, td, thr, cand_cap=1, max_pairs=cands - 1)


# ------------------------------------------------------------------ 7. workspace poison
@pytest.mark.parametrize("case", ["bf16", "fp32, split in the call", "fp32, hi given, no residual bound", "bf16 masked"])
def test_outputs_do_not_depend_on_workspace_contents(ref, device, case):
    from mmr_amd import _lib
    N, Q, E = 4000, 7, 512
    dtype = torch.bfloat16 if case.startswith("bf16") else torch.float32
    gal, labels, centres = H.labelled_gallery(N, E, seed=61, dtype=dtype)
    q, targets = H.labelled_queries(Q, E, centres, seed=62, dtype=dtype)
    thr = np.linspace(-0.15, 0.3, 200)
    gd, qd, ld, td = gal.to(device), q.to(device), labels.to(device), targets.to(device)
    hi = words = None
    mask = None
    if "hi given" in case:
        hi = torch.empty(N, E, dtype=torch.bfloat16, device=device)
        lo = torch.empty_like(hi)
        _lib.check(_lib.lib().mmr_gallery_split_bf16(gd.data_ptr(), N, E, hi.data_ptr(), lo.data_ptr(), None, _lib.stream_ptr(device)))
    if "masked" in case:
        from mmr_amd import search
        mask = np.random.default_rng(4).random(N) < 0.6
        words = search._pack_row_mask(torch.from_numpy(mask).to(device), None, N)
    cap = Q * N
    zero = _raw_sweep(device, qd, gd, ld, td, thr, cap, 0x00, words, hi)
    ones = _raw_sweep(device, qd, gd, ld, td, thr, cap, 0xFF, words, hi)
    for a, b in zip(zero, ones):
        assert torch.equal(a, b)
    gf, lf = H.f32(gal), labels.numpy()
    if mask is not None:
        gf, lf = gf[mask], lf[mask]
    want_ge, want_total, _ = H.oracle_sweep(ref, H.f32(q), gf, lf, targets.numpy(), thr)
    assert np.array_equal(ones[0].cpu().numpy(), want_ge) and np.array_equal(ones[1].cpu().numpy(), want_total)


# ------------------------------------------------------------------ 8. score_extent
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_score_extent_is_the_exact_minimum_and_maximum(S, device, dtype):
    from oracle import search_ref
    N, Q, E = 5003, 6, 512
    gal, labels, centres = H.labelled_gallery(N, E, seed=71, dtype=dtype)
    q, _ = H.labelled_queries(Q, E, centres, seed=72, dtype=dtype)
    gf, qf = H.f32(gal), H.f32(q)
    mask = np.random.default_rng(8).random(N) < 0.5
    index = S.GalleryIndex(gal.to(device))
    for m in (mask, None):
        g_ = gf if m is None else gf[m]
        _, _, dmax = search_ref.cosine_topk(qf, g_, 1)
        _, _, dmin = search_ref.cosine_topk(-qf, g_, 1)
        lo, hi = index.score_extent(q.to(device), None if m is None else torch.from_numpy(m).to(device))
        assert np.array_equal(hi.cpu().numpy().view(np.int64), np.asarray(dmax, dtype=np.float64).reshape(-1).view(np.int64))
        assert np.array_equal(lo.cpu().numpy().view(np.int64), (-np.asarray(dmin, dtype=np.float64).reshape(-1)).view(np.int64))
    lo1, hi1 = index.score_extent(q[0].to(device))
    assert lo1.dim() == 0 and float(hi1) == float(hi[0]) and float(lo1) == float(lo[0])


# ------------------------------------------------------------------ the example
def test_threshold_sweep_example(device):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "threshold_sweep_synthetic.py")
    spec = importlib.util.spec_from_file_location("threshold_sweep_synthetic", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    report = mod.main(["--rows", "20000"])
    assert len(report) == 7
    for c, thr, f1, precision, recall in report:
        assert 0.0 < thr < 0.3 and 0.6 < f1 <= 1.0 and 0.0 < precision <= 1.0 and 0.0 < recall <= 1.0, report[c]
