"""GPU parity: decision masks (cosine_decide / GalleryIndex.decide / mmr_cosine_decide, mmr_row_mask_combine,
mmr_decision_counts) against the brute-force fp64 oracle of tests/decide_helpers.py.  Words are compared bit for bit,
pad bits included."""
import functools

import numpy as np
import pytest
import torch

import decide_helpers as H
import sweep_helpers as SH
from mmr_amd import synth

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "fp16", "fp32"]


@pytest.fixture(scope="module")
def S(device):
    from mmr_amd import search
    return search


@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


@functools.lru_cache(maxsize=None)
def _rows(n, E, seed):
    return synth.synth_unit_rows(n, E, seed=seed)


def _thresholds(Q, E):
    """Distinct per query: [0] below every dot of unit rows, [1] above every one, the rest spread over where the dots of
    random unit rows lie (standard deviation E^-1/2)."""
    sd = E ** -0.5
    thr = np.linspace(-2.0 * sd, 2.5 * sd, Q) + 1e-4 * np.arange(Q)
    if Q >= 1:
        thr[0] = -1.5
    if Q >= 2:
        thr[1] = 1.5
    return thr


def _threshold_sets(Q, E):
    """One call holds a threshold below every dot, one above and some in between; with fewer than three queries the three
    kinds take a call each."""
    if Q >= 3:
        return [_thresholds(Q, E)]
    sd = E ** -0.5
    return [np.full(Q, -1.5) - np.arange(Q), np.full(Q, 1.5) + np.arange(Q), np.linspace(-0.5 * sd, 0.5 * sd, Q + 1)[:Q]]


def _raw_decide(device, q, g, thr, cand_cap, fill=0xFF, mask_words=None, hi=None, resid=None, bound_dev=None):
    """mmr_cosine_decide through the C ABI with out_masks, counts and the workspace pre-filled with `fill` bytes.
    -> (words int32 [Q, W], counts int64 [2]) device tensors"""
    from mmr_amd import _lib
    L = _lib.lib()
    Q, E = q.shape
    N = g.shape[0]
    W = (N + 31) // 32
    need = L.mmr_decide_workspace_bytes(N, E, Q, cand_cap, _lib.dtype_code(g.dtype), int(hi is not None))
    assert need > 0
    ws = torch.full((need,), fill, dtype=torch.uint8, device=device)
    words = torch.full((max(Q * W, 1) * 4,), fill, dtype=torch.uint8, device=device).view(torch.int32)
    counts = torch.full((16,), fill, dtype=torch.uint8, device=device).view(torch.int64)
    thr_dev = torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float64)).to(device)
    _lib.check(L.mmr_cosine_decide(q.data_ptr(), g.data_ptr(), _lib.ptr(hi), _lib.dtype_code(g.dtype), Q, N, E,
                                   thr_dev.data_ptr(), 0.0, _lib.ptr(bound_dev), _lib.ptr(resid), _lib.ptr(mask_words), cand_cap,
                                   words.data_ptr(), counts.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr(device)))
    torch.cuda.synchronize(device)
    return words[:Q * W].view(Q, W), counts


def _assert_words(got, want, N):
    got = H.words_np(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        diff = H.unpack_words(got ^ want, want.shape[1] * 32)
        qs, rs = np.nonzero(diff)
        raise AssertionError(f"{len(qs)} bits differ from the oracle; first (query, row): {list(zip(qs[:8], rs[:8]))}, N={N}")


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("E", [128, 512, 768])
@pytest.mark.parametrize("Q", [1, 7, 33, 300])
@pytest.mark.parametrize("N", [1, 31, 33, 1000, 10007])
def test_parity(S, ref, device, N, Q, E, dtype):
    g = _rows(N, E, 1000 + N).to(dtype)
    q = _rows(Q, E, 2000 + Q).to(dtype)
    gf, qf = H.f32(g), H.f32(q)
    gd, qd = g.to(device), q.to(device)
    index = S.GalleryIndex(gd) if N > 1000 else None
    for thr in _threshold_sets(Q, E):
        want = H.oracle_decide(ref, qf, gf, thr)
        res = S.cosine_decide(qd, gd, thr) if index is None else index.decide(qd, thr)
        assert res.num_rows == N and tuple(res.words.shape) == (Q, (N + 31) // 32) and res.words.dtype == torch.int32
        _assert_words(res, want, N)
        done, cands = res.counts
        assert done == cands <= Q * N
        bits = H.unpack_words(want, N)
        if thr[0] == -1.5:
            assert bits[0].all()                                  # a threshold below every dot: all N bits
        if Q >= 2 and thr[1] == 1.5:
            assert not bits[1].any()                              # one above every dot: none
        assert np.array_equal(res.to_bool().cpu().numpy(), bits)
        assert np.array_equal(res.num_set().cpu().numpy(), bits.sum(1))
    if Q >= 3 and N >= 1000:
        assert 0 < bits[2:].sum() < (Q - 2) * N                   # and the thresholds in between split the gallery


def test_one_dimensional_query_and_a_scalar_threshold(S, ref, device):
    g = _rows(1000, 512, 2000).bfloat16()
    q = _rows(7, 512, 2007).bfloat16()
    gf, qf = H.f32(g), H.f32(q)
    res = S.cosine_decide(q[3].to(device), g.to(device), 0.01)
    assert tuple(res.words.shape) == (1, 32)
    _assert_words(res, H.oracle_decide(ref, qf[3:4], gf, [0.01]), 1000)
    res = S.cosine_decide(q.to(device), g.to(device), torch.full((7,), 0.02, dtype=torch.float64, device=device))
    _assert_words(res, H.oracle_decide(ref, qf, gf, np.full(7, 0.02)), 1000)


# ------------------------------------------------------------------ 2. thresholds that sit on exact dots
@pytest.mark.parametrize("case", ["bf16", "fp16", "fp32", "fp32 presplit"])
def test_boundary_twins(S, ref, device, case):
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(case, torch.float32)
    K = 16
    q, g, thr, rows = H.boundary_fixture(ref, 3001, 512, K, seed=11, dtype=dtype)
    qf, gf = H.f32(q), H.f32(g)
    bits, redecided = H.oracle_bits(ref, qf, gf, thr)
    assert redecided >= 2 * K
    H.check_twins(bits, rows)
    want = H.pack_bits(bits)
    qd, gd = q.to(device), g.to(device)
    results = {"cosine_decide": S.cosine_decide(qd, gd, thr)}
    if case == "fp32":
        results["index, split in the call"] = S.GalleryIndex(gd, presplit=False).decide(qd, thr)
    elif case == "fp32 presplit":
        results["index, presplit"] = S.GalleryIndex(gd, presplit=True).decide(qd, thr)
    else:
        results["index"] = S.GalleryIndex(gd).decide(qd, thr)
    for name, res in results.items():
        _assert_words(res, want, 3001)
        H.check_twins(res.to_bool().cpu().numpy(), rows)
        done, cands = res.counts
        print(f"{case} / {name}: {cands} candidates of {2 * K * 3001} pairs")
        assert done == cands and done >= 2 * K, (name, res.counts)   # the recheck ran, on the planted pairs at least
        assert cands < 2 * K * 3001                                  # and the scan decided the rest


# ------------------------------------------------------------------ 3. poison
@pytest.mark.parametrize("N", [33, 1000])
@pytest.mark.parametrize("Q", [1, 33, 300])
def test_every_word_is_written_whatever_the_buffers_held(ref, device, Q, N):
    E = 512
    g = _rows(N, E, 1000 + N).bfloat16()
    q = _rows(Q, E, 2000 + Q).bfloat16()
    thr = _thresholds(Q, E) if Q >= 3 else np.array([0.01])
    want = H.oracle_decide(ref, H.f32(q), H.f32(g), thr)
    gd, qd = g.to(device), q.to(device)
    outs = [_raw_decide(device, qd, gd, thr, 4096, fill) for fill in (0xFF, 0xA5, 0x00)]
    for words, counts in outs:
        _assert_words(words, want, N)                            # every word written, pad bits 0
        assert counts.tolist() == outs[0][1].tolist() and 0 <= counts[1] <= 4096
    if N % 32:
        assert int(H.words_np(outs[0][0])[:, -1].max()) < (1 << (N % 32))


def test_poison_with_an_fp32_gallery_split_in_the_call_and_a_mask(S, ref, device):
    N, Q, E = 1000, 33, 256
    g, q = _rows(N, E, 3000), _rows(Q, E, 3001)
    thr = _thresholds(Q, E)
    mask = np.random.default_rng(2).random(N) < 0.5
    words = S._pack_row_mask(torch.from_numpy(mask).to(device), None, N)
    want = H.oracle_decide(ref, H.f32(q), H.f32(g), thr, mask)
    for fill in (0xFF, 0xA5):
        got, counts = _raw_decide(device, q.to(device), g.to(device), thr, Q * N, fill, mask_words=words)
        _assert_words(got, want, N)
        assert counts[0] == counts[1]


# ------------------------------------------------------------------ 4. row masks, deletions, combinations
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_row_masks_and_deletions(S, ref, device, dtype):
    N, Q, E = 5003, 9, 512
    g, q = _rows(N, E, 4000).to(dtype), _rows(Q, E, 4001).to(dtype)
    gf, qf = H.f32(g), H.f32(q)
    thr = _thresholds(Q, E)
    gd, qd = g.to(device), q.to(device)
    plain_bits, _ = H.oracle_bits(ref, qf, gf, thr)
    plain = S.cosine_decide(qd, gd, thr)
    _assert_words(plain, H.pack_bits(plain_bits), N)
    rng = np.random.default_rng(3)
    for name, m in (("random", rng.random(N) < 0.5), ("all ones", np.ones(N, dtype=bool)), ("all zeros", np.zeros(N, dtype=bool))):
        res = S.cosine_decide(qd, gd, thr, row_mask=torch.from_numpy(m).to(device))
        _assert_words(res, H.pack_bits(plain_bits & m[None, :]), N)                     # unmasked AND mask
        _assert_words(res, H.oracle_decide(ref, qf, gf, thr, m), N)
    index = S.GalleryIndex(gd)
    gone = rng.choice(N, 700, replace=False)
    index.delete_rows(torch.from_numpy(gone))
    live = np.ones(N, dtype=bool)
    live[gone] = False
    _assert_words(index.decide(qd, thr), H.pack_bits(plain_bits & live[None, :]), N)
    half = rng.random(N) < 0.5
    _assert_words(index.decide(qd, thr, row_mask=torch.from_numpy(half).to(device)), H.pack_bits(plain_bits & (live & half)[None, :]), N)
    # a mask row feeds a masked search and delete_rows
    rm = plain.row_mask(2)
    assert rm.dtype == torch.bool and np.array_equal(rm.cpu().numpy(), plain_bits[2])
    _, idx = S.GalleryIndex(gd).search(qd[:1], 5, row_mask=rm)
    assert plain_bits[2][idx.cpu().numpy().reshape(-1)].all()
    index.restore_rows(torch.from_numpy(gone))
    index.delete_rows(rm.nonzero().reshape(-1))
    assert not index.decide(qd, thr).to_bool()[:, rm].any()


def test_combine_against_numpy(S, device):
    rng = np.random.default_rng(5)
    Q, N = 5, 1003
    a_bits, b_bits = rng.random((Q, N)) < 0.5, rng.random((Q, N)) < 0.3
    mk = lambda bits: S.DecisionMasks(torch.from_numpy(H.pack_bits(bits).view(np.int32).copy()).to(device), N)
    a, b = mk(a_bits), mk(b_bits)
    assert np.array_equal(H.words_np(a | b), H.pack_bits(a_bits | b_bits))
    assert np.array_equal(H.words_np(a & b), H.pack_bits(a_bits & b_bits))
    assert np.array_equal(H.words_np(a.andnot(b)), H.pack_bits(a_bits & ~b_bits))
    assert np.array_equal(H.words_np(a), H.pack_bits(a_bits)) and np.array_equal(H.words_np(b), H.pack_bits(b_bits))
    assert (a | b).num_rows == N and (a | b).counts is None
    # in place through the C call: out aliases a (OR), then out aliases b (AND-NOT)
    from mmr_amd import _lib
    c, d = mk(a_bits), mk(b_bits)
    for x, y, op, out in ((c, b, 0, c), (a, d, 2, d)):
        _lib.check(_lib.lib().mmr_row_mask_combine(x.words.data_ptr(), y.words.data_ptr(), op, out.words.numel(), out.words.data_ptr(),
                                                   _lib.stream_ptr(device)))
    assert np.array_equal(H.words_np(c), H.pack_bits(a_bits | b_bits))
    assert np.array_equal(H.words_np(d), H.pack_bits(a_bits & ~b_bits))


# ------------------------------------------------------------------ 5. capacities
def test_candidate_overflow_is_reported_and_the_wrapper_retries(S, ref, device):
    K = 16
    q, g, thr, rows = H.boundary_fixture(ref, 3001, 512, K, seed=11, dtype=torch.bfloat16)
    want = H.oracle_decide(ref, H.f32(q), H.f32(g), thr)
    qd, gd = q.to(device), g.to(device)
    words, counts = _raw_decide(device, qd, gd, thr, cand_cap=1)
    done, cands = counts.tolist()
    assert done == 1 and cands > 1                               # overflow: reported, masks incomplete
    words, counts = _raw_decide(device, qd, gd, thr, cand_cap=cands)
    assert counts.tolist() == [cands, cands]
    _assert_words(words, want, 3001)
    res = S.cosine_decide(qd, gd, thr, cand_cap=1)               # the wrapper's retry
    _assert_words(res, want, 3001)
    assert res.counts == (cands, cands)
    with pytest.raises(MemoryError):
        S.cosine_decide(qd, gd, thr, cand_cap=1, max_pairs=cands - 1)


# ------------------------------------------------------------------ 6. non-finite and extreme inputs
def _edge(dtype):
    return _rows(1000, 512, 6000).clone(), _rows(6, 512, 6001).clone(), np.array([-1.5, 1.5, -0.05, 0.0, 0.03, 0.06])


def _decide_vs_oracle(S, ref, device, g, q, thr, dtype, slack=1e-6, **kw):
    g, q = g.to(dtype), q.to(dtype)
    bits, _ = H.oracle_bits(ref, H.f32(q), H.f32(g), thr, slack=slack)
    res = S.cosine_decide(q.to(device), g.to(device), thr, **kw)
    _assert_words(res, H.pack_bits(bits), g.shape[0])
    return res, bits


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_nan_rows_and_a_nan_query(S, ref, device, dtype):
    g, q, thr = _edge(dtype)
    nan_rows = [0, 31, 32, 500, 999]
    g[nan_rows, 5] = float("nan")
    res, bits = _decide_vs_oracle(S, ref, device, g, q, thr, dtype, cand_cap=6000)
    assert not bits[:, nan_rows].any() and bits[0].sum() == 1000 - len(nan_rows)      # a NaN dot sets no bit
    q[2, 7] = float("nan")
    res, bits = _decide_vs_oracle(S, ref, device, g, q, thr, dtype, cand_cap=6000)
    assert not bits[2].any() and bits[0].sum() == 1000 - len(nan_rows)                # its neighbours are unaffected


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_an_infinite_row_makes_every_query_wild(S, ref, device, dtype):
    g, q, thr = _edge(dtype)
    g[10, 3] = float("inf")
    res, bits = _decide_vs_oracle(S, ref, device, g, q, thr, dtype, cand_cap=6000)
    assert res.counts == (6000, 6000)                            # an infinite norm bound: the recheck alone decides
    qf = H.f32(q.to(dtype))
    assert np.all(qf[:, 3] != 0)
    assert np.array_equal(bits[:, 10], qf[:, 3] > 0)             # +inf passes every finite threshold, -inf none


# fp16 holds neither 2^60 nor 2^30 (largest value 65504), and scaling unit rows DOWN pushes their small elements into
# fp16's subnormals, where the scaled row is no longer an exact image of the unscaled one: fp16 takes the upward scales
# its range allows, 2^8 on the rows and 2^4 on both operands.
_SCALES = [(torch.bfloat16, e) for e in ((60, 0), (-60, 0), (30, 30), (-30, -30))] + \
          [(torch.float32, e) for e in ((60, 0), (-60, 0), (30, 30), (-30, -30))] + [(torch.float16, e) for e in ((8, 0), (4, 4))]


@pytest.mark.parametrize("dtype,scales", _SCALES, ids=[f"{str(d).split('.')[1]}-{e[0]}-{e[1]}" for d, e in _SCALES])
def test_scaled_rows_decide_like_the_unscaled_ones(S, ref, device, dtype, scales):
    """Rows scaled by 2^60 (1e18) and 2^-60 (1e-18), and both operands by 2^+-30: power-of-two scales leave every dot's
    significand alone, so the masks are those of the unscaled call at the scaled thresholds."""
    eg, eq = scales
    g, q, thr = _edge(dtype)
    g, q = g.to(dtype).float(), q.to(dtype).float()
    base, bits = _decide_vs_oracle(S, ref, device, g, q, thr, dtype)
    sg, sq = 2.0 ** eg, 2.0 ** eq
    res, sbits = _decide_vs_oracle(S, ref, device, g * sg, q * sq, thr * (sg * sq), dtype, slack=1e-6 * sg * sq)
    assert np.array_equal(sbits, bits) and torch.equal(res.words, base.words)


# ------------------------------------------------------------------ 7. agreement with the existing calls
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_rows_are_exactly_range_searchs(S, device, dtype):
    N, Q, E = 10007, 7, 512
    gd, qd = _rows(N, E, 7000).to(dtype).to(device), _rows(Q, E, 7001).to(dtype).to(device)
    thr = np.linspace(0.02, 0.09, Q)
    index = S.GalleryIndex(gd)
    res = index.decide(qd, thr)
    for i in range(Q):
        rows, _ = index.range_search(qd[i], float(thr[i]))
        assert torch.equal(res.row_mask(i).nonzero().reshape(-1), rows), i
    assert int(res.num_set().sum()) > 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_confusion_equals_the_sweep_at_one_threshold(S, device, dtype):
    N, Q, E = 5003, 9, 512
    gal, labels, centres = SH.labelled_gallery(N, E, seed=21, dtype=dtype)
    q, targets = SH.labelled_queries(Q, E, centres, seed=22, dtype=dtype)
    gd, qd, ld, td = gal.to(device), q.to(device), labels.to(device), targets.to(device)
    t = 0.08
    sweep = S.threshold_sweep(qd, gd, ld, td, [t])
    res = S.cosine_decide(qd, gd, t)
    conf = res.confusion(ld, td)
    assert torch.equal(conf.tp, sweep.tp[:, 0]) and torch.equal(conf.fp, sweep.fp[:, 0])
    assert torch.equal(conf.fn, sweep.fn[:, 0]) and torch.equal(conf.tn, sweep.tn[:, 0])     # no NaN rows: the totals agree
    assert int(conf.tp.sum()) > 0 and int(conf.fp.sum()) > 0
    for mine, theirs in zip(conf.metrics(), sweep.metrics()):
        assert np.array_equal(mine, theirs[:, 0])
    # int64 labels and targets, and a row mask on both sides
    m = torch.from_numpy(np.random.default_rng(4).random(N) < 0.5).to(device)
    msweep = S.threshold_sweep(qd, gd, ld, td, [t], row_mask=m)
    mconf = res.confusion(ld.long(), td.long(), row_mask=m)
    assert torch.equal(mconf.tp, msweep.tp[:, 0]) and torch.equal(mconf.fp, msweep.fp[:, 0])
    assert torch.equal(mconf.pos, msweep.pos) and torch.equal(mconf.neg, msweep.neg)


def test_decision_counts_against_numpy(S, device):
    from mmr_amd import _lib
    rng = np.random.default_rng(6)
    for Q, N in ((1, 1), (3, 33), (5, 1003), (2, 300_001)):
        bits = rng.random((Q, N)) < 0.4
        labels = rng.integers(0, 4, N).astype(np.int32)
        targets = (np.arange(Q) % 5).astype(np.int32)            # target 4 is carried by no row
        live = rng.random(N) < 0.7
        masks = torch.from_numpy(H.pack_bits(bits).view(np.int32).copy()).to(device)
        ld, td = torch.from_numpy(labels).to(device), torch.from_numpy(targets).to(device)
        lw = S._pack_row_mask(torch.from_numpy(live).to(device), None, N)
        for use_labels in (True, False):
            for use_mask in (True, False):
                out = torch.full((Q, 4), -1, dtype=torch.int64, device=device)      # the call zeroes it
                _lib.check(_lib.lib().mmr_decision_counts(masks.data_ptr(), Q, N, _lib.ptr(ld if use_labels else None),
                                                          _lib.ptr(td if use_labels else None), _lib.ptr(lw if use_mask else None),
                                                          out.data_ptr(), _lib.stream_ptr(device)))
                lv = live if use_mask else np.ones(N, dtype=bool)
                same = (labels[None, :] == targets[:, None]) if use_labels else np.ones((Q, N), dtype=bool)
                want = np.stack([(bits & lv & same).sum(1), (bits & lv & ~same).sum(1), (lv & same).sum(1), (lv & ~same).sum(1)], 1)
                assert np.array_equal(out.cpu().numpy(), want), (Q, N, use_labels, use_mask)


def test_two_runs_are_bit_identical(S, ref, device):
    q, g, thr, rows = H.boundary_fixture(ref, 10007, 512, 16, seed=13, dtype=torch.bfloat16)
    qd, gd = q.to(device), g.to(device)
    thr = thr - 1e-5 * (np.arange(32) % 3)                       # some candidates pass the recheck, in any order
    a, b = S.cosine_decide(qd, gd, thr), S.cosine_decide(qd, gd, thr)
    assert torch.equal(a.words, b.words) and a.counts == b.counts and a.counts[0] > 0


# ------------------------------------------------------------------ 8. hipGraph capture
def test_capture_and_replay_with_new_thresholds(S, ref, device):
    from mmr_amd import _lib
    L = _lib.lib()
    N, Q, E = 10007, 33, 512
    g, q = _rows(N, E, 1000 + N).bfloat16(), _rows(Q, E, 2000 + Q).bfloat16()
    gf, qf = H.f32(g), H.f32(q)
    gd, qd = g.to(device), q.to(device)
    index = S.GalleryIndex(gd)                                   # its measured norm bound: the device scalar
    W = (N + 31) // 32
    cap = 1 << 16
    need = L.mmr_decide_workspace_bytes(N, E, Q, cap, _lib.dtype_code(gd.dtype), 0)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    words = torch.full((Q, W), -1, dtype=torch.int32, device=device)
    counts = torch.zeros(2, dtype=torch.int64, device=device)
    thr_dev = torch.from_numpy(_thresholds(Q, E)).to(device)

    def call():
        _lib.check(L.mmr_cosine_decide(qd.data_ptr(), gd.data_ptr(), None, _lib.dtype_code(gd.dtype), Q, N, E, thr_dev.data_ptr(),
                                       0.0, index.norm_bound_dev.data_ptr(), None, None, cap, words.data_ptr(), counts.data_ptr(),
                                       ws.data_ptr(), need, _lib.stream_ptr(device)))

    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        call()                                                   # warm: the kernels' attributes are set
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream(device).wait_stream(side)
    for shift in (0.01, -0.02):
        thr = _thresholds(Q, E) + shift
        thr_dev.copy_(torch.from_numpy(thr).to(device))
        words.fill_(-1)
        graph.replay()
        torch.cuda.synchronize(device)
        _assert_words(words, H.oracle_decide(ref, qf, gf, thr), N)
        done, cands = counts.tolist()
        assert done == cands <= cap


# ------------------------------------------------------------------ the example
def test_union_predict_example(ref, device, capsys):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "union_predict_synthetic.py")
    spec = importlib.util.spec_from_file_location("union_predict_synthetic", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--rows", "20000"])
    printed = capsys.readouterr().out
    labels = out["labels"]
    # the decisions themselves, recomputed from the features and the thresholds the example used
    en, cn = (H.oracle_bits(ref, H.f32(q), H.f32(g), thr)[0] for q, g, thr in (out["en"], out["cn"]))
    assert np.array_equal(out["en_bits"], en) and np.array_equal(out["cn_bits"], cn)
    union = en | cn
    C = union.shape[0]
    for c in range(C):
        pos = labels == c
        tp, fp = int((union[c] & pos).sum()), int((union[c] & ~pos).sum())
        fn, tn = int(pos.sum()) - tp, int((~pos).sum()) - fp
        assert out["report"][c][1:5] == (tp, fp, fn, tn), c
        assert f"class {c}: union TP {tp} FP {fp} FN {fn} TN {tn}" in printed
        assert tp > 0 and out["report"][c][5] > 0.5              # the union finds its class
        top = out["top5"][c]
        assert len(top) == 5 and union[c][top].all()             # the restricted search stays inside the union mask
