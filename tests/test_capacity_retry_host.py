"""CPU: the capacity-and-retry protocol of the six calls whose answer has an open size (``_retry.run``'s docstring), and
the driver itself.

The wrappers run on CPU tensors against a fake library: its ``mmr_*_workspace_bytes`` return a scripted size, its
``mmr_*`` calls record their arguments and write the next scripted ``counts`` through the pointer they were handed.
Nothing is computed, so the shapes are tiny.  The wrapper-level tests use only the six functions, ``_lib.lib`` and
``_lib.stream_ptr``; both are restored by ``monkeypatch``.

Not pinned here: that range search, the sweep and the hash join allocate their workspace anew on the retry.  Only the
pointer could tell, and an allocator may hand the same address out again; the size they pass (``max(need, 256)`` of that
attempt's capacities) is pinned.
"""
import ctypes

import pytest
import torch

from mmr_amd import _lib, dedup, search

Q, N, E, K = 3, 100, 128, 2
COUNTS, WS_PTR, WS_BYTES, STREAM = -4, -3, -2, -1       # the tail every one of these C calls ends with


class _Any:
    def __eq__(self, other):
        return True

    def __repr__(self):
        return "ANY"


ANY = _Any()


class FakeLib:
    """``script``: the counts each C call reports, in order.  ``ws``: bytes, or a function of the workspace call's arguments."""

    def __init__(self, script, ws=1000):
        self.script, self.ws = list(script), ws
        self.calls, self.ws_calls = [], []

    def __getattr__(self, name):
        if not name.startswith("mmr_"):
            raise AttributeError(name)
        if name.endswith("_workspace_bytes"):
            def size(*args):
                self.ws_calls.append((name, args))
                return self.ws(*args) if callable(self.ws) else self.ws
            return size

        def call(*args):
            self.calls.append((name, args))
            out = ctypes.cast(args[COUNTS], ctypes.POINTER(ctypes.c_int64))
            for i, c in enumerate(self.script.pop(0)):
                out[i] = c
            return 0
        return call

    def args(self, i=0):
        return self.calls[i][1]


@pytest.fixture
def fake(monkeypatch):
    def install(script, ws=1000):
        L = FakeLib(script, ws)
        monkeypatch.setattr(_lib, "lib", lambda: L)
        monkeypatch.setattr(_lib, "stream_ptr", lambda device=None: 0)
        return L
    return install


class T:
    """The operands, made once: no call writes to them."""
    g = torch.zeros(N, E, dtype=torch.bfloat16)
    q = torch.zeros(Q, E, dtype=torch.bfloat16)
    g32 = torch.zeros(3000, E, dtype=torch.float32)
    q32 = torch.zeros(Q, E, dtype=torch.float32)
    split = (torch.zeros(3000, E, dtype=torch.bfloat16), torch.zeros(3000, E, dtype=torch.bfloat16),
             torch.zeros((), dtype=torch.float32))
    words = torch.zeros((N + 31) // 32, dtype=torch.int32)
    qmasks = (torch.zeros(Q, 4, dtype=torch.int32), 4)
    labels = torch.zeros(N, dtype=torch.int32)
    targets = torch.zeros(Q, dtype=torch.int32)
    grid = torch.tensor([0.1, 0.2, 0.3, 0.4], dtype=torch.float64)
    thr = torch.zeros(Q, dtype=torch.float64)
    cent = torch.zeros(5, E, dtype=torch.bfloat16)
    bias = torch.zeros(5, dtype=torch.float64)
    refs = torch.zeros(N, 2, 1, dtype=torch.int64)
    hq = torch.zeros(Q, 2, 1, dtype=torch.int64)


def _range(q=T.q, words=None, cap=None, cand_cap=None, max_pairs=1 << 27, threshold=0.5, g=T.g, split=None):
    return search._range_call(q, g, threshold, 1.0, None, None, split, cap, cand_cap, max_pairs, words)


def _deep(tile_cap=None, surv_cap=None, max_pairs=1 << 27, qmasks=None, k=K, q=T.q, g=T.g, split=None, workspace=None,
          words=None, want_dot64=False):
    return search._deep_call(q, g, k, 1.0, None, None, split, words, max_pairs, tile_cap, surv_cap, want_dot64, workspace, qmasks)


# ---- the four calls with one capacity: (wrapper(cap, ceiling, workspace), C call, workspace call, capacity's place in each,
#      counts for a needed size, the two messages, returned counts, returned workspace)

class One:
    def __init__(self, run, cname, wsname, cap_at, ws_cap_at, default_cap, overflow_msg, ceiling_msg, counts_of=None,
                 workspace_of=None, once=()):
        self.run, self.cname, self.wsname, self.cap_at, self.ws_cap_at = run, cname, wsname, cap_at, ws_cap_at
        self.default_cap, self.overflow_msg, self.ceiling_msg = default_cap, overflow_msg, ceiling_msg
        self.counts_of, self.workspace_of, self.once = counts_of, workspace_of, once
        self.hash = "hash" in cname

    def counts(self, needed):
        return (needed,) if self.hash else (1, needed)


def _sweep(qmasks=None):
    return lambda cap, ceiling, ws: search._sweep_call(T.q, T.g, T.labels, T.targets, T.grid, None, None, None, cap, ceiling,
                                                       T.words, False, qmasks)


def _hash(queries):
    return lambda cap, ceiling, ws: dedup._hash_call(queries, T.refs, [5, 3], T.words, cap, ceiling)


_SWEEP_MSGS = ("threshold sweep: {n} candidates exceed the capacity {cap} it reported",
               "threshold sweep needs room for {n} candidate pairs, above max_pairs={ceiling}: use a coarser grid or raise max_pairs")
_HASH_MSGS = ("hash join: {n} matches exceed the capacity {cap} the first call reported",
              "hash join at thresholds [5, 3] needs room for {n} pairs, above max_pairs={ceiling}: lower the thresholds or raise "
              "max_pairs")
ONES = {
    "sweep": One(_sweep(), "mmr_threshold_sweep", "mmr_sweep_workspace_bytes", -7, 4, 1 << 16, *_SWEEP_MSGS,
                 counts_of=lambda r: r.counts, once=(-6, -5)),
    "sweep_qmasked": One(_sweep(T.qmasks), "mmr_threshold_sweep_qmasked", "mmr_sweep_workspace_bytes", -7, 4, 1 << 16, *_SWEEP_MSGS,
                         counts_of=lambda r: r.counts, once=(-6, -5)),
    "decide": One(lambda cap, ceiling, ws: search._decide_call(T.q, T.g, T.thr, None, None, None, cap, ceiling, T.words, ws),
                  "mmr_cosine_decide", "mmr_decide_workspace_bytes", -6, 3, 1 << 16,
                  "decide: {n} candidates exceed the capacity {cap} it reported",
                  "decide needs room for {n} candidate pairs, above max_pairs={ceiling}: raise max_pairs",
                  counts_of=lambda r: r[0].counts, workspace_of=lambda r: r[1], once=(-5,)),
    "assign": One(lambda cap, ceiling, ws: search._assign_call(T.g, T.cent, T.bias, None, None, T.words, True, cap, ceiling, ws),
                  "mmr_cosine_assign", "mmr_assign_workspace_bytes", -7, 3, 1 << 16,
                  "assign: {n} ambiguous rows exceed the capacity {cap} it reported",
                  "assign needs room for {n} ambiguous rows, above max_ambiguous={ceiling}: raise max_ambiguous",
                  counts_of=lambda r: r[2], workspace_of=lambda r: r[3], once=(-6, -5)),
    "hash_self": One(_hash(None), "mmr_hash_self_join", "mmr_hash_join_workspace_bytes", -8, 4, 1 << 16, *_HASH_MSGS),
    "hash_cross": One(_hash(T.hq), "mmr_hash_cross_join", "mmr_hash_join_workspace_bytes", -8, 4, 1 << 16, *_HASH_MSGS),
}
one = pytest.mark.parametrize("w", ONES.values(), ids=ONES.keys())
REUSES = [k for k, w in ONES.items() if w.workspace_of]


@one
def test_one_capacity_fits_first_time(fake, w):
    L = fake([w.counts(5)])
    r = w.run(5, 1 << 20, None)
    assert [c[0] for c in L.calls] == [w.cname] and [c[0] for c in L.ws_calls] == [w.wsname]
    assert L.args()[w.cap_at] == 5 and L.ws_calls[0][1][w.ws_cap_at] == 5
    assert L.args()[WS_BYTES] == 1000 and L.args()[STREAM] == 0
    if w.counts_of:
        assert w.counts_of(r) == (1, 5)
    else:                                                # the joins slice their lists to the count
        assert [t.shape[0] for t in r] == [5, 5, 5] and [t.dtype for t in r] == [torch.int32, torch.int32, torch.int64]
        assert [t.untyped_storage().nbytes() for t in r] == [20, 20, 40]
        assert [t.data_ptr() for t in r] == list(L.args()[-7:-4])


@one
def test_one_capacity_default_first_capacity(fake, w):
    for cap in (None,) if w.hash else (None, 0):
        L = fake([w.counts(0)])
        w.run(cap, 1 << 27, None)
        assert L.args()[w.cap_at] == w.default_cap and len(L.calls) == 1


@one
def test_one_capacity_overflow_then_fit(fake, w):
    L = fake([w.counts(40), w.counts(40)], ws=lambda *a: 16 * a[w.ws_cap_at])
    r = w.run(5, 40, None)                               # the ceiling itself is allowed
    assert [c[0] for c in L.calls] == [w.cname] * 2
    assert [a[w.cap_at] for _, a in L.calls] == [5, 40] and [a[w.ws_cap_at] for _, a in L.ws_calls] == [5, 40]
    assert [a[WS_BYTES] for _, a in L.calls] == [256, 640]
    assert L.args(0)[COUNTS] == L.args(1)[COUNTS]                       # counts is made once
    for at in w.once:                                                   # and so are the outputs of a fixed size
        assert L.args(0)[at] == L.args(1)[at]
    # nothing but the capacity, the workspace and (for the joins) the outputs changes between the attempts
    varies = {w.cap_at, WS_PTR, WS_BYTES} | (set() if w.counts_of else {-7, -6, -5})
    n = len(L.args(0))
    assert [x for i, x in enumerate(L.args(0)) if i - n not in varies] == [x for i, x in enumerate(L.args(1)) if i - n not in varies]
    if w.counts_of:
        assert w.counts_of(r) == (1, 40)
    else:
        assert [t.shape[0] for t in r] == [40] * 3 and r[0].untyped_storage().nbytes() == 160


@one
def test_one_capacity_overflow_twice(fake, w):
    L = fake([w.counts(40), w.counts(41)])
    with pytest.raises(RuntimeError) as e:
        w.run(5, 1 << 20, None)
    assert str(e.value) == w.overflow_msg.format(n=41, cap=40) and type(e.value) is RuntimeError
    assert [a[w.cap_at] for _, a in L.calls] == [5, 40]


@one
def test_one_capacity_over_the_ceiling(fake, w):
    L = fake([w.counts(40)])
    with pytest.raises(MemoryError) as e:
        w.run(5, 39, None)
    assert str(e.value) == w.ceiling_msg.format(n=40, ceiling=39)
    assert len(L.calls) == 1


def test_assign_default_capacity_stops_at_the_ceiling(fake):
    for ceiling, want in ((100, 100), (0, 1), (1 << 20, 1 << 16)):
        L = fake([(0, 0)])
        search._assign_call(T.g, T.cent, None, None, None, None, False, None, ceiling)
        assert L.args()[-7] == want and L.args()[-5] == 0                # no best64 asked for: a null pointer


def test_hash_cap_zero_still_has_outputs(fake):
    L = fake([(0,)])
    r = dedup._hash_call(None, T.refs, 5, None, 0, 1 << 20)
    assert L.args()[-8] == 0 and [t.shape[0] for t in r] == [0] * 3 and r[0].untyped_storage().nbytes() == 4


@pytest.mark.parametrize("w", [ONES[k] for k in REUSES], ids=REUSES)
def test_one_capacity_workspace_is_reused_when_large_enough(fake, w):
    ws = torch.empty(4096, dtype=torch.uint8)
    L = fake([w.counts(5)], ws=4096)
    assert w.workspace_of(w.run(5, 1 << 20, ws)) is ws
    assert L.args()[WS_PTR] == ws.data_ptr() and L.args()[WS_BYTES] == 4096
    for need, want in ((4097, 4097), (100, 256)):                       # too small, none at all: max(need, 256) new bytes
        for given in (ws, None):
            if given is ws and need <= ws.numel():
                continue
            L = fake([w.counts(5)], ws=need)
            got = w.workspace_of(w.run(5, 1 << 20, given))
            assert got is not ws and got.dtype == torch.uint8 and got.numel() == want
            assert L.args()[WS_PTR] == got.data_ptr() and L.args()[WS_BYTES] == want
    # the retry keeps the workspace unless the need grew
    L = fake([w.counts(40), w.counts(40)], ws=4000)
    assert w.workspace_of(w.run(5, 1 << 20, ws)) is ws
    assert [a[WS_PTR] for _, a in L.calls] == [ws.data_ptr()] * 2
    L = fake([w.counts(40), w.counts(40)], ws=lambda *a: 1000 * a[w.ws_cap_at])
    got = w.workspace_of(w.run(4, 1 << 20, ws))                         # 4000 bytes, then 40000
    assert got is not ws and got.numel() == 40000
    assert [a[WS_PTR] for _, a in L.calls] == [ws.data_ptr(), got.data_ptr()] and [a[WS_BYTES] for _, a in L.calls] == [4096, 40000]


def test_one_capacity_prechecks_come_before_any_call(fake):
    for key, text in (("decide", "cand_cap must be >= 1"), ("assign", "amb_cap must be >= 1"), ("hash_self", "cap=-1 must be >= 0"),
                      ("hash_cross", "cap=-1 must be >= 0")):
        L = fake([])
        with pytest.raises(ValueError) as e:
            ONES[key].run(-1, 1 << 20, None)
        assert str(e.value) == text and not L.calls and not L.ws_calls


def test_one_capacity_c_arguments(fake):
    p = lambda t: t.data_ptr()  # noqa: E731
    tail = [ANY, ANY, 1000, 0]
    L = fake([(1, 5)])
    r = ONES["sweep"].run(5, 99, None)
    assert list(L.args()) == [p(T.q), p(T.g), 0, 1, Q, N, E, p(T.labels), p(T.targets), p(T.grid), 4, 0.0, 0, 0, p(T.words), 5,
                              ANY, ANY] + tail
    assert L.ws_calls[0][1] == (N, E, Q, 4, 5, 1, 0)
    assert r.tp.shape == (Q, 4) and r.pos.shape == (Q,) and r.tp.data_ptr() != r.fp.data_ptr()
    L = fake([(1, 5)])
    ONES["sweep_qmasked"].run(5, 99, None)
    assert list(L.args()) == [p(T.q), p(T.g), 0, 1, Q, N, E, p(T.labels), p(T.targets), p(T.grid), 4, 0.0, 0, 0, p(T.qmasks[0]), 4,
                              p(T.words), 5, ANY, ANY] + tail
    L = fake([(1, 5)])
    masks, _ = ONES["decide"].run(5, 99, None)
    assert list(L.args()) == [p(T.q), p(T.g), 0, 1, Q, N, E, p(T.thr), 0.0, 0, 0, p(T.words), 5, p(masks.words)] + tail
    assert L.ws_calls[0][1] == (N, E, Q, 5, 1, 0)
    assert masks.words.shape == (Q, 4) and masks.words.dtype == torch.int32 and masks.num_rows == N
    L = fake([(1, 5)])
    labels, best64, _, _ = ONES["assign"].run(5, 99, None)
    assert list(L.args()) == [p(T.g), p(T.cent), 1, N, 5, E, p(T.bias), 0.0, 0, p(T.words), 5, p(labels), p(best64)] + tail
    assert L.ws_calls[0][1] == (N, E, 5, 5, 1)
    assert (labels.shape, labels.dtype, best64.shape, best64.dtype) == ((N,), torch.int32, (N,), torch.float64)
    L = fake([(5,)])
    a, b, d = ONES["hash_self"].run(5, 99, None)
    assert list(L.args()[:4]) == [p(T.refs), N, 2, 1] and list(L.args()[4]) == [5, 3]
    assert list(L.args()[5:]) == [p(T.words), 5, p(a), p(b), p(d)] + tail
    assert L.ws_calls[0][1] == (0, N, 2, 1, 5)
    L = fake([(5,)])
    a, b, d = ONES["hash_cross"].run(5, 99, None)
    assert list(L.args()[:6]) == [p(T.hq), Q, p(T.refs), N, 2, 1] and list(L.args()[6]) == [5, 3]
    assert list(L.args()[7:]) == [p(T.words), 5, p(a), p(b), p(d)] + tail
    assert L.ws_calls[0][1] == (Q, N, 2, 1, 5)


# ---- range search: two capacities, (matches, candidates)

RANGE_FORMS = {"range": (T.q, None, "mmr_cosine_range"), "self_join": (None, None, "mmr_gallery_self_join"),
               "range_masked": (T.q, T.words, "mmr_cosine_range_masked"),
               "self_join_masked": (None, T.words, "mmr_gallery_self_join_masked")}
range_forms = pytest.mark.parametrize("q,words,cname", RANGE_FORMS.values(), ids=RANGE_FORMS.keys())


def _range_caps(L):
    return [(a[-10], a[-9]) for _, a in L.calls]


@range_forms
def test_range_fits_first_time(fake, q, words, cname):
    L = fake([(7, 9)])
    r = _range(q, words, cap=10, cand_cap=12)
    assert [c[0] for c in L.calls] == [cname] and [c[0] for c in L.ws_calls] == ["mmr_range_workspace_bytes"]
    assert _range_caps(L) == [(10, 12)] and L.ws_calls[0][1] == (N, E, 0 if q is None else Q, 12, 1, 0)
    assert [t.shape[0] for t in r] == [7] * 4
    assert [t.dtype for t in r] == [torch.int32, torch.int32, torch.float32, torch.float64]
    assert [t.untyped_storage().nbytes() for t in r] == [40, 40, 40, 80]
    p = lambda t: t.data_ptr()  # noqa: E731
    head = [p(T.g), 0, 1, N, E, 0.5] if q is None else [p(T.q), p(T.g), 0, 1, Q, N, E, 0.5]
    mask = [] if words is None else [p(words)]
    assert list(L.args()) == head + [1.0, 0.0, 0, 0] + mask + [10, 12] + [p(t) for t in r] + [ANY, ANY, 1000, 0]


def test_range_default_capacities(fake):
    for cap, cand_cap, want in ((None, None, (1 << 16, 1 << 16)), (None, 0, (1 << 16, 1 << 16)), (None, 50, (50, 50)),
                                (7, None, (7, 1 << 16)), (0, 9, (0, 9))):
        L = fake([(0, 0)])
        r = _range(cap=cap, cand_cap=cand_cap)
        assert _range_caps(L) == [want]
        assert r[0].untyped_storage().nbytes() == 4 * max(want[0], 1)


@range_forms
@pytest.mark.parametrize("caps,first,second", [
    ((3, 5), (50, 200), (200, 200)),        # the candidates overflow: the matches are undercounted, so both grow to them
    ((1, 5), (2, 4), (2, 5)),               # only the matches overflow
    ((500, 5), (50, 200), (500, 200)),      # the candidates overflow under a cap that exceeds them already: it is kept
])
def test_range_overflow_then_fit(fake, q, words, cname, caps, first, second):
    L = fake([first, (2, 4)], ws=lambda *a: 16 * a[3])
    r = _range(q, words, cap=caps[0], cand_cap=caps[1], max_pairs=200)
    assert [c[0] for c in L.calls] == [cname] * 2
    assert _range_caps(L) == [caps, second] and [a[3] for _, a in L.ws_calls] == [caps[1], second[1]]
    assert [a[WS_BYTES] for _, a in L.calls] == [max(16 * caps[1], 256), max(16 * second[1], 256)]
    assert L.args(0)[COUNTS] == L.args(1)[COUNTS]
    assert [t.shape[0] for t in r] == [2] * 4 and r[3].untyped_storage().nbytes() == 8 * second[0]
    assert [t.data_ptr() for t in r] == list(L.args(1)[-8:-4])
    n = len(L.args(0))
    fixed = [i for i in range(n) if i - n not in (-10, -9, -8, -7, -6, -5, WS_PTR, WS_BYTES)]
    assert [L.args(0)[i] for i in fixed] == [L.args(1)[i] for i in fixed]


def test_range_overflow_twice(fake):
    L = fake([(50, 200), (60, 300)])
    with pytest.raises(RuntimeError) as e:
        _range(cap=3, cand_cap=5)
    assert str(e.value) == "range search: counts 60/300 exceed the capacities 200/200 it reported" and type(e.value) is RuntimeError
    assert _range_caps(L) == [(3, 5), (200, 200)]
    L = fake([(2, 4), (3, 4)])                                           # the matches alone, twice
    with pytest.raises(RuntimeError) as e:
        _range(cap=1, cand_cap=5)
    assert str(e.value) == "range search: counts 3/4 exceed the capacities 2/5 it reported"


def test_range_over_the_ceiling(fake):
    L = fake([(50, 200)])
    with pytest.raises(MemoryError) as e:
        _range(cap=3, cand_cap=5, max_pairs=199)
    assert str(e.value) == ("range search at threshold 0.5 needs room for 200 candidate pairs, above max_pairs=199: "
                            "raise the threshold or max_pairs")
    assert len(L.calls) == 1
    L = fake([(9, 20)])                       # the candidates fit the caller's capacity, yet exceed the caller's ceiling
    with pytest.raises(MemoryError, match="room for 20 candidate pairs, above max_pairs=10"):
        _range(cap=3, cand_cap=30, max_pairs=10)
    assert len(L.calls) == 1


def test_range_threshold_is_checked_before_any_call(fake):
    for bad in (float("nan"), float("inf"), float("-inf")):
        L = fake([])
        with pytest.raises(ValueError) as e:
            _range(threshold=bad)
        assert str(e.value) == f"threshold must be finite (got {bad})" and not L.calls and not L.ws_calls


def test_range_split_gallery(fake):
    L = fake([(0, 0)])
    _range(T.q32, g=T.g32, split=T.split, cap=4, cand_cap=4)
    assert list(L.args()[:8]) == [T.q32.data_ptr(), T.g32.data_ptr(), T.split[0].data_ptr(), 0, Q, 3000, E, 0.5]
    assert L.args()[11] == T.split[2].data_ptr() and L.ws_calls[0][1] == (3000, E, Q, 4, 0, 1)


# ---- deep top-k: two capacities, (listed tiles, survivors)

DEEP_FORMS = {"deep": (None, "mmr_cosine_topk_deep", "mmr_deep_topk_workspace_bytes"),
              "deep_qmasked": (T.qmasks, "mmr_cosine_topk_deep_qmasked", "mmr_deep_topk_qmasked_workspace_bytes")}
deep_forms = pytest.mark.parametrize("qmasks,cname,wsname", DEEP_FORMS.values(), ids=DEEP_FORMS.keys())


def _deep_caps(L):
    return [(a[-9], a[-8]) for _, a in L.calls]


@deep_forms
def test_deep_fits_first_time(fake, qmasks, cname, wsname):
    L = fake([(4, 6)])
    idx, score, dot64, ws, counts = _deep(4, 6, qmasks=qmasks, words=T.words, want_dot64=True)
    assert [c[0] for c in L.calls] == [cname] and [c[0] for c in L.ws_calls] == [wsname]
    assert counts == (4, 6) and L.ws_calls[0][1] == (N, E, Q, K, 4, 6, 1, 0)
    assert [t.shape for t in (idx, score, dot64)] == [(Q, K)] * 3
    assert [t.dtype for t in (idx, score, dot64)] == [torch.int64, torch.float32, torch.float64]
    assert ws.numel() == 1000 and ws.dtype == torch.uint8
    p = lambda t: t.data_ptr()  # noqa: E731
    head = [p(T.q), p(T.g), 0, 0, 0, 1, Q, N, E, K, 1.0, 0.0, 0]
    mid = [] if qmasks is None else [p(qmasks[0]), 4]
    assert list(L.args()) == head + mid + [p(T.words), 4, 6, p(idx), p(score), p(dot64), ANY, p(ws), 1000, 0]
    L = fake([(1, 1)])
    assert _deep(4, 6, qmasks=qmasks)[2] is None and L.args()[-5] == 0 and L.args()[-10] == 0       # no dot64, no shared mask


def test_deep_default_and_clamped_first_capacities(fake):
    L = fake([(1, 1)])
    _deep()                                   # 2 * Q * k + 4096 entries, but no more than Q * tiles / Q * N
    assert _deep_caps(L) == [(Q * 4, Q * N)]
    L = fake([(1, 1)])
    _deep(q=T.q32, g=T.g32)                   # unsplit fp32: 16-row tiles, 3 * 188 of them
    assert _deep_caps(L) == [(564, 2 * Q * K + 4096)]
    L = fake([(1, 1)])
    _deep(k=4)                                # k * 32 >= N: every tile is listed and every row kept, so start there
    assert _deep_caps(L) == [(Q * 4, Q * N)]
    L = fake([(1, 1)])
    _deep(10 ** 6, 10 ** 6)
    assert _deep_caps(L) == [(Q * 4, Q * N)]


@deep_forms
def test_deep_tile_list_overflow_sizes_the_survivors_by_the_tiles(fake, qmasks, cname, wsname):
    L = fake([(500, 20), (500, 280)], ws=lambda *a: 8 * a[4] + 32 * a[5])
    *_, ws, counts = _deep(4, 6, qmasks=qmasks)
    assert [c[0] for c in L.calls] == [cname] * 2
    assert _deep_caps(L) == [(4, 6), (500, 300)]                         # 500 * 32 rows, clamped to Q * N
    assert counts == (500, 280) and ws.numel() == 8 * 500 + 32 * 300
    assert [a[4:6] for _, a in L.ws_calls] == [(4, 6), (500, 300)]
    n = len(L.args(0))
    fixed = [i for i in range(n) if i - n not in (-9, -8, WS_PTR, WS_BYTES)]
    assert [L.args(0)[i] for i in fixed] == [L.args(1)[i] for i in fixed]    # counts and the outputs are made once


def test_deep_tile_rows_of_the_retry(fake):
    L = fake([(500, 20), (1, 1)])
    _deep(4, 6, q=T.q32, g=T.g32)                                        # fp32 without a split: 16 rows per tile
    assert _deep_caps(L) == [(4, 6), (500, 8000)]
    L = fake([(500, 20), (1, 1)])
    _deep(4, 6, q=T.q32, g=T.g32, split=T.split)                         # split: 32, clamped to Q * N = 9000
    assert _deep_caps(L) == [(4, 6), (500, 9000)]
    assert list(L.args()[2:5]) == [t.data_ptr() for t in T.split]


def test_deep_only_the_survivors_overflow(fake):
    L = fake([(3, 20), (3, 20)])
    assert _deep(4, 6)[4] == (3, 20)
    assert _deep_caps(L) == [(4, 6), (4, 20)]


def test_deep_overflow_twice(fake):
    L = fake([(500, 20), (600, 20)])
    with pytest.raises(RuntimeError) as e:
        _deep(4, 6)
    assert str(e.value) == "deep top-k: counts 600/20 exceed the capacities 500/300 it reported" and type(e.value) is RuntimeError
    assert len(L.calls) == 2


def test_deep_over_the_ceiling(fake):
    L = fake([(500, 20)])
    with pytest.raises(MemoryError) as e:
        _deep(4, 6, max_pairs=400)
    assert str(e.value) == ("deep top-k with k=2 needs room for 500 listed tiles and up to 300 surviving rows, above max_pairs=400: "
                            "lower k or raise max_pairs")
    assert len(L.calls) == 1
    L = fake([(3, 20)])
    with pytest.raises(MemoryError, match="room for 3 listed tiles and up to 20 surviving rows, above max_pairs=10:"):
        _deep(4, 6, max_pairs=10)
    assert len(L.calls) == 1
    L = fake([(3, 20), (3, 20)])
    _deep(4, 6, max_pairs=20)                                            # the ceiling itself is allowed
    assert len(L.calls) == 2


def test_deep_prechecks_come_before_any_call(fake):
    L = fake([])
    for k in (0, 4097):
        with pytest.raises(ValueError) as e:
            _deep(k=k)
        assert str(e.value) == f"k={k} outside [1, 4096]"
    for caps in ((-1, 6), (4, -1)):
        with pytest.raises(ValueError) as e:
            _deep(*caps)
        assert str(e.value) == "tile_cap and surv_cap must be >= 1"
    with pytest.raises(MemoryError) as e:
        _deep(4, 6, max_pairs=5)
    assert str(e.value) == ("deep top-k with k=2: first capacities 4 tiles / 6 rows exceed max_pairs=5: lower k, pass tile_cap / "
                            "surv_cap, or raise max_pairs")
    assert not L.calls and not L.ws_calls


def test_deep_without_queries_returns_before_any_call(fake):
    L = fake([])
    ws = torch.empty(8, dtype=torch.uint8)
    idx, score, dot64, got, counts = _deep(q=T.q[:0], workspace=ws, want_dot64=True)
    assert idx.shape == score.shape == dot64.shape == (0, K) and got is ws and counts == (0, 0)
    assert not L.calls and not L.ws_calls


def test_deep_workspace(fake):
    ws = torch.empty(4096, dtype=torch.uint8)
    L = fake([(1, 1)], ws=4096)
    assert _deep(4, 6, workspace=ws)[3] is ws and L.args()[WS_PTR] == ws.data_ptr() and L.args()[WS_BYTES] == 4096
    for need, given, want in ((4097, ws, 4097), (100, None, 256), (5000, None, 5000)):
        L = fake([(1, 1)], ws=need)
        got = _deep(4, 6, workspace=given)[3]
        assert got is not ws and got.numel() == want and L.args()[WS_PTR] == got.data_ptr() and L.args()[WS_BYTES] == want
    L = fake([(3, 20), (3, 20)], ws=4000)                                # the retry needs no more: the same tensor
    assert _deep(4, 6, workspace=ws)[3] is ws and [a[WS_PTR] for _, a in L.calls] == [ws.data_ptr()] * 2
    L = fake([(3, 20), (3, 20)], ws=lambda *a: 500 * a[5])               # 3000 bytes, then 10000
    got = _deep(4, 6, workspace=ws)[3]
    assert got.numel() == 10000 and [a[WS_PTR] for _, a in L.calls] == [ws.data_ptr(), got.data_ptr()]


# ---- the driver itself, on scripted launches (new with the driver; everything above also passes on the copies it replaced)

def _drive(script, caps, needed=None, ceiling=1 << 20):
    from mmr_amd import _retry
    seen, script = [], list(script)

    def launch(*caps):
        seen.append(caps)
        return script.pop(0)

    def run():
        return _retry.run(launch, caps, ceiling, lambda counts, caps: f"counts {list(counts)} over {list(caps)}",
                          lambda need: f"need {list(need)}", **({"needed": needed} if needed else {}))
    return run, seen


def _undercount(caps, counts):                      # range search's rule: an overflowed second list starves the first
    return (counts[1] if counts[1] > caps[1] else counts[0], counts[1])


def test_driver_fits_first_time():
    run, seen = _drive([[3, 5]], (5,))
    assert run() == [3, 5] and seen == [(5,)]                            # a count equal to the capacity fits
    run, seen = _drive([(7, 9)], (7, 9), _undercount)
    assert run() == (7, 9) and seen == [(7, 9)]


def test_driver_retries_once_at_the_larger_of_capacity_and_need():
    run, seen = _drive([[0, 40], [2, 40]], (5,), ceiling=40)
    assert run() == [2, 40] and seen == [(5,), (40,)]                    # the second attempt's counts are the answer
    run, seen = _drive([(50, 200), (60, 200)], (3, 5), _undercount)
    assert run() == (60, 200) and seen == [(3, 5), (200, 200)]
    run, seen = _drive([(2, 4), (2, 4)], (1, 5), _undercount)
    assert run() == (2, 4) and seen == [(1, 5), (2, 5)]                  # a capacity that was enough is kept, not shrunk
    run, seen = _drive([(50, 200), (50, 200)], (500, 5), _undercount)
    assert run() and seen == [(500, 5), (500, 200)]


def test_driver_second_overflow_is_a_runtime_error():
    run, seen = _drive([[0, 40], [0, 41]], (5,))
    with pytest.raises(RuntimeError) as e:
        run()
    assert str(e.value) == "counts [0, 41] over [40]" and seen == [(5,), (40,)]      # the counts and capacities of the retry


def test_driver_need_over_the_ceiling_is_a_memory_error_before_any_retry():
    run, seen = _drive([[0, 40]], (5,), ceiling=39)
    with pytest.raises(MemoryError) as e:
        run()
    assert str(e.value) == "need [40]" and seen == [(5,)]
    run, seen = _drive([(2, 300)], (1, 500), _undercount, ceiling=100)   # any entry of the need counts, fitting or not
    with pytest.raises(MemoryError, match=r"need \[2, 300\]"):
        run()
    assert seen == [(1, 500)]


def test_driver_module_is_pure_python():
    import os
    src = open(os.path.join(os.path.dirname(search.__file__), "_retry.py")).read()
    assert "import torch" not in src and "_lib" not in src
