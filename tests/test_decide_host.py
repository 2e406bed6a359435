"""CPU: the decision masks' host side.  The boundary fixture of tests/decide_helpers.py has teeth (an fp32 evaluation gets
it wrong); the word packer round-trips against np.packbits; the Python argument checks raise before touching the library;
the C ABI's argument validation returns before any launch; the workspace holds no sort storage and does not grow with N;
include/mmr.h declares the new symbols and _lib.py binds them."""
import os

import numpy as np
import pytest
import torch

import decide_helpers as H

NEW_SYMBOLS = ("mmr_decide_workspace_bytes", "mmr_cosine_decide", "mmr_row_mask_combine", "mmr_decision_counts")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


def test_an_fp32_evaluation_fails_the_boundary_fixture(ref):
    """The failing control: numpy fp32 `q32 @ g32.T >= thr` disagrees with the oracle on at least K bits, so a rule that
    decides from an approximate dot cannot pass the GPU boundary test."""
    K = 16
    q, g, thr, rows = H.boundary_fixture(ref, 2000, 512, K, seed=5)
    qf, gf = H.f32(q), H.f32(g)
    want, redecided = H.oracle_bits(ref, qf, gf, thr)
    assert redecided >= 2 * K                                   # the planted pairs, at least, lie within the slack
    H.check_twins(want, rows)
    approx = (qf @ gf.T).astype(np.float64) >= thr[:, None]
    wrong = int((approx != want).sum())
    print(f"fp32 evaluation: {wrong} wrong bits of {want.size}, {redecided} pairs re-decided by the oracle")
    assert wrong >= K
    # and on the planted pairs themselves: one twin of (nearly) every pair
    twins_wrong = sum(int(approx[2 * k, r] != want[2 * k, r]) + int(approx[2 * k + 1, r] != want[2 * k + 1, r])
                      for k, r in enumerate(rows))
    assert twins_wrong >= K // 2


def test_the_packer_round_trips_against_packbits():
    rng = np.random.default_rng(0)
    for Q, N in ((1, 1), (3, 31), (2, 32), (5, 33), (4, 1000), (2, 10007)):
        bits = rng.random((Q, N)) < 0.4
        words = H.pack_bits(bits)
        W = (N + 31) // 32
        assert words.shape == (Q, W) and words.dtype == np.uint32
        padded = np.zeros((Q, W * 32), dtype=bool)
        padded[:, :N] = bits
        want = np.packbits(padded, axis=1, bitorder="little").view("<u4")
        assert np.array_equal(words, want)
        assert np.array_equal(H.unpack_words(words, N), bits)
        if N % 32:
            assert int(words[:, -1].max()) < (1 << (N % 32))    # pad bits clear
        # the package's own unpacking agrees
        from mmr_amd.search import DecisionMasks
        m = DecisionMasks(torch.from_numpy(words.view(np.int32).copy()), N)
        assert np.array_equal(m.to_bool().numpy(), bits)
        assert np.array_equal(m.row_mask(Q - 1).numpy(), bits[Q - 1])


def test_python_argument_errors_raise_before_any_launch():
    """Queries on the meta device: nothing could be launched even if a check were missing."""
    from mmr_amd import search

    q = torch.empty(3, 512, dtype=torch.bfloat16, device="meta")
    ok = search._check_decide_args(q, 512, [0.1, 0.2, 0.3])
    assert ok.dtype == torch.float64 and ok.tolist() == [0.1, 0.2, 0.3] and ok.device.type == "cpu"
    assert search._check_decide_args(q, 512, 0.25).tolist() == [0.25] * 3              # one number: every query's threshold
    assert search._check_decide_args(q, 512, torch.tensor(0.5)).tolist() == [0.5] * 3
    assert search._check_decide_args(q, 512, np.float64(0.1) + np.arange(3)).tolist() == [0.1, 1.1, 2.1]
    assert search._check_decide_args(q, 512, 0.1).tolist() == [0.1] * 3                # fp64, not rounded through fp32
    bad = [[0.1, 0.2], [0.1, 0.2, 0.3, 0.4], [[0.1, 0.2, 0.3]], [], float("nan"), float("inf"), [0.1, float("-inf"), 0.3],
           [0.1, float("nan"), 0.3], torch.tensor([0.1, float("inf"), 0.2]), [True, False, True], ["a", "b", "c"]]
    for thr in bad:
        with pytest.raises(ValueError):
            search._check_decide_args(q, 512, thr)
    with pytest.raises(ValueError):
        search._check_decide_args(torch.empty(3, 256, device="meta"), 512, 0.1)
    with pytest.raises(ValueError):
        search._check_decide_args(torch.empty(0, 512, device="meta"), 512, 0.1)
    with pytest.raises(RuntimeError):                           # a CPU gallery: there is no CPU path
        search.cosine_decide(torch.zeros(1, 512), torch.zeros(10, 512), 0.1)

    a = search.DecisionMasks(torch.zeros(2, 4, dtype=torch.int32), 100)
    for other in (search.DecisionMasks(torch.zeros(3, 4, dtype=torch.int32), 100),             # another Q
                  search.DecisionMasks(torch.zeros(2, 4, dtype=torch.int32), 101),             # another N, same words
                  search.DecisionMasks(torch.zeros(2, 5, dtype=torch.int32), 130),
                  torch.zeros(2, 4, dtype=torch.int32)):
        for op in (lambda x, y: x | y, lambda x, y: x & y, lambda x, y: x.andnot(y)):
            with pytest.raises(ValueError):
                op(a, other)
    with pytest.raises(ValueError):
        a.confusion(torch.zeros(99, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        a.confusion(torch.zeros(100, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        a.confusion(torch.zeros(100), torch.zeros(2, dtype=torch.int32))
    import mmr_amd
    assert mmr_amd.cosine_decide is search.cosine_decide and mmr_amd.DecisionMasks is search.DecisionMasks
    assert hasattr(search.GalleryIndex, "decide")


def test_confusion_metrics_share_the_sweeps_arithmetic():
    from mmr_amd.search import Confusion, ThresholdSweep

    tp, fp = np.array([30, 0, 7, 0]), np.array([10, 5, 0, 0])
    pos, neg = np.array([50, 0, 7, 12]), np.array([950, 100, 93, 88])
    t = torch.from_numpy
    c = Confusion(t(tp), t(fp), t(pos), t(neg))
    assert torch.equal(c.fn, t(pos - tp)) and torch.equal(c.tn, t(neg - fp))
    sweep = ThresholdSweep(torch.tensor([0.5], dtype=torch.float64), t(np.stack([fp, tp], 1)[:, :, None]), t(np.stack([neg, pos], 1)))
    for mine, theirs in zip(c.metrics(), sweep.metrics()):
        assert mine.shape == (4,) and np.array_equal(mine, theirs[:, 0])
    p, r, f1 = c.metrics()
    assert p.tolist() == [0.75, 0.0, 1.0, 0.0] and r.tolist() == [0.6, 0.0, 1.0, 0.0] and f1[2] == 1.0 and f1[3] == 0.0


def test_header_declares_and_lib_binds_the_new_symbols(lib):
    names = set(lib.HEADER.functions)
    L = lib.lib()
    for n in NEW_SYMBOLS:
        assert n in names, n
        f = getattr(L, n)
        assert f.argtypes is not None, n                        # bound with a signature, not ctypes' int default
    assert L.mmr_decide_workspace_bytes.restype is not None


def _decide(L, *, q=16, gallery=16, hi=None, dtype=1, Q=4, N=100, E=512, thr=16, bound=1.0, mask=None, cand_cap=8, out=16,
            counts=16, ws=16, ws_bytes=1 << 30):
    """Device pointers are fake (16): every call here must return from the host checks, which never dereference them."""
    return L.mmr_cosine_decide(q, gallery, hi, dtype, Q, N, E, thr, bound, None, None, mask, cand_cap, out, counts, ws,
                               ws_bytes, 0)


def test_argument_validation_happens_before_any_launch(lib):
    L = lib.lib()
    err = lambda: L.mmr_last_error()
    for null in ("q", "thr", "gallery", "out", "counts", "ws"):
        assert _decide(L, **{null: None}) == -22 and b"null pointer" in err(), null
    assert _decide(L, E=100) == -95 and b"E=100" in err()
    assert _decide(L, dtype=7) == -22 and b"dtype" in err()
    assert _decide(L, Q=0) == -22 and b"Q=0" in err()
    assert _decide(L, N=-1) == -22 and _decide(L, N=1 << 31) == -22
    assert _decide(L, cand_cap=0) == -22 and b"cand_cap" in err()
    assert _decide(L, bound=float("inf")) == -22 and b"gallery_norm_bound" in err()
    assert _decide(L, bound=float("nan")) == -22
    assert _decide(L, ws_bytes=8) == -28 and b"workspace" in err()
    assert _decide(L, mask=18) == -22 and b"row_mask" in err()
    assert _decide(L, q=24) == -22 and b"16-byte" in err()
    assert _decide(L, thr=20) == -22 and b"8-byte" in err()
    assert _decide(L, out=18) == -22 and b"4-byte" in err()
    assert b"mmr_cosine_decide" in err()

    assert L.mmr_row_mask_combine(16, 16, 3, 10, 16, 0) == -22 and b"op=3" in err()
    assert L.mmr_row_mask_combine(16, 16, 0, -1, 16, 0) == -22
    assert L.mmr_row_mask_combine(None, 16, 0, 10, 16, 0) == -22 and b"null pointer" in err()
    assert L.mmr_row_mask_combine(16, 18, 0, 10, 16, 0) == -22 and b"4-byte" in err()
    assert L.mmr_row_mask_combine(None, None, 1, 0, None, 0) == 0                          # nothing to do

    assert L.mmr_decision_counts(16, 2, -1, None, None, None, 16, 0) == -22
    assert L.mmr_decision_counts(16, -1, 100, None, None, None, 16, 0) == -22
    assert L.mmr_decision_counts(16, 2, 100, None, None, None, None, 0) == -22 and b"null pointer" in err()
    assert L.mmr_decision_counts(None, 2, 100, None, None, None, 16, 0) == -22 and b"null pointer" in err()
    assert L.mmr_decision_counts(16, 2, 100, 16, None, None, 16, 0) == -22 and b"targets" in err()
    assert L.mmr_decision_counts(16, 2, 100, None, None, 18, 16, 0) == -22 and b"row_mask" in err()
    assert L.mmr_decision_counts(16, 2, 100, None, None, None, 20, 0) == -22 and b"8-byte" in err()
    assert L.mmr_decision_counts(None, 0, 100, None, None, None, None, 0) == 0             # nothing to do


def test_workspace_has_no_sort_storage_and_does_not_grow_with_n(lib):
    L = lib.lib()
    f, r = L.mmr_decide_workspace_bytes, L.mmr_range_workspace_bytes
    cap = 1 << 16
    base = f(1000, 512, 10, cap, 1, 0)
    assert 0 < base <= cap * 8 + 4096                           # the candidate list and fixed scalars: 8 bytes per pair
    assert f(1_000_000, 512, 10, cap, 1, 0) == base == f(0, 512, 300, cap, 2, 1)
    assert r(1000, 512, 10, cap, 1, 0) >= 4 * cap * 8 > base    # range search keeps four 8-byte arrays and sort storage
    assert f(1000, 512, 10, 2 * cap, 1, 0) == base + cap * 8
    # fp32: the bf16 queries and their residuals; a pre-split hi half keeps it independent of N
    given = f(1000, 512, 10, cap, 0, 1)
    assert base < given <= base + 10 * 512 * 2 + 512 and f(1_000_000, 512, 10, cap, 0, 1) == given
    assert f(1000, 512, 10, cap, 0, 0) == given + 1000 * 512 * 2
    for bad in ((-1, 512, 10, 8, 1, 0), (10, 512, -1, 8, 1, 0), (10, 512, 10, 0, 1, 0), (10, 512, 10, 8, 3, 0)):
        assert f(*bad) == 0, bad
