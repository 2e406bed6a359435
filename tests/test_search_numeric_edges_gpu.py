"""GPU: the search family (top-k, range search, self-join, masked forms, merge) at the numeric edges -- non-finite
rows and queries, total ties, power-of-two scales, the k and merge limits.

The contract under test is the paragraph "Non-finite values, ties and scale" of include/mmr.h:
a pair whose exact dot64 is NaN is absent; +inf / -inf are ordinary numbers; ties go to the lowest row id; results are
exact at every scale of finite inputs.  Expected values come from oracle/search_ref.c (top-k: the oracle over the
compacted gallery, ids mapped back; range / join: brute force, search_helpers.py) and are compared bit for bit
(``equal_nan`` where an output may hold a NaN).  Every case runs for a bf16 gallery, an fp32 gallery per call and an fp32
GalleryIndex with the pre-split hi / lo halves, and again under a random 50 % row mask."""
import functools
import itertools

import numpy as np
import pytest
import torch

from mmr_amd import synth
from search_helpers import assert_topk, expect_topk, oracle_join, oracle_range, plan_tpt, to_np

pytestmark = pytest.mark.gpu

FORMS = ("bf16", "f32", "f32-index")
SIZES = tuple(itertools.product((4097, 20011), (5, 70)))      # ragged tiles; one and three 32-query blocks
K = 10
NAN = float("nan")


@pytest.fixture(scope="module")
def S(device):
    from mmr_amd import search
    return search


@pytest.fixture(scope="module")
def oracle():
    from oracle import search_ref
    return search_ref


@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


def _dtype(form):
    return torch.bfloat16 if form == "bf16" else torch.float32


def _same(a, b, what=""):
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), what


class _Run:
    """One gallery on the device, searched the way ``form`` says: per call (bf16, f32) or through a pre-split index."""

    def __init__(self, S, device, form, g):
        self.S, self.device, self.form = S, device, form
        self.gd = g.to(device)
        self._ix = None

    def index(self, fresh=False):
        if fresh:
            return self.S.GalleryIndex(self.gd, presplit=self.form == "f32-index")
        if self._ix is None:
            self._ix = self.S.GalleryIndex(self.gd, presplit=self.form == "f32-index")
        return self._ix

    def _mask(self, mask):
        return None if mask is None else torch.from_numpy(mask).to(self.device)

    def topk(self, q, k, mask=None, scale=1.0, path=None, norm_bound=None):
        """-> (score, idx, dot64, status).  path: None = the form's own, "index" / "call" force one"""
        qd = q.to(self.device)
        if path == "index" or (path is None and self.form == "f32-index"):
            return self.index().search(qd, k, scale, return_dot64=True, return_status=True, row_mask=self._mask(mask))
        return self.S.cosine_topk(qd, self.gd, k, scale, gallery_norm_bound=norm_bound, return_dot64=True,
                                  return_status=True, row_mask=self._mask(mask))

    def range(self, q, tau, mask=None, path=None):
        qd = q.to(self.device)
        if path == "index" or (path is None and self.form == "f32-index"):
            return self.index().range_search(qd, tau, return_dot64=True, row_mask=self._mask(mask))
        return self.S.cosine_range(qd, self.gd, tau, return_dot64=True, row_mask=self._mask(mask))

    def join(self, tau, mask=None, path=None):
        if path == "index" or (path is None and self.form == "f32-index"):
            return self.index().near_duplicates(tau, row_mask=self._mask(mask))
        return self.S.gallery_self_join(self.gd, tau, row_mask=self._mask(mask))


def _assert_range(res, Q, want, what=""):
    off, idx, score, d64 = res
    off = off.cpu().numpy()
    wq, wr, wd = want
    assert off.shape == (Q + 1,) and off[0] == 0 and off[-1] == idx.numel() == score.numel() == d64.numel(), what
    assert np.array_equal(np.repeat(np.arange(Q), np.diff(off)), wq) and np.array_equal(idx.cpu().numpy(), wr), what
    assert np.array_equal(d64.cpu().numpy().view(np.int64), wd.view(np.int64)), what
    with np.errstate(over="ignore", under="ignore"):
        assert np.array_equal(score.cpu().numpy(), wd.astype(np.float32)), what


def _assert_join(res, want, what=""):
    a, b, score, d64 = res
    wa, wb, wd = want
    assert np.array_equal(a.cpu().numpy(), wa) and np.array_equal(b.cpu().numpy(), wb), what
    assert np.array_equal(d64.cpu().numpy().view(np.int64), wd.view(np.int64)), what
    with np.errstate(over="ignore", under="ignore"):
        assert np.array_equal(score.cpu().numpy(), wd.astype(np.float32)), what


def _kth_largest(s, n):
    """the n-th largest finite value of an array"""
    v = s[np.isfinite(s)]
    return float(np.partition(v, v.size - n)[v.size - n])


# =================================================================== A. NaN rows: poison that must vanish
def _cold_block(N):
    """rows of one whole scan tile and of one whole scan task, for the bf16 plan (32-row tiles) and the fp32 plan (16)"""
    rows = set()
    for dt in (torch.bfloat16, torch.float32):
        tr, tpt = plan_tpt(N, dt)
        t = (N // tr) // 2
        rows.update(range(t * tr, (t + 1) * tr))
        rows.update(range(tr * tpt, 2 * tr * tpt))          # task 1
    return np.array(sorted(r for r in rows if r < N))


@functools.lru_cache(maxsize=4)
def _nan_case(bf16, E, N, Q):
    """The tie-free synthetic gallery, the poisons (i)-(vi) and, per poison, the oracle over the rows that stay.
    The rows of the cold block are shrunk by 1/4 (exact) so that a whole tile and a whole task lie outside every
    query's top-40: poisoning them cannot change a k-th value (K = 10), which is what the status relation needs."""
    from oracle import search_ref
    dtype = torch.bfloat16 if bf16 else torch.float32
    g = synth.synth_unit_rows(N, E, seed=1000 + N + E).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=2000 + Q + E).to(dtype)
    cold = _cold_block(N)
    g[cold] = g[cold] * 0.25
    top40 = search_ref.cosine_topk(q, g, 40)[0]
    hot = set(top40.ravel().tolist())
    assert not hot & set(cold.tolist()), "the cold block must lie outside every query's top-40"
    free = [r for r in range(N // 3, N) if r not in hot and r not in set(cold.tolist())]
    rng = np.random.default_rng(N + E)
    poisons = {                                               # name -> (rows, column or None = the whole row)
        "i": (np.array([free[0]]), None),
        "ii": (np.array([free[1]]), 7),
        "iii": (cold, None),
        "iv": (np.unique(top40[:, 0]), None),
        "v": (np.arange(K), None),
        "vi": (np.setdiff1d(np.arange(N), rng.choice(N, 7, replace=False)), None),
    }
    mask50 = rng.random(N) < 0.5
    want = {}
    for name, (rows, _) in poisons.items():
        keep = np.ones(N, bool)
        keep[rows] = False
        want[name, False] = expect_topk(search_ref, q, g, keep, K)
        want[name, True] = expect_topk(search_ref, q, g, keep & mask50, K)
    return g, q, poisons, mask50, want


def _poisoned(g, rows, col):
    gp = g.clone()
    if col is None:
        gp[rows] = NAN
    else:
        gp[rows, col] = NAN
    return gp


@pytest.mark.parametrize("form", FORMS)          # the form varies fastest: f32 and f32-index share one cached case
@pytest.mark.parametrize("E", [128, 512, 768])
def test_nan_rows_are_absent_from_topk(S, device, form, E):
    """A(i)-(vi): the poisoned gallery returns what the gallery without those rows returns; masking or deleting the
    poisoned rows changes nothing, status included; poison outside every top-40 never costs a query its fast path;
    the measured norm bound is the clean rows'."""
    for N, Q in SIZES:
        g, q, poisons, mask50, want = _nan_case(form == "bf16", E, N, Q)
        clean = _Run(S, device, form, g)
        st_clean = {m: clean.topk(q, K, mask50 if m else None)[3].cpu().numpy() for m in (False, True)}
        for name, (rows, col) in poisons.items():
            what = (form, E, N, Q, name)
            run = _Run(S, device, form, _poisoned(g, rows, col))
            got = {}
            for masked in (False, True):
                got[masked] = run.topk(q, K, mask50 if masked else None)
                assert_topk(got[masked], want[name, masked])
                if name in ("i", "ii", "iii"):
                    st = got[masked][3].cpu().numpy()
                    print("status", what, "masked" if masked else "", "poisoned", st.tolist(), "clean", st_clean[masked].tolist())
                    assert (st <= st_clean[masked]).all(), what
            keep = np.ones(N, bool)
            keep[rows] = False
            if name in ("i", "ii", "iii"):
                _same(got[False], run.topk(q, K, keep), what)                    # masked out: identical, status too
                ix = run.index(fresh=True)
                ix.delete_rows(torch.from_numpy(rows))
                _same(got[False], ix.search(q.to(device), K, return_dot64=True, return_status=True), what)
            true_max = float(g.double().norm(dim=-1)[torch.from_numpy(keep)].max())
            nb = float(S.gallery_norm_bound(run.gd))
            assert true_max <= nb <= true_max * 1.001, (what, nb, true_max)


@pytest.mark.parametrize("E", [128, 512, 768])
@pytest.mark.parametrize("form", FORMS)
def test_nan_rows_never_match_in_range_search_or_self_join(S, ref, device, form, E):
    """A, range side: cosine_range / gallery_self_join / GalleryIndex.range_search / .near_duplicates / .dedup on
    poisoned galleries at thresholds with a few hundred matches: the brute-force pairs, same order, same bits."""
    from mmr_amd import dedup
    dtype = _dtype(form)
    for N, Q, join in ((4097, 70, True), (20011, 5, False)):
        g = synth.synth_unit_rows(N, E, seed=3000 + N + E).to(dtype)
        q = synth.synth_unit_rows(Q, E, seed=4000 + Q + E).to(dtype)
        gn, qn = to_np(g), to_np(q)
        s = qn.astype(np.float64) @ gn.astype(np.float64).T
        tau = _kth_largest(s, 300)
        mask50 = np.random.default_rng(E + N).random(N) < 0.5
        cq, cr, _ = oracle_range(ref, qn, gn, tau)
        poisons = {"i+ii": ([N // 2 + 3], [(N // 2 + 40, 7)]), "iii": (_cold_block(N).tolist(), []),
                   "matched": (np.unique(cr[:40]).tolist(), [])}
        if join:
            g64 = gn.astype(np.float64)
            tau_j = _kth_largest(np.triu(g64 @ g64.T, 1) + np.tril(np.full((N, N), -np.inf)), 300)
            ja, jb, _ = oracle_join(ref, gn, tau_j)
            poisons["matched"] = (np.unique(np.concatenate([cr[:40], ja[:20], jb[-20:]])).tolist(), [])
        for name, (rows, elems) in poisons.items():
            gp = g.clone()
            gp[rows] = NAN
            for r, c in elems:
                gp[r, c] = NAN
            dead = set(rows) | {r for r, _ in elems}
            gpn = to_np(gp)
            run = _Run(S, device, form, gp)
            for masked in (False, True):
                mask = mask50 if masked else None
                what = (form, E, N, name, masked)
                want = oracle_range(ref, qn, gpn, tau, mask)
                assert 50 < want[0].size and not dead & set(want[1].tolist())
                _assert_range(run.range(q, tau, mask), Q, want, what)
                _assert_range(run.range(q, tau, mask, path="index"), Q, want, what)
                if join:
                    wj = oracle_join(ref, gpn, tau_j, mask)
                    assert 20 < wj[0].size and not dead & (set(wj[0].tolist()) | set(wj[1].tolist()))
                    _assert_join(run.join(tau_j, mask), wj, what)
                    _assert_join(run.join(tau_j, mask, path="index"), wj, what)
            if join:
                wj = oracle_join(ref, gpn, tau_j)
                keep, dup = dedup.keep_first(N, torch.from_numpy(wj[0]), torch.from_numpy(wj[1]))
                dropped, partner = run.index(fresh=True).dedup(tau_j)
                assert np.array_equal(dropped.cpu().numpy(), np.flatnonzero(~keep))
                assert np.array_equal(partner.cpu().numpy(), dup[~keep])
                assert dropped.numel() > 0 and not dead & set(dropped.tolist()) and not dead & set(partner.tolist())


# =================================================================== B. NaN / Inf elsewhere
@pytest.mark.parametrize("E", [128, 512, 768])
@pytest.mark.parametrize("form", FORMS)
def test_nan_query_gets_empty_slots_and_leaves_its_neighbours_alone(S, device, form, E):
    dtype = _dtype(form)
    for (N, Q), j in zip(((4097, 5), (20011, 70)), (2, 45)):
        g = synth.synth_unit_rows(N, E, seed=5000 + N + E).to(dtype)
        q = synth.synth_unit_rows(Q, E, seed=6000 + Q + E).to(dtype)
        qp = q.clone()
        qp[j, E - 3] = NAN
        mask50 = np.random.default_rng(E).random(N) < 0.5
        run = _Run(S, device, form, g)
        others = [i for i in range(Q) if i != j]
        for mask in (None, mask50):
            a, b = run.topk(q, K, mask), run.topk(qp, K, mask)
            assert (b[1][j] == -1).all() and torch.isneginf(b[0][j]).all() and torch.isneginf(b[2][j]).all()
            assert int(b[3][j]) in (0, 1)
            _same([x[others] for x in a], [x[others] for x in b], (form, E, N, "neighbours of the NaN query"))
            tau = _kth_largest(to_np(q).astype(np.float64) @ to_np(g).astype(np.float64).T, 300)
            ra, rb = run.range(q, tau, mask), run.range(qp, tau, mask)
            oa, ob = ra[0].cpu().numpy(), rb[0].cpu().numpy()
            assert ob[j + 1] == ob[j], "a NaN query matches nothing"
            for i in others:
                for x, y in zip(ra[1:], rb[1:]):
                    assert torch.equal(x[oa[i]:oa[i + 1]], y[ob[i]:ob[i + 1]])


def _inf_case(dtype, N, E, Q, seed):
    """row R holds +inf in column C; the queries' element there is 0, > 0, < 0 (dot NaN, +inf, -inf); query 3 is all-zero"""
    R, C = N // 4, 17
    g = synth.synth_unit_rows(N, E, seed=seed).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=seed + 1).to(dtype)
    g[R, C] = float("inf")
    q[0, C], q[1, C], q[2, C] = 0.0, 0.125, -0.125
    q[3] = 0.0
    return g, q, R


@pytest.mark.parametrize("E", [128, 512, 768])
@pytest.mark.parametrize("form", FORMS)
def test_infinite_gallery_element_topk(S, oracle, device, form, E):
    """+inf ranks first, -inf last but present, NaN absent, per query; the measured bound is +inf and every query takes
    the exhaustive path and is still exact."""
    for N, Q in ((4097, 5), (20011, 70)):
        g, q, R = _inf_case(_dtype(form), N, E, Q, 7000 + N + E)
        run = _Run(S, device, form, g)
        assert float(S.gallery_norm_bound(run.gd)) == float("inf")
        got = run.topk(q, K, scale=100.0)
        assert_topk(got, expect_topk(oracle, q, g, np.ones(N, bool), K, scale=100.0))
        idx, d64 = got[1].cpu().numpy(), got[2].cpu().numpy()
        assert R not in idx[0] and idx[1, 0] == R and d64[1, 0] == np.inf and float(got[0][1, 0]) == np.inf
        assert R not in idx[2] and idx[3].tolist() == list(range(K)) and not np.signbit(d64[3]).any()
        assert (got[3] == 1).all(), "an infinite measured bound leaves no query on the fast path"
        few = np.zeros(N, bool)                               # 6 live rows, R among them: k = 10 reaches the -inf row
        few[[3, 77, R, N - 900, N - 31, N - 1]] = True
        mask50 = np.random.default_rng(E).random(N) < 0.5
        mask50[R] = True
        got = run.topk(q, K, mask50)
        assert_topk(got, expect_topk(oracle, q, g, mask50, K))
        assert (got[3] == 1).all()
        got = run.topk(q, K, few)             # (no excluded live tile: the bound is -inf and the fast path may certify)
        assert_topk(got, expect_topk(oracle, q, g, few, K))
        idx, d64 = got[1].cpu().numpy(), got[2].cpu().numpy()
        assert idx[2, 5] == R and d64[2, 5] == -np.inf and (idx[2, 6:] == -1).all()        # -inf: returned, with its id
        assert R not in idx[0] and (idx[0, 5:] == -1).all() and idx[1, 0] == R


@pytest.mark.parametrize("E", [128, 512, 768])
@pytest.mark.parametrize("form", FORMS)
def test_infinite_gallery_element_range_and_join(S, ref, device, form, E):
    """With an infinite measured bound every non-NaN pair is a candidate: N * Q fits the default candidate capacity for
    range search, the self-join needs (exactly) the wrapper's one retry.  A zero query still matches every finite row
    at a threshold <= 0 (its margin 8e-5 * 0 * inf must not poison the candidate threshold)."""
    N, Q = 4096, 8
    g, q, R = _inf_case(_dtype(form), N, E, Q, 8000 + E)
    gn, qn = to_np(g), to_np(q)
    with np.errstate(invalid="ignore"):
        s = qn.astype(np.float64) @ gn.astype(np.float64).T
    tau = _kth_largest(s, 300)
    run = _Run(S, device, form, g)
    mask50 = np.random.default_rng(E).random(N) < 0.5
    mask50[R] = True
    for mask in (None, mask50):
        want = oracle_range(ref, qn, gn, tau, mask)
        assert R in want[1][want[0] == 1] and R not in want[1][np.isin(want[0], (0, 2, 3))]      # +inf; NaN, -inf, zero query
        for path in (None, "index"):
            _assert_range(run.range(q, tau, mask, path=path), Q, want, (form, E, path))
        # the zero query (and query 0, whose dot with row R is NaN) at thresholds 0.0 and -0.0
        qz, qzn = q[[3, 0]], qn[[3, 0]]
        for t0 in (0.0, -0.0):
            want = oracle_range(ref, qzn, gn, t0, mask)
            live = N - 1 if mask is None else int(mask.sum()) - 1
            assert int((want[0] == 0).sum()) == live and R not in want[1]
            for path in (None, "index"):
                _assert_range(run.range(qz, t0, mask, path=path), 2, want, (form, E, path, "zero query"))
    N2 = 2048
    g2 = g[:N2]
    g2n = gn[:N2]
    g64 = g2n.astype(np.float64)
    with np.errstate(invalid="ignore"):
        sj = np.triu(g64 @ g64.T, 1) + np.tril(np.full((N2, N2), -np.inf))
    tau_j = _kth_largest(sj, 300)
    run2 = _Run(S, device, form, g2)
    for mask in (None, mask50[:N2]):
        want = oracle_join(ref, g2n, tau_j, mask)
        assert ((want[0] == R) | (want[1] == R)).sum() > 100         # the +inf dots match
        for path in (None, "index"):
            _assert_join(run2.join(tau_j, mask, path=path), want, (form, E, path))


@pytest.mark.parametrize("E", [128, 512, 768, 1024])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_similarity_propagates_non_finite_values_like_the_oracle(S, oracle, device, dtype, E):
    N, Q = 777, 6
    g = (synth.synth_unit_rows(N, E, seed=E) * 3.0).to(dtype)
    q = (synth.synth_unit_rows(Q, E, seed=E + 1) * 0.5).to(dtype)
    g[5] = NAN
    g[6, 9] = NAN
    g[100, 17] = float("inf")
    g[101, 17] = float("-inf")
    g[102, 17], g[102, 18] = float("inf"), float("-inf")
    g[776, E - 1] = float("inf")
    q[0, 17], q[1, 17], q[2, 17] = 0.0, 0.125, -0.125
    q[3] = 0.0
    q[4, E - 1] = NAN
    sim = S.similarity(g.to(device), q.to(device), 100.0)            # [N,Q]
    want = oracle.similarity(q, g, 100.0)                            # [Q,N]
    assert np.isnan(want[:, 5]).all() and np.isnan(want[4]).all() and want[1, 100] == np.inf and want[2, 100] == -np.inf
    assert np.isnan(want[0, 100]) and np.isfinite(want[:4, 200:776]).all()
    assert np.array_equal(sim.t().cpu().numpy(), want, equal_nan=True)


@pytest.mark.parametrize("form", FORMS)
def test_l2_normalize_of_a_zero_row_is_nan_and_the_search_drops_it(S, oracle, device, form):
    """The reference's 0/0: a blank gallery slot becomes a NaN row; its neighbours in the same 4-row workgroup are
    untouched, and every later search treats the row as absent (case A(i) on the normalised gallery)."""
    N, E, Z = 4097, 512, 1001                                  # rows 1000..1003 share a workgroup
    dtype = _dtype(form)
    x = (synth.synth_unit_rows(N, E, seed=91) * 4.0).to(dtype)
    xz = x.clone()
    xz[Z] = 0.0
    y0, y = S.l2_normalize(x.to(device)), S.l2_normalize(xz.to(device))
    assert torch.isnan(y[Z]).all() and np.isnan(oracle.l2norm_rows(xz[Z:Z + 1])).all()
    keep = np.ones(N, bool)
    keep[Z] = False
    _same([y[torch.from_numpy(keep).to(device)]], [y0[torch.from_numpy(keep).to(device)]])
    q = synth.synth_unit_rows(37, E, seed=92).to(dtype)
    q[0] = y0[Z].cpu()                                         # the blank slot would have been this query's best hit
    run = _Run(S, device, form, y.cpu())
    mask50 = np.random.default_rng(1).random(N) < 0.5
    for mask in (None, mask50):
        got = run.topk(q, K, mask)
        assert_topk(got, expect_topk(oracle, q, y.cpu(), keep if mask is None else keep & mask, K))
        assert Z not in got[1].cpu().numpy()


# =================================================================== C. total ties
@pytest.mark.parametrize("E", [128, 512, 768])
@pytest.mark.parametrize("form", FORMS)
def test_zero_query_ties_with_every_row(S, ref, device, form, E):
    """Every dot64 is exactly +0.0: rows 0..k-1 (under a mask the first k live rows), the margin is 0 and the k-th value
    equals the bound, so the query takes the exhaustive path; range search at 0.0 / -0.0 matches all N rows
    (inclusive rule), at the next double above 0 none."""
    dtype = _dtype(form)
    for N in (4097, 20011):
        g = synth.synth_unit_rows(N, E, seed=9000 + N + E).to(dtype)      # random signs
        q = synth.synth_unit_rows(5, E, seed=9100 + E).to(dtype)
        q[1] = 0.0
        q[3] = -0.0
        run = _Run(S, device, form, g)
        mask50 = np.random.default_rng(N).random(N) < 0.5
        for mask in (None, mask50):
            score, idx, d64, status = run.topk(q, K, mask)
            first = np.arange(K) if mask is None else np.flatnonzero(mask)[:K]
            for j in (1, 3):
                assert np.array_equal(idx[j].cpu().numpy(), first)
                assert (d64[j].cpu().numpy().view(np.int64) == 0).all(), "dot64 must be +0.0, bit for bit"
                assert (score[j].cpu().numpy().view(np.int32) == 0).all()
                assert int(status[j]) == 1
            live = N if mask is None else int(mask.sum())
            qz = q[[1, 3]]
            for t0 in (0.0, -0.0):
                off, ridx, rscore, rd = run.range(qz, t0, mask)
                assert off.tolist() == [0, live, 2 * live]
                rows = np.arange(N) if mask is None else np.flatnonzero(mask)
                assert np.array_equal(ridx.cpu().numpy(), np.concatenate([rows, rows]))
                assert (rd.cpu().numpy().view(np.int64) == 0).all()
            assert run.range(qz, float(np.nextafter(0.0, 1.0)), mask)[0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("form,E", [("bf16", 128), ("bf16", 512), ("bf16", 768), ("f32", 512), ("f32-index", 512)])
def test_gallery_of_identical_rows(S, oracle, device, form, E):
    """N = 50 000 copies of one row: every tile maximum is equal, the answer is rows 0..k-1; with one better row planted
    in the last tile [planted, 0, 1, ...].  Queries: exact copies of the row, and an unrelated one."""
    N = 50000
    dtype = _dtype(form)
    row = synth.synth_unit_rows(1, E, seed=77 + E).to(dtype)
    q = synth.synth_unit_rows(4, E, seed=78 + E).to(dtype)
    q[0] = row[0]
    q[2] = row[0]
    g = row.repeat(N, 1).contiguous()
    mask50 = np.random.default_rng(E).random(N) < 0.5
    for planted in (None, N - 3):
        if planted is not None:
            g = g.clone()
            g[planted] = row[0] * 2.0                          # beats every copy for the queries that are copies
            mask50[planted] = True
        run = _Run(S, device, form, g)
        for mask in (None, mask50):
            got = run.topk(q, K, mask)
            assert_topk(got, expect_topk(oracle, q, g, np.ones(N, bool) if mask is None else mask, K))
            live = np.arange(N) if mask is None else np.flatnonzero(mask)
            want0 = live[:K] if planted is None else np.concatenate([[planted], live[:K - 1]])
            assert np.array_equal(got[1][0].cpu().numpy(), want0) and np.array_equal(got[1][2].cpu().numpy(), want0)


# =================================================================== D. power-of-two scales
SCALES = ((-60, 0), (0, -60), (-60, -60), (-30, -30), (40, 0), (70, 0), (60, 60))
NORMAL_RANGE = tuple(s for s in SCALES if s not in ((-60, -60), (70, 0)))    # products, sums of squares, dots stay normal fp32
# beyond the issue's list: squares of the rows / queries / split residuals are far below fp32's range (a norm measured in
# fp32 would be 0 and the margin with it), products and sums are subnormal or quantised to nothing, and net scales of
# 2^0 and 2^-15 reached from both ends.  All values stay normal numbers of their dtype (checked by _scaled).
FAR_SCALES = ((-90, 0), (0, -90), (-70, -70), (-90, 90), (-75, 60))


def _scaled(x, e):
    """x * 2^e, checked exact on the host: finite, non-zero where x was, and scaling back gives x"""
    y = (x.float() * (2.0 ** e)).to(x.dtype)
    assert torch.isfinite(y).all() and bool(((y != 0) == (x != 0)).all())
    assert torch.equal(y.double() * (2.0 ** -e), x.double())
    return y


def _near_tie_gallery():
    """the construction of test_uncertified_queries_fall_back_to_exact (test_search_gpu.py): 60 rows within a few bf16 ulps
    of row 5 straddle the top-k boundary of query 0"""
    torch.manual_seed(0)
    E = 512
    gal = synth.synth_unit_rows(8192, E, seed=21).bfloat16()
    base = gal[5].clone()
    rows = torch.randperm(8192)[:60]
    for j, r in enumerate(rows.tolist()):
        v = base.clone()
        v.view(torch.int16)[j] += (j % 5) - 2
        gal[r] = v
    q = base.unsqueeze(0).repeat(2, 1)
    q[1] = synth.synth_unit_rows(1, E, seed=22).bfloat16()[0]
    return gal, q


def _scale_topk_checks(S, oracle, device, form, g, q, k, scale, crowded, scales=SCALES):
    """idx equal to the unscaled oracle's, dot64 == ldexp(dot64, a + b), score per the oracle, and the status rules"""
    oi, _, od = oracle.cosine_topk(q, g, k, scale=scale)
    nb0 = float(np.float32(float(g.double().norm(dim=-1).max()) * 1.000001))      # an honest host bound (fp32, rounded up)
    paths = ("index",) if form == "f32-index" else ("call", "host", "index")
    base = _Run(S, device, form, g)
    st0 = {}
    for path in paths:
        got = base.topk(q, k, scale=scale, path="index" if path == "index" else "call", norm_bound=nb0 if path == "host" else None)
        assert_topk(got, oracle.cosine_topk(q, g, k, scale=scale))
        st0[path] = got[3].cpu().numpy()
    for a, b in scales:
        gs, qs = _scaled(g, a), _scaled(q, b)
        wd = np.ldexp(od, a + b)
        with np.errstate(over="ignore", under="ignore"):
            ws = (wd * np.float64(np.float32(scale))).astype(np.float32)
        run = _Run(S, device, form, gs)
        for path in paths:
            what = (form, g.shape, q.shape[0], k, (a, b), path)
            got = run.topk(qs, k, scale=scale, path="index" if path == "index" else "call",
                           norm_bound=float(np.ldexp(np.float32(nb0), a)) if path == "host" else None)
            assert_topk(got, (oi, ws, wd))
            st = got[3].cpu().numpy()
            print("status", what, st.tolist(), "unscaled", st0[path].tolist())
            if crowded is not None:
                assert st[crowded] == 1, what
            if (a, b) == (70, 0) and path != "host" and g.shape[0] > 32 * 32:
                # (up to 32 candidate tiles of 32 rows: a smaller gallery leaves no tile out, its certificate is vacuous)
                assert (st == 1).all(), (what, "the fp32 sum of squares overflows: the measured bound is +inf")
            if (a, b) in NORMAL_RANGE:
                assert np.array_equal(st, st0[path]), (what, "every fp32 quantity of the scan and the margin scales exactly")


@pytest.mark.parametrize("E", [128, 512, 768])
@pytest.mark.parametrize("form", FORMS)
def test_power_of_two_scales_topk(S, oracle, device, form, E):
    """the fixture of test_topk_vs_oracle_shapes, gallery * 2^a, queries * 2^b"""
    dtype = _dtype(form)
    for N, Q, k in [(1, 1, 1), (31, 3, 5), (33, 2, 10), (4097, 37, 10), (20011, 70, 20), (3000, 5, 30)]:
        g = synth.synth_unit_rows(N, E, seed=100 + N).to(dtype)
        q = synth.synth_unit_rows(Q, E, seed=200 + Q).to(dtype)
        _scale_topk_checks(S, oracle, device, form, g, q, k, 100.0, None)


@pytest.mark.parametrize("form", FORMS)
def test_power_of_two_scales_crowded_boundary(S, oracle, device, form):
    g, q = _near_tie_gallery()
    _scale_topk_checks(S, oracle, device, form, g.to(_dtype(form)), q.to(_dtype(form)), K, 1.0, 0, SCALES + FAR_SCALES)


def _ladder(gal, q, qis, step, first_row, seed):
    """test_filtered_search_gpu.py's ladder: for each query 40 unit rows at cosine 0.9, 0.9 - step, ... in 40 different
    tiles; step 1e-4 is below the bf16 tier's resolution (needs the three-product tier), 1e-6 needs the exhaustive one"""
    N, E = gal.shape
    stride = (N - 200) // 40
    w = synth.synth_unit_rows(40, E, seed=seed).double()
    c = 0.9 - step * torch.arange(40, dtype=torch.float64)
    for j, qi in enumerate(qis):
        u = (q[qi] / q[qi].norm()).bfloat16().double()
        q[qi] = u.float()
        u /= u.norm()
        wj = w - (w @ u).unsqueeze(1) * u
        wj /= wj.norm(dim=1, keepdim=True)
        rows = [first_row + 7 * j + stride * t for t in range(40)]
        gal[rows] = (c.unsqueeze(1) * u + (1 - c * c).sqrt().unsqueeze(1) * wj).float()


@pytest.mark.parametrize("form", ["f32", "f32-index"])
def test_power_of_two_scales_split_tiers(S, oracle, device, form):
    """fp32 rows that are not bf16 values, with ladders only the second tier (1e-4) or the exhaustive tier (1e-6) can
    order: the measured residuals |q - bf16(q)| and max_row |g - hi| are part of the first tier's margin and must
    scale with the data instead of underflowing."""
    N, E, Q = 20000, 256, 8
    g = synth.synth_unit_rows(N, E, seed=31)
    q = synth.synth_unit_rows(Q, E, seed=32)
    _ladder(g, q, [0, 3], 1e-4, 100, 33)
    _ladder(g, q, [2, 5], 1e-6, 50, 34)
    _scale_topk_checks(S, oracle, device, form, g, q, K, 1.0, None, SCALES + FAR_SCALES)


@pytest.mark.parametrize("E", [128, 768])
@pytest.mark.parametrize("form", FORMS)
def test_power_of_two_scales_range_and_join(S, ref, device, form, E):
    """thresholds scaled by 2^(a+b) (2^(2a) for the self-join): the same pairs, every dot64 scaled exactly"""
    N, Q = 4097, 37
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=100 + N).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=200 + Q).to(dtype)
    gn, qn = to_np(g), to_np(q)
    tau = _kth_largest(qn.astype(np.float64) @ gn.astype(np.float64).T, 300)
    g64 = gn.astype(np.float64)
    tau_j = _kth_largest(np.triu(g64 @ g64.T, 1) + np.tril(np.full((N, N), -np.inf)), 300)
    wr, wj = oracle_range(ref, qn, gn, tau), oracle_join(ref, gn, tau_j)
    assert wr[0].size > 250 and wj[0].size > 250
    for a, b in SCALES + FAR_SCALES:
        run = _Run(S, device, form, _scaled(g, a))
        qs = _scaled(q, b)
        for path in (None, "index"):
            what = (form, E, (a, b), path)
            _assert_range(run.range(qs, float(np.ldexp(tau, a + b)), path=path), Q, (wr[0], wr[1], np.ldexp(wr[2], a + b)), what)
            if b == 0 or a == b or (a, b) == (-75, 60):        # the join has no queries: each distinct a once
                _assert_join(run.join(float(np.ldexp(tau_j, 2 * a)), path=path), (wj[0], wj[1], np.ldexp(wj[2], 2 * a)), what)


# =================================================================== E. k and merge limits
@pytest.mark.parametrize("form", FORMS)
def test_k_at_the_fast_path_boundary_and_at_k_max(S, oracle, device, form):
    from mmr_amd._lib import MMRError
    E = 512
    dtype = _dtype(form)
    q = synth.synth_unit_rows(5, E, seed=12).to(dtype)
    for N in (20011, 50):
        g = synth.synth_unit_rows(N, E, seed=11 + N).to(dtype)
        run = _Run(S, device, form, g)
        mask50 = np.random.default_rng(N).random(N) < 0.5
        for k in (26, 27, 63, 64):
            for mask in (None, mask50):
                got = run.topk(q, k, mask, scale=100.0)
                assert_topk(got, expect_topk(oracle, q, g, np.ones(N, bool) if mask is None else mask, k, scale=100.0))
                live = N if mask is None else int(mask.sum())
                assert bool((got[1][:, min(live, k):] == -1).all()) and bool((got[1][:, :min(live, k)] >= 0).all())
                if k > 26:
                    assert (got[3] == 1).all(), "k + 6 > KS_MAX: exhaustive only"
        for k in (65, 0):
            with pytest.raises(MMRError):
                run.topk(q, k)


def _merge_lists(parts, k, Q, seed):
    """synthetic per-shard lists: dots from a 20-value pool (dense ties across parts) plus NaN and -inf, ids up to 2^40,
    ids repeated across parts carry the same dot (overlapping shards), -1 slots in the middle, one all-empty part"""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.standard_normal(20), [np.nan, -np.inf, -np.inf]])
    M = max(parts * k // 2, k + 3)
    ids = np.empty((parts, Q, k), np.int64)
    dots = np.empty((parts, Q, k), np.float64)
    for qi in range(Q):
        universe = rng.integers(0, 1 << 40, M, dtype=np.int64)
        universe[0] = (1 << 40) - 1
        assert np.unique(universe).size == M
        val = pool[rng.integers(0, pool.size, M)]
        for p in range(parts):
            pick = rng.choice(M, k, replace=False)
            ids[p, qi], dots[p, qi] = universe[pick], val[pick]
    hole = rng.random(ids.shape) < 0.1
    ids[hole] = -1
    dots[hole] = 123.0                                         # an empty slot's dot must be ignored
    if parts > 1:
        ids[parts // 2] = -1
    return ids, dots


@pytest.mark.parametrize("parts,k", [(1, 1), (2, 10), (8, 64), (16, 64), (16, 10)])
def test_merge_on_synthetic_lists(S, oracle, device, parts, k):
    for Q in (1, 300):
        ids, dots = _merge_lists(parts, k, Q, seed=parts * 100 + k + Q)
        wi, ws, wd = oracle.topk_merge(ids, dots, scale=100.0)
        if parts * k >= 20 and Q == 300:
            assert np.isnan(dots).any() and np.isneginf(dots[ids >= 0]).any() and (ids == -1).any()
        ti, td = torch.from_numpy(ids).to(device), torch.from_numpy(dots).to(device)
        packed = torch.stack([ti, td.view(torch.int64)], dim=-1)
        for got in (S.merge_topk(ti, td, 100.0), S.merge_topk_packed(packed, 100.0)):
            assert np.array_equal(got[1].cpu().numpy(), wi), (parts, k, Q)
            assert np.array_equal(got[2].cpu().numpy().view(np.int64), wd.view(np.int64))
            assert np.array_equal(got[0].cpu().numpy().view(np.int32), ws.view(np.int32))
