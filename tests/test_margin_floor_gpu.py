"""The certificates' margins, pinned from below, as the search calls use them.

Every "exact" call decides a pair from the MFMA scan's approximate dot ``acc`` only when it lies more than ``eps`` from
the threshold (or from the k-th score) and rechecks everything closer in fp64; it is exact only while
|acc - dot64| <= eps.  The rest of the suite bounds ``eps`` from ABOVE (candidate counts, pruning); nothing there fails
when it is too small, because the MFMA term is 38x above the real error and the split terms are Cauchy-Schwarz bounds
that random rows stay a factor sqrt(E) under.  Here:

(a) fixtures whose scan error is 94 % of the smallest sound margin (margin_helpers.doc_margin) go through every route
    that scans a bf16 ``hi`` half, with thresholds half an error away from the exact dot and ON it, and with a ladder of
    decoys that keeps the planted rows out of the first tier's 32 candidate tiles; results must equal the oracle's;
(b) the same calls with the caller's residual scalar understated (R / 4) must give a WRONG answer -- a control that still
    comes out exact means the fixture has no teeth, and fails.  ||q - bf16(q)|| and the R of a call that splits for itself
    are measured inside the call and cannot be understated from outside; for those terms the evidence is
    test_margin_fixtures_host.py: with the term dropped the planted error is more than twice the margin that is left,
    so a kernel that under-measured them by half fails (a);
(c) on bf16 / fp16 galleries, whose margin is the MFMA term alone, counts[1] must reach the number of pairs within 0.9
    eps of their threshold (the worst accumulation error is 2.6 % of eps, profiles/mfma_acc_probe.txt, so such a pair's
    ``acc`` is within 0.93 eps), and the same call under a host bound of G / 2 must fall below that floor.

The controls provoke wrong answers, never faults: every pointer and capacity stays valid, and the capacities grow to
the counts the calls report.  test_margin_fixtures_host.py proves the fixtures' arithmetic without a GPU."""
import functools

import numpy as np
import pytest
import torch

import margin_helpers as M
from assign_helpers import ambiguous_rows
from decide_helpers import oracle_decide, words_np
from search_helpers import dot64, oracle_join, oracle_range
from sweep_helpers import check_sweep, oracle_sweep

pytestmark = pytest.mark.gpu

ES = [128, 256, 512, 768]
K = 10
MAXP = 1 << 27


@pytest.fixture(scope="module")
def S(device):
    from mmr_amd import search
    return search


@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


class Dev:
    """A fixture on the device with its split and its measured bounds"""
    def __init__(self, S, fx, device):
        self.fx = fx
        self.q = torch.from_numpy(fx.q).to(device)
        self.g = torch.from_numpy(fx.g).to(device)
        self.hi, self.lo, self.resid = S._split_fp32(self.g)
        self.nb = S.gallery_norm_bound(self.g)
        self.split = (self.hi, self.lo, self.resid)
        self.no_resid = (self.hi, self.lo, None)
        self.quarter = (self.hi, self.lo, self.resid / 4)           # the control: R understated four times


_cache = {}


def dev_fx(S, device, form, E):
    key = (form, E)
    if key not in _cache:
        fx = {"gallery": M.aligned_gallery_fixture, "query": M.aligned_query_fixture,
              "join": functools.partial(M.aligned_gallery_fixture, self_join=True)}[form](E)
        _cache[key] = Dev(S, fx, device)
    return _cache[key]


def _share(d):
    """|acc - dot64| of the planted pairs as a share of doc_margin built from the bounds the DEVICE measured"""
    fx = d.fx
    qh = M.bf16_round(fx.q)
    dm = M.doc_margin("split", qh, float(d.nb.item()), R=float(d.resid.item()), qr=M.resid_norm(fx.q))
    return fx.D / dm[0]


def _taus(fx):
    """query id -> the thresholds half an error from the planted pairs' exact dot (the scan's product is 0.47 eps on the
    wrong side) and ON it (0.94 eps)"""
    t = {0: [fx.base + fx.D / 2, fx.base + fx.D]}
    if fx.q.shape[0] > 1:
        t[1] = [fx.base - fx.D / 2, fx.base - fx.D]
    return t


# ------------------------------------------------------------------------------------------- (a) + (b): range search
def _range(S, d, tau, split, nb):
    a, b, _, dd = S._range_call(d.q, d.g, tau, 1.0, None, nb, split, None, None, MAXP)
    return a.cpu().numpy().astype(np.int64), b.cpu().numpy().astype(np.int64), dd.cpu().numpy()


def _same_pairs(got, want):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(got, want))


@pytest.mark.parametrize("form", ["gallery", "query"])
@pytest.mark.parametrize("E", ES)
def test_range_search_keeps_pairs_at_the_edge_of_the_margin(S, ref, device, form, E):
    d = dev_fx(S, device, form, E)
    fx = d.fx
    print(f"range {form} E={E}: planted error = {_share(d):.4f} of doc_margin")
    for tau in sorted({t for ts in _taus(fx).values() for t in ts}):
        want = oracle_range(ref, fx.q, fx.g, tau, slack=1e-9)
        assert set(fx.planted.tolist()) <= set(want[1][want[0] == 0].tolist())
        routes = {"split in the call": (None, None), "hi and its residual bound": (d.split, d.nb),
                  "hi without a residual bound (2^-8 G)": (d.no_resid, d.nb)}
        for name, (split, nb) in routes.items():
            got = _range(S, d, tau, split, nb)
            assert _same_pairs(got, want), (form, E, tau, name, len(got[0]), len(want[0]))
        if form == "gallery" and tau > fx.base:
            got = _range(S, d, tau, d.quarter, d.nb)
            assert not _same_pairs(got, want), "control: R / 4 still gave the exact pair set -- the fixture has no teeth"
            assert not set(fx.planted.tolist()) & set(got[1].tolist())


@pytest.mark.parametrize("E", ES)
def test_self_join_keeps_pairs_at_the_edge_of_the_margin(S, ref, device, E):
    d = dev_fx(S, device, "join", E)
    fx = d.fx
    a = fx.partner
    special = np.sort(np.concatenate([fx.planted, fx.anti, fx.decoys, [a]]))
    sub = np.ascontiguousarray(fx.g[special])
    exact = dot64(ref, fx.g[a], fx.g[fx.planted[0]])
    err = exact - dot64(ref, M.bf16_round(fx.g[a]), fx.gh)
    R = float(d.resid.item())
    dm = M.doc_margin("split", M.bf16_round(fx.g[a:a + 1]), float(d.nb.item()), R=R, qr=[R])[0]     # the query is a row: qr <= R
    print(f"self-join E={E}: planted error = {err / dm:.4f} of doc_margin")
    # pairs with a filler cannot come near (test_self_join_fixture_reaches_the_margin): the oracle looks at the rest
    for tau in (exact - err / 2, exact):
        wi, wj, wd = oracle_join(ref, sub, tau, slack=1e-9)
        want = (special[wi], special[wj], wd)
        assert len(wd) >= 4
        i, j, _, dd = S._range_call(None, d.g, tau, 1.0, None, None, None, None, None, MAXP)
        got = (i.cpu().numpy().astype(np.int64), j.cpu().numpy().astype(np.int64), dd.cpu().numpy())
        assert _same_pairs(got, want), (E, tau, len(got[0]), len(want[0]))


# ------------------------------------------------------------------------------------------- (a) + (b): sweep, decide
def _grid(fx):
    """An ascending grid with, for either kind of planted pair, the threshold half an error away and the one ON the exact
    dot.  The anti-aligned pairs (gallery form: rows gh - DELTA s; query form: query 1) have acc ABOVE a threshold their
    dot64 fails."""
    pts = {fx.base - 2.5 * fx.D, fx.base - fx.D, fx.base - fx.D / 2, fx.base + fx.D / 2, fx.base + fx.D, fx.base + 2.5 * fx.D}
    return np.array(sorted(pts), dtype=np.float64)


@pytest.mark.parametrize("form", ["gallery", "query"])
@pytest.mark.parametrize("E", ES)
def test_sweep_bins_pairs_at_the_edge_of_the_margin(S, ref, device, form, E):
    d = dev_fx(S, device, form, E)
    fx = d.fx
    Q = fx.q.shape[0]
    labels = (np.arange(fx.N) % 3).astype(np.int32)
    targets = np.arange(Q, dtype=np.int32) % 3
    thr = _grid(fx)
    want_ge, want_total, _ = oracle_sweep(ref, fx.q, fx.g, labels, targets, thr)
    lab, tg = torch.from_numpy(labels).to(device), torch.from_numpy(targets).to(device)
    tt = torch.from_numpy(thr)

    def run(split, nb):
        return S._sweep_call(d.q, d.g, lab, tg, tt, None, nb, split, None, MAXP, None, False)

    for name, (split, nb) in {"split in the call": (None, None), "hi given": (d.split, d.nb)}.items():
        check_sweep(run(split, nb), want_ge, want_total)
    if form == "gallery":
        res = run(d.quarter, d.nb)
        same = (np.array_equal(res.tp.cpu().numpy(), want_ge[:, 1]) and np.array_equal(res.fp.cpu().numpy(), want_ge[:, 0]))
        assert not same, "control: R / 4 still gave the exact counts -- the fixture has no teeth"


@pytest.mark.parametrize("form", ["gallery", "query"])
@pytest.mark.parametrize("E", ES)
def test_decide_keeps_pairs_at_the_edge_of_the_margin(S, ref, device, form, E):
    d = dev_fx(S, device, form, E)
    fx = d.fx
    # one query per threshold: the aligned pairs just under and on their exact dot, the anti-aligned ones likewise
    if form == "gallery":
        qsel = [0, 0, 0, 0]
        thr = np.array([fx.base + fx.D / 2, fx.base + fx.D, fx.base - fx.D / 2, fx.base - fx.D])
    else:
        qsel = [0, 0, 1, 1]
        thr = np.array([fx.D / 2, fx.D, -fx.D / 2, -fx.D])
    qn = np.ascontiguousarray(fx.q[qsel])
    qd = torch.from_numpy(qn).to(device)
    want = oracle_decide(ref, qn, fx.g, thr, slack=1e-9)
    td = torch.from_numpy(thr).to(device)

    def run(split, nb):
        return words_np(S._decide_call(qd, d.g, td, None, nb, split, None, MAXP, None)[0])

    for name, (split, nb) in {"split in the call": (None, None), "hi given": (d.split, d.nb)}.items():
        assert np.array_equal(run(split, nb), want), (form, E, name)
    if form == "gallery":
        got = run(d.quarter, d.nb)
        assert not np.array_equal(got, want), "control: R / 4 still gave the exact masks -- the fixture has no teeth"
        # both directions: an aligned row is missing under its threshold, an anti-aligned row passes one it fails
        r, w = int(fx.planted[2]), int(fx.anti[0])
        assert not (got[0, r >> 5] >> np.uint32(r & 31)) & 1 and (got[2, w >> 5] >> np.uint32(w & 31)) & 1


# ------------------------------------------------------------------------------------------- (a) + (b): the top-k calls
def _topk_same(idx, d64, want):
    return (np.array_equal(idx.cpu().numpy().astype(np.int64), want[0])
            and np.array_equal(d64.cpu().numpy().view(np.int64), want[2].view(np.int64)))


@pytest.mark.parametrize("form", ["gallery", "query"])
@pytest.mark.parametrize("E", ES)
def test_topk_routes_find_a_planted_row_outside_the_first_tiers_tiles(S, device, form, E):
    """The planted rows are the oracle's ranks 1-4, and 48 decoy tiles (against KS_MAX = 32) score higher in the hi-half
    scan; kth - (best excluded maximum) is 0.58 of the planted error, so the first tier may certify only with a margin
    under 0.55 eps.  ``status`` is not asserted: which tier answers is not part of the contract."""
    from oracle import search_ref
    d = dev_fx(S, device, form, E)
    fx = d.fx
    want = search_ref.cosine_topk(fx.q, fx.g, K)
    assert want[0][0, 0] == fx.planted[0]
    print(f"top-k {form} E={E}: planted error = {_share(d):.4f} of doc_margin")

    def split_call(split):
        idx, _, d64, _, _ = S._local_topk(d.q, d.g, K, 1.0, None, True, True, norm_bound_dev=d.nb, split=split)
        return idx, d64

    def deep_call(split):
        idx, _, d64, _, _ = S._deep_call(d.q, d.g, K, 1.0, None, d.nb, split, None, MAXP, None, None, True)
        return idx, d64

    assert _topk_same(*split_call(d.split), want), "mmr_cosine_topk_split"
    assert _topk_same(*split_call(d.no_resid), want), "mmr_cosine_topk_split without a residual bound"
    assert _topk_same(*deep_call(d.split), want), "mmr_cosine_topk_deep over hi / lo"
    assert _topk_same(*deep_call(d.no_resid), want), "mmr_cosine_topk_deep without a residual bound"
    index = S.GalleryIndex(d.g, presplit=True)
    assert index._split is not None
    _, idx, d64 = index.search(d.q, k=K, return_dot64=True)
    assert _topk_same(idx, d64, want), "GalleryIndex(presplit=True).search"
    _, idx, d64 = index.search_deep(d.q, K, return_dot64=True)
    assert _topk_same(idx, d64, want), "GalleryIndex(presplit=True).search_deep"
    if form == "gallery":
        for name, call in (("mmr_cosine_topk_split", split_call), ("mmr_cosine_topk_deep", deep_call)):
            idx, d64 = call(d.quarter)
            assert not _topk_same(idx, d64, want), f"control: {name} with R / 4 is still exact -- the fixture has no teeth"
            assert fx.planted[0] not in idx.cpu().numpy()[0]


# ------------------------------------------------------------------------------------------- (c): candidate floors
CROWD = [(dt, E) for dt in (torch.bfloat16, torch.float16) for E in ES]
TAU = 0.5
NQ, NROWS = 40, 20011


class Crowd:
    def __init__(self, dtype, E, device):
        self.q, self.g, self.dots = M.crowd_fixture(dtype, E, NROWS, NQ, TAU)
        self.qd, self.gd = self.q.to(device), self.g.to(device)
        self.qf, self.gf = M.f32(self.q), M.f32(self.g)
        self.G = M.max_norm(self.gf)
        self.eps = M.doc_margin("plain", self.qf, self.G)[:, None]   # [Q, 1]


_crowd = {}


def crowd(dtype, E, device):
    if (dtype, E) not in _crowd:
        _crowd[(dtype, E)] = Crowd(dtype, E, device)
    return _crowd[(dtype, E)]


def _range_counts(S, q, g, tau, host_bound, cand_cap, device):
    """the raw call: counts = (matches, candidates)"""
    from mmr_amd import _lib
    L = _lib.lib()
    N, E = g.shape
    Q = 0 if q is None else q.shape[0]
    code = _lib.dtype_code(g.dtype)
    ws = torch.empty(L.mmr_range_workspace_bytes(N, E, Q, cand_cap, code, 0), dtype=torch.uint8, device=device)
    outs = [torch.empty(cand_cap, dtype=dt, device=device) for dt in (torch.int32, torch.int32, torch.float32, torch.float64)]
    counts = torch.zeros(2, dtype=torch.int64, device=device)
    tail = (1.0, float(host_bound), None, None, cand_cap, cand_cap, *(o.data_ptr() for o in outs), counts.data_ptr(), ws.data_ptr(),
            ws.numel(), _lib.stream_ptr(device))
    if q is None:
        _lib.check(L.mmr_gallery_self_join(g.data_ptr(), None, code, N, E, float(tau), *tail))
    else:
        _lib.check(L.mmr_cosine_range(q.data_ptr(), g.data_ptr(), None, code, Q, N, E, float(tau), *tail))
    m, c = counts.tolist()
    assert c <= cand_cap
    return m, c


def _floor_report(what, dtype, E, cands, floor, control):
    print(f"{what} {str(dtype)[6:]} E={E}: counts[1] = {cands}, floor = {floor}, slack = {cands - floor}; under G / 2: {control}")
    assert cands >= floor, f"{what}: {cands} candidates, but {floor} pairs lie within 0.9 eps of their threshold"
    assert control < floor, f"{what}: the control (host bound G / 2) still reaches the floor -- the floor has no teeth"


@pytest.mark.parametrize("dtype,E", CROWD)
def test_range_candidates_reach_the_floor(S, device, dtype, E):
    """range search: candidate iff acc >= tau - eps (one-sided)"""
    c = crowd(dtype, E, device)
    floor = int((c.dots >= TAU - 0.9 * c.eps).sum())
    m, cands = _range_counts(S, c.qd, c.gd, TAU, 0.0, NQ * NROWS, device)
    assert m <= cands
    _, control = _range_counts(S, c.qd, c.gd, TAU, c.G / 2, NQ * NROWS, device)
    _floor_report("range", dtype, E, cands, floor, control)


@pytest.mark.parametrize("dtype,E", CROWD)
def test_self_join_candidates_reach_the_floor(S, device, dtype, E):
    """the self-join: the crowd's queries and the first 6000 of its rows as one gallery; candidate iff acc >= tau - eps
    with eps from either row of the pair -- the floor takes the shorter one"""
    c = crowd(dtype, E, device)
    n = 6000
    j = torch.cat([c.q, c.g[:n]]).contiguous()
    jf = M.f32(j).astype(np.float64)
    norms = np.sqrt((jf * jf).sum(1))
    G = float(norms.max())
    floor = 0
    for s0 in range(0, jf.shape[0], 1024):
        s = jf[s0:s0 + 1024] @ jf.T
        eps = M.R_EPS_REL * np.minimum(norms[s0:s0 + 1024, None], norms[None, :]) * G
        upper = np.arange(jf.shape[0])[None, :] > np.arange(s0, min(s0 + 1024, jf.shape[0]))[:, None]
        floor += int(((s >= TAU - 0.9 * eps) & upper).sum())
    assert floor >= 1000
    jd = j.to(device)
    m, cands = _range_counts(S, None, jd, TAU, 0.0, 1 << 22, device)
    _, control = _range_counts(S, None, jd, TAU, G / 2, 1 << 22, device)
    _floor_report("self-join", dtype, E, cands, floor, control)


@pytest.mark.parametrize("dtype,E", CROWD)
def test_decide_candidates_reach_the_floor(S, device, dtype, E):
    """decide (include/mmr.h): "a >= thresholds[q] + eps (rounded up to fp32) is a certain pass and
    a < thresholds[q] - eps (rounded down) a certain fail; every other pair [...] is a CANDIDATE" -- two-sided"""
    c = crowd(dtype, E, device)
    floor = int((np.abs(c.dots - TAU) <= 0.9 * c.eps).sum())
    thr = torch.full((NQ,), TAU, dtype=torch.float64, device=device)
    cands = S._decide_call(c.qd, c.gd, thr, None, None, None, None, MAXP, None)[0].counts[1]
    control = S._decide_call(c.qd, c.gd, thr, c.G / 2, None, None, None, MAXP, None)[0].counts[1]
    _floor_report("decide", dtype, E, cands, floor, control)


@pytest.mark.parametrize("dtype,E", CROWD)
def test_sweep_candidates_reach_the_floor(S, device, dtype, E):
    """sweep (csrc/sweep_scan_body.h): "[lo, hi] holds the exact dot (bounds rounded outward)", hi = f32_up(av + eps),
    lo = f32_down(av - eps); b = #{j : down[j] <= hi}; "decided = ... up[b] <= lo", i.e. a pair is decided iff no grid
    point lies in [a - eps, a + eps] and is a candidate otherwise -- two-sided, against every grid point"""
    c = crowd(dtype, E, device)
    grid = np.array([0.3, TAU, 0.7])
    near = np.abs(c.dots[:, :, None] - grid[None, None, :]).min(-1)
    floor = int((near <= 0.9 * c.eps).sum())
    labels = (torch.arange(NROWS, dtype=torch.int32) % 5).to(device)
    targets = (torch.arange(NQ, dtype=torch.int32) % 5).to(device)
    tt = torch.from_numpy(grid)
    cands = S._sweep_call(c.qd, c.gd, labels, targets, tt, None, None, None, None, MAXP, None, False).counts[1]
    control = S._sweep_call(c.qd, c.gd, labels, targets, tt, c.G / 2, None, None, None, MAXP, None, False).counts[1]
    _floor_report("sweep", dtype, E, cands, floor, control)


@pytest.mark.parametrize("dtype,E", CROWD)
def test_assign_ambiguous_rows_reach_the_floor(S, device, dtype, E):
    """assign: a row is decided iff its winner's lower bound is strictly above every other upper bound, so a row with
    winner - runner-up <= 0.9 (eps_a + eps_b) must be ambiguous"""
    g, cen, _ = M.assign_crowd_fixture(dtype, E, 8003, 40)
    gf, cf = M.f32(g), M.f32(cen)
    floor = int(ambiguous_rows(gf, cf, factor=0.9, doc=True).sum())
    assert floor >= 1000
    gd, cd = g.to(device), cen.to(device)
    cands = S._assign_call(gd, cd, None, None, None, None, False, None, MAXP)[2][1]
    control = S._assign_call(gd, cd, None, M.max_norm(gf) / 2, None, None, False, None, MAXP)[2][1]
    _floor_report("assign", dtype, E, cands, floor, control)
