"""GPU: deep top-k (mmr_cosine_topk_deep, cosine_topk_deep, GalleryIndex.search_deep), k up to 4096.

Expected values are oracle/search_ref.c's top-k over the compacted gallery gallery[mask], ids mapped back
(search_helpers.expect_topk); idx, score and dot64 are compared bit for bit over ALL queries.  The oracle's list for k'
< k is the first k' entries of its list for k (one total order), so one oracle run at the largest k serves every k.
Forms: a bf16 gallery per call, an fp32 gallery per call, an fp32 GalleryIndex with the pre-split halves, a bf16 index."""
import numpy as np
import pytest
import torch

from mmr_amd import synth
from search_helpers import assert_topk, expect_topk, to_np

pytestmark = pytest.mark.gpu

FORMS = ("bf16", "f32", "f32-index", "bf16-index")
KS = (1, 10, 64, 65, 100, 1000, 4096)
# every N of {50, 4097, 20011, 50000} with a small and a large Q of {1, 5, 70, 300}: one, three and ten 32-query blocks,
# more than one scan chunk (300 > 256 / 128 queries per pass), ragged last tiles, k above the tile count and above N
SHAPES = ((50, 5), (50, 300), (4097, 1), (4097, 70), (20011, 5), (20011, 300), (50000, 1), (50000, 70))


@pytest.fixture(scope="module")
def S(device):
    from mmr_amd import search
    return search


@pytest.fixture(scope="module")
def oracle():
    from oracle import search_ref
    return search_ref


def _dtype(form):
    return torch.bfloat16 if form.startswith("bf16") else torch.float32


class _Run:
    """One gallery on the device, searched the way ``form`` says."""

    def __init__(self, S, device, form, g, norm_bound=None):
        self.S, self.device, self.form = S, device, form
        self.gd = g.to(device)
        self.ix = S.GalleryIndex(self.gd, norm_bound=norm_bound, presplit=form == "f32-index") if form.endswith("index") else None

    def deep(self, q, k, mask=None, scale=1.0, **kw):
        rm = None if mask is None else torch.from_numpy(mask).to(self.device)
        if self.ix is not None:
            return self.ix.search_deep(q.to(self.device), k, scale, return_dot64=True, row_mask=rm, **kw)
        return self.S.cosine_topk_deep(q.to(self.device), self.gd, k, scale, return_dot64=True, row_mask=rm, **kw)


def _prefix(want, k):
    return tuple(np.ascontiguousarray(w[:, :k]) for w in want)


def _check_all_k(run, oracle, q, g, mask, ks, scale=1.0, **kw):
    want = expect_topk(oracle, q, g, np.ones(g.shape[0], bool) if mask is None else mask, max(ks), scale=scale)
    for k in ks:
        got = run.deep(q, k, mask, scale, **kw)
        assert got[1].dtype == torch.int64 and got[0].dtype == torch.float32 and got[2].dtype == torch.float64
        assert tuple(got[1].shape) == (q.shape[0], k)
        try:
            assert_topk(got, _prefix(want, k))
        except AssertionError as e:
            raise AssertionError(f"{run.form} N={g.shape[0]} E={g.shape[1]} Q={q.shape[0]} k={k} masked={mask is not None}: {e}")


# =================================================================== A. forms x shapes x k
@pytest.mark.parametrize("E", [128, 512, 768])
@pytest.mark.parametrize("form", FORMS)
def test_deep_topk_vs_oracle(S, oracle, device, form, E):
    dtype = _dtype(form)
    for N, Q in SHAPES:
        g = synth.synth_unit_rows(N, E, seed=3 + N).to(dtype)
        q = synth.synth_unit_rows(Q, E, seed=4 + Q).to(dtype)
        run = _Run(S, device, form, g)
        _check_all_k(run, oracle, q, g, None, KS)
        mask = np.random.default_rng(N + E).random(N) < 0.5
        _check_all_k(run, oracle, q, g, mask, KS)


@pytest.mark.parametrize("form", FORMS)
def test_scale_and_one_dimensional_query(S, oracle, device, form):
    N, E = 4097, 512
    g = synth.synth_unit_rows(N, E, seed=31).to(_dtype(form))
    q = synth.synth_unit_rows(5, E, seed=32).to(_dtype(form))
    run = _Run(S, device, form, g)
    _check_all_k(run, oracle, q, g, None, (10, 100, 1000), scale=100.0)
    got = run.deep(q[2], 100, scale=100.0)                       # a 1-D query squeezes, as in cosine_topk
    assert tuple(got[0].shape) == tuple(got[1].shape) == tuple(got[2].shape) == (100,)
    want = expect_topk(oracle, q[2:3], g, np.ones(N, bool), 100, scale=100.0)
    assert_topk(tuple(t.unsqueeze(0) for t in got), want)
    two = run.deep(q, 10)
    assert len(two) == 3                                         # return_dot64 off: (values, indices) alone
    plain = (run.ix.search_deep(q.to(device), 10) if run.ix is not None else S.cosine_topk_deep(q.to(device), run.gd, 10))
    assert len(plain) == 2 and torch.equal(plain[1], two[1]) and torch.equal(plain[0], two[0])


@pytest.mark.parametrize("form", ["f32-index", "bf16-index"])
def test_after_delete_rows(S, oracle, device, form):
    N, E, Q = 20011, 512, 70
    g = synth.synth_unit_rows(N, E, seed=41).to(_dtype(form))
    q = synth.synth_unit_rows(Q, E, seed=42).to(_dtype(form))
    run = _Run(S, device, form, g)
    rng = np.random.default_rng(43)
    live = np.ones(N, bool)
    dead = rng.choice(N, N // 3, replace=False)
    # every query's best 20 rows go too
    best = expect_topk(oracle, q, g, live, 20)[0].reshape(-1)
    dead = np.unique(np.concatenate([dead, best]))
    run.ix.delete_rows(torch.from_numpy(dead))
    live[dead] = False
    _check_all_k(run, oracle, q, g, live, (10, 100, 1000))
    extra = rng.random(N) < 0.5                                  # live AND row_mask
    want = expect_topk(oracle, q, g, live & extra, 1000, scale=100.0)
    assert_topk(run.deep(q, 1000, extra, scale=100.0), want)
    run.ix.restore_rows(torch.from_numpy(dead))
    _check_all_k(run, oracle, q, g, None, (100,))


# =================================================================== B. agreement with the old path
@pytest.mark.parametrize("form", FORMS)
def test_deep_equals_cosine_topk_where_both_accept_k(S, device, form):
    N, E, Q = 20011, 512, 70
    g = synth.synth_unit_rows(N, E, seed=51).to(_dtype(form))
    q = synth.synth_unit_rows(Q, E, seed=52).to(_dtype(form))
    run = _Run(S, device, form, g)
    mask = np.random.default_rng(53).random(N) < 0.5
    for m in (None, mask):
        rm = None if m is None else torch.from_numpy(m).to(device)
        for k in (10, 26, 27, 64):
            if run.ix is not None:
                old = run.ix.search(q.to(device), k, 100.0, return_dot64=True, row_mask=rm)
            else:
                old = S.cosine_topk(q.to(device), run.gd, k, 100.0, return_dot64=True, row_mask=rm)
            new = run.deep(q, k, m, 100.0)
            for a, b in zip(old, new):
                assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), (form, k)
    # the old calls keep their limit
    with pytest.raises(Exception, match="k=65"):
        S.cosine_topk(q.to(device), run.gd, 65)


# =================================================================== C. contract edges ("Non-finite values, ties and scale")
@pytest.mark.parametrize("E", [128, 768])
@pytest.mark.parametrize("form", FORMS)
def test_nan_rows_are_absent_and_masking_them_changes_nothing(S, oracle, device, form, E):
    N, Q, k = 20011, 70, 100
    g = synth.synth_unit_rows(N, E, seed=61).to(_dtype(form))
    q = synth.synth_unit_rows(Q, E, seed=62).to(_dtype(form))
    rng = np.random.default_rng(63)
    bad = np.unique(np.concatenate([rng.choice(N, 300, replace=False), np.arange(6400, 6464), [0, N - 1]]))   # two whole tiles too
    best = expect_topk(oracle, q, g, np.ones(N, bool), 5)[0].reshape(-1)           # and rows that would have ranked
    bad = np.unique(np.concatenate([bad, best]))
    g[torch.from_numpy(bad), 7] = float("nan")
    clean = np.ones(N, bool)
    clean[bad] = False
    want = expect_topk(oracle, q, g, clean, k)
    run = _Run(S, device, form, g)
    got = run.deep(q, k)
    assert_topk(got, want)
    assert not np.isin(got[1].cpu().numpy(), bad).any()
    assert_topk(run.deep(q, k, clean), want)                     # masking the NaN rows changes nothing
    half = rng.random(N) < 0.5
    assert_topk(run.deep(q, 1000, half), expect_topk(oracle, q, g, half & clean, 1000))


@pytest.mark.parametrize("E", [128, 512])
@pytest.mark.parametrize("form", FORMS)
def test_infinite_rows_rank_first_and_last_and_make_every_query_wild(S, oracle, device, form, E):
    N, Q, k, C = 4097, 5, 100, 17
    g = synth.synth_unit_rows(N, E, seed=71).to(_dtype(form))
    q = synth.synth_unit_rows(Q, E, seed=72).to(_dtype(form))
    R = N // 4
    g[R, C] = float("inf")
    q[0, C], q[1, C], q[2, C] = 0.0, 0.125, -0.125               # dot with row R: NaN, +inf, -inf
    q[3] = 0.0                                                   # NaN with row R, 0 with every other row
    run = _Run(S, device, form, g)
    assert float(S.gallery_norm_bound(run.gd)) == float("inf")   # every query is wild: all tiles listed, results stay exact
    got = run.deep(q, k, scale=100.0)
    assert_topk(got, expect_topk(oracle, q, g, np.ones(N, bool), k, scale=100.0))
    idx, d64 = got[1].cpu().numpy(), got[2].cpu().numpy()
    assert R not in idx[0] and idx[1, 0] == R and d64[1, 0] == np.inf and float(got[0][1, 0]) == np.inf
    assert R not in idx[2] and idx[3].tolist() == [r for r in range(k + 1) if r != R][:k] and not np.signbit(d64[3]).any()
    few = np.zeros(N, bool)                                      # 6 live rows, R among them: the -inf row is returned last
    few[[3, 77, R, N - 900, N - 31, N - 1]] = True
    got = run.deep(q, k, few)
    assert_topk(got, expect_topk(oracle, q, g, few, k))
    idx, d64 = got[1].cpu().numpy(), got[2].cpu().numpy()
    assert idx[2, 5] == R and d64[2, 5] == -np.inf and (idx[2, 6:] == -1).all() and (d64[2, 6:] == -np.inf).all()
    assert R not in idx[0] and (idx[0, 5:] == -1).all() and idx[1, 0] == R
    big = run.deep(q, 4096)                                      # k above the 4096 non-NaN rows query 0 can return
    assert_topk(big, expect_topk(oracle, q, g, np.ones(N, bool), 4096))


@pytest.mark.parametrize("form", FORMS)
def test_total_ties_return_the_first_k_live_rows(S, oracle, device, form):
    """The zero query, and a gallery of identical rows: every tile is listed and every row survives (the all-listed
    case); small first capacities make the call retry at the sizes it reports."""
    N, E, k = 3000, 512, 100
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=81).to(dtype)
    q = synth.synth_unit_rows(3, E, seed=82).to(dtype)
    q[1] = 0.0
    mask = np.random.default_rng(83).random(N) < 0.5
    run = _Run(S, device, form, g)
    for m in (None, mask):
        for caps in ({}, {"tile_cap": 8, "surv_cap": 8}):
            got = run.deep(q, k, m, **caps)
            assert_topk(got, expect_topk(oracle, q, g, np.ones(N, bool) if m is None else m, k))
            rows = np.arange(N) if m is None else np.flatnonzero(m)
            assert got[1][1].cpu().numpy().tolist() == rows[:k].tolist()
            assert (got[2][1] == 0).all() and not np.signbit(got[2][1].cpu().numpy()).any()
    same = g[5:6].repeat(N, 1).contiguous()
    run = _Run(S, device, form, same)
    for m in (None, mask):
        got = run.deep(q, k, m, tile_cap=8, surv_cap=8)
        assert_topk(got, expect_topk(oracle, q, same, np.ones(N, bool) if m is None else m, k))
        rows = np.arange(N) if m is None else np.flatnonzero(m)
        assert (got[1].cpu().numpy() == rows[:k][None, :]).all()


@pytest.mark.parametrize("form", FORMS)
def test_duplicates_of_the_kth_row_resolve_by_id(S, oracle, device, form):
    N, E, Q, k = 20011, 512, 5, 100
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=91).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=92).to(dtype)
    first = expect_topk(oracle, q, g, np.ones(N, bool), k)[0]
    kth = int(first[0, k - 1])
    taken = set(first.reshape(-1).tolist())
    spots = [r for r in range(211, N, 487) if r not in taken][:40]          # 40 copies, 487 rows apart: 40 different tiles
    assert len(spots) == 40
    g[torch.tensor(spots)] = g[kth].clone()
    want = expect_topk(oracle, q, g, np.ones(N, bool), k + 60)
    ties = np.flatnonzero(want[2][0] == want[2][0][k - 1])
    assert ties.size == 41 and ties[0] <= k - 1 and np.all(np.diff(want[0][0][ties]) > 0)     # one value, ids ascending
    run = _Run(S, device, form, g)
    for kk in (k, k + 19, k + 60):
        assert_topk(run.deep(q, kk), _prefix(want, kk))


SCALES = ((60, 0), (0, -60), (60, 60), (-60, -60), (-60, 60))


def _scaled(x, e):
    y = (x.float() * (2.0 ** e)).to(x.dtype)
    assert torch.isfinite(y).all() and bool(((y != 0) == (x != 0)).all())
    assert torch.equal(y.double() * (2.0 ** -e), x.double())
    return y


@pytest.mark.parametrize("form", FORMS)
def test_power_of_two_scales(S, oracle, device, form):
    """gallery * 2^a, queries * 2^b: idx unchanged, every dot64 multiplied by 2^(a+b) exactly"""
    N, E, Q, k = 4097, 512, 37, 100
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=101).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=102).to(dtype)
    oi, _, od = oracle.cosine_topk(to_np(q), to_np(g), k, scale=100.0)
    for a, b in SCALES:
        wd = np.ldexp(od, a + b)
        with np.errstate(over="ignore", under="ignore"):
            ws = (wd * np.float64(np.float32(100.0))).astype(np.float32)
        run = _Run(S, device, form, _scaled(g, a))
        try:
            assert_topk(run.deep(_scaled(q, b), k, scale=100.0), (oi, ws, wd))
        except AssertionError as e:
            raise AssertionError(f"{form} scales 2^{a}, 2^{b}: {e}")


def _c_deep(device, q, g, k, tile_cap, surv_cap, host_bound=0.0, dev_bound=None, split=None, scale=1.0, out=None):
    """The C call itself -> (score, idx, dot64, counts); ``out``: reuse these output tensors (graph capture)."""
    from mmr_amd import _lib
    L = _lib.lib()
    Q, E = q.shape
    N = g.shape[0]
    code = _lib.dtype_code(g.dtype)
    hi, lo, resid = split if split is not None else (None, None, None)
    need = L.mmr_deep_topk_workspace_bytes(N, E, Q, k, tile_cap, surv_cap, code, int(hi is not None))
    assert need > 0
    if out is None:
        out = (torch.empty(Q, k, dtype=torch.float32, device=device), torch.empty(Q, k, dtype=torch.int64, device=device),
               torch.empty(Q, k, dtype=torch.float64, device=device), torch.zeros(2, dtype=torch.int64, device=device),
               torch.empty(need, dtype=torch.uint8, device=device))
    score, idx, d64, counts, ws = out
    _lib.check(L.mmr_cosine_topk_deep(q.data_ptr(), g.data_ptr(), _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(resid), code, Q, N, E, k,
                                      float(scale), float(host_bound), _lib.ptr(dev_bound), 0, tile_cap, surv_cap, idx.data_ptr(),
                                      score.data_ptr(), d64.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _lib.stream_ptr(device)))
    return out


@pytest.mark.parametrize("form", ["bf16", "f32"])
def test_understated_caller_bound_cannot_shrink_the_margin(S, oracle, device, form):
    """margin = max(caller's number, device scalar): with the measured scalar present, a caller's 1e-6 changes nothing"""
    N, E, Q, k = 20011, 512, 8, 100
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=111).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=112).to(dtype)
    gd, qd = g.to(device), q.to(device)
    nb = S.gallery_norm_bound(gd)
    honest = _c_deep(device, qd, gd, k, 8 * Q * k, 8 * Q * k, 0.0, nb)
    lying = _c_deep(device, qd, gd, k, 8 * Q * k, 8 * Q * k, 1e-6, nb)
    torch.cuda.synchronize(device)
    assert honest[3].tolist() == lying[3].tolist()
    for a, b in zip(honest[:3], lying[:3]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert_topk(lying, expect_topk(oracle, q, g, np.ones(N, bool), k))
    ix = S.GalleryIndex(gd, norm_bound=1e-6)
    assert_topk(ix.search_deep(qd, k, return_dot64=True), expect_topk(oracle, q, g, np.ones(N, bool), k))


# =================================================================== D. capacity protocol
@pytest.mark.parametrize("form", FORMS)
def test_capacity_protocol(S, oracle, device, form):
    N, E, Q, k = 20011, 512, 8, 100
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=121).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=122).to(dtype)
    run = _Run(S, device, form, g)
    want = expect_topk(oracle, q, g, np.ones(N, bool), k)
    assert_topk(run.deep(q, k, tile_cap=1, surv_cap=1), want)           # exact after one retry
    assert_topk(run.deep(q, k, tile_cap=1 << 20, surv_cap=1), want)     # survivor list alone too small
    with pytest.raises(MemoryError, match="max_pairs"):
        run.deep(q, k, tile_cap=1, surv_cap=1, max_pairs=Q * k - 1)     # at least Q * k survivors are needed
    with pytest.raises(MemoryError, match="max_pairs"):
        run.deep(q, k, max_pairs=Q * k)                                 # the default first capacities are checked too
    with pytest.raises(ValueError):
        run.deep(q, k, tile_cap=-5)


@pytest.mark.parametrize("form", ["bf16", "f32", "f32-index"])
def test_counts_and_outputs_are_reproducible(S, device, form):
    N, E, Q, k = 50000, 512, 8, 1000
    dtype = _dtype(form)
    gd = synth.synth_unit_rows(N, E, seed=3).to(dtype).to(device)
    qd = synth.synth_unit_rows(Q, E, seed=4).to(dtype).to(device)
    ix = S.GalleryIndex(gd, presplit=form == "f32-index")
    split = ix._split if form == "f32-index" else None
    runs = [_c_deep(device, qd, gd, k, 4 * Q * k, 4 * Q * k, 0.0, ix.norm_bound_dev, split) for _ in range(2)]
    small = _c_deep(device, qd, gd, k, 16, 4 * Q * k, 0.0, ix.norm_bound_dev, split)     # overflow: the counter keeps counting
    torch.cuda.synchronize(device)
    assert runs[0][3].tolist() == runs[1][3].tolist()
    assert small[3][0].item() == runs[0][3][0].item() and small[3][1].item() <= 16 * (16 if form == "f32" else 32)
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# =================================================================== E. pruning really happens
def _margins(form, q, g):
    """Per query the largest margin a route of this form may use (range_common.h: scan_margin), from the data alone, plus
    1e-9 for the fp64 summation order.  1.0001 / 1.00002: the kernels' upward roundings of |q| and of the measured bounds."""
    q64 = q.double().numpy()
    G = float(torch.linalg.vector_norm(g.float(), dim=1, dtype=torch.float64).max()) * 1.00002
    if form == "bf16":
        return 8.0001e-5 * np.sqrt((q64 * q64).sum(1)) * 1.0001 * G + 1e-9
    qh = q.bfloat16().double().numpy()
    R = float(torch.linalg.vector_norm(g - g.bfloat16().float(), dim=1, dtype=torch.float64).max()) * 1.00002
    qr = np.sqrt(((q64 - qh) ** 2).sum(1)) * 1.00002
    qn = np.sqrt((qh * qh).sum(1)) * 1.0001
    return 8.0001e-5 * qn * G * (1 + 2.0 ** -8) + qr * G + qn * R + 1e-9


@pytest.mark.parametrize("form,N", [("bf16", 50000), ("bf16", 200000), ("f32-index", 50000)])
def test_pruning_really_happens(S, device, form, N):
    """counts[1] <= rows with dot >= M_k - 2 eps, counts[0] <= tiles with max >= M_k - 4 eps (M_k: the exact k-th largest
    32-row-tile maximum; numpy fp64): the device lists bmax >= b_k - 2 eps with |bmax - m_t| <= eps and b_k >= M_k - eps.
    On these inputs the row cap stays within 1.7 k per query, so a path that quietly lists everything fails here."""
    E, Q = 512, 8
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=3).to(dtype)
    q = synth.synth_unit_rows(Q, E, seed=4).to(dtype)
    gd, qd = g.to(device), q.to(device)
    ix = S.GalleryIndex(gd, presplit=form == "f32-index")
    split = ix._split if form == "f32-index" else None
    eps = _margins(form, q, g)[:, None]
    s = torch.cat([q.double() @ g[r:r + 50000].double().T for r in range(0, N, 50000)], 1).numpy()    # [Q, N] fp64
    pad = (-N) % 32
    m = np.concatenate([s, np.full((Q, pad), -np.inf)], 1).reshape(Q, -1, 32).max(2)  # [Q, tiles]
    for k in (100, 1000):
        Mk = np.sort(m, axis=1)[:, -k][:, None]
        row_cap = int((s >= Mk - 2 * eps).sum())
        tile_cap = int((m >= Mk - 4 * eps).sum())
        out = _c_deep(device, qd, gd, k, Q * m.shape[1], Q * N, 0.0, ix.norm_bound_dev, split)
        torch.cuda.synchronize(device)
        listed, surv = out[3].tolist()
        print(f"{form} N={N} k={k}: listed {listed} <= {tile_cap}, survivors {surv} <= {row_cap}, Q*k = {Q * k}")
        assert k * Q <= surv <= row_cap, (form, N, k, surv, row_cap)
        assert k * Q <= listed <= tile_cap, (form, N, k, listed, tile_cap)
        if form == "bf16":
            assert row_cap <= 1.7 * k * Q, "the cap itself is loose on this input"


# =================================================================== F. graph capture
@pytest.mark.parametrize("form", ["bf16", "f32-index"])
def test_c_call_is_graph_capturable(S, oracle, device, form):
    N, E, Q, k = 20011, 512, 16, 100
    dtype = _dtype(form)
    g = synth.synth_unit_rows(N, E, seed=131).to(dtype)
    qs = [synth.synth_unit_rows(Q, E, seed=132 + i).to(dtype) for i in range(3)]
    gd = g.to(device)
    ix = S.GalleryIndex(gd, presplit=form == "f32-index")
    split = ix._split if form == "f32-index" else None
    cap = 8 * Q * k
    eager = []
    for q in qs:
        e = _c_deep(device, q.to(device), gd, k, cap, cap, 0.0, ix.norm_bound_dev, split, 100.0)
        torch.cuda.synchronize(device)
        assert e[3][0].item() <= cap and e[3][1].item() <= cap
        eager.append([t.clone() for t in e[:4]])
    static_q = qs[0].to(device).clone()
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        out = _c_deep(device, static_q, gd, k, cap, cap, 0.0, ix.norm_bound_dev, split, 100.0)      # warm, outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _c_deep(device, static_q, gd, k, cap, cap, 0.0, ix.norm_bound_dev, split, 100.0, out=out)
    torch.cuda.current_stream(device).wait_stream(side)
    for i in (1, 2, 0, 1):
        static_q.copy_(qs[i].to(device))
        graph.replay()
        torch.cuda.synchronize(device)
        for a, b in zip(out[:4], eager[i]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (form, i)
        assert_topk(out, expect_topk(oracle, qs[i], g, np.ones(N, bool), k, scale=100.0))


# =================================================================== G. the BASELINE-size case
@pytest.mark.slow
def test_one_million_rows_k1000(S, oracle, device):
    N, E, Q, k = 1_000_000, 512, 16, 1000
    g = synth.synth_unit_rows(N, E, seed=3).bfloat16()
    q = synth.synth_unit_rows(Q, E, seed=4).bfloat16()
    ix = S.GalleryIndex(g.to(device))
    assert_topk(ix.search_deep(q.to(device), k, 100.0, return_dot64=True), expect_topk(oracle, q, g, np.ones(N, bool), k, scale=100.0))
