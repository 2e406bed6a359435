"""GPU: fp16 galleries and queries through the whole search surface, bit for bit against the CPU oracle.

An fp16 gallery is searched as it is (no widening copy): the scans multiply fp16 operands on the f16 MFMA instructions,
the exact re-scores read the fp16 rows, and the contract is bf16's -- order (-dot64, +row), dot64 in the oracle's fixed
summation order, idx / score / dot64 bit-exact.  The oracle (oracle/search_ref.py) widens fp16 to fp32 exactly, so every
expected value here is the oracle's over the widened data; and every result must equal the same call on ``g.float()``,
``q.float()`` (the route fp16 data took before)."""

import numpy as np
import pytest
import torch

import mmr_amd
from mmr_amd import synth

import sweep_helpers as H
from search_helpers import assert_topk, dot64, expect_topk, oracle_join, oracle_range, to_np

pytestmark = pytest.mark.gpu

N_TOPK = 20011          # ragged last tile (20011 = 625 * 32 + 11), 626 tiles -> 3 tiles per scan task


@pytest.fixture(scope="module")
def S(device):
    from mmr_amd import search
    return search


@pytest.fixture(scope="module")
def oracle():
    from oracle import search_ref
    return search_ref


@pytest.fixture(scope="module")
def ref(oracle):
    return oracle._load()


def _mask_half_with_a_dead_tile(N, seed, keep=()):
    m = np.random.default_rng(seed).random(N) < 0.5
    m[5 * 32:6 * 32] = False                    # one whole 32-row tile without a live row
    m[list(keep)] = True
    return m


def _same_topk(a, b, what=""):
    """(score, idx, dot64) of two routes, bit for bit"""
    assert torch.equal(a[1], b[1]), what
    assert torch.equal(a[2].view(torch.int64), b[2].view(torch.int64)), what
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), what


# ------------------------------------------------------------------ top-k
@pytest.mark.parametrize("E", [128, 256, 512, 768, 1024])
def test_topk_every_route(S, oracle, device, E):
    """cosine_topk, GalleryIndex.search, row_mask=, search_packed and the fp32 route of the same data, Q in {1, 33, 300}
    (300: two scan passes) x k in {1, 10, 27, 64} (27, 64: past the fast path's k).  One oracle call at k = 64 serves
    every k: the lists are ordered, so top-k is a prefix of top-64."""
    g = synth.synth_unit_rows(N_TOPK, E, seed=300 + E).half()
    q = synth.synth_unit_rows(300, E, seed=400 + E).half()
    mask = _mask_half_with_a_dead_tile(N_TOPK, E)
    want = oracle.cosine_topk(q, g, 64, scale=100.0)
    want_m = expect_topk(oracle, q, g, mask, 64, scale=100.0)
    gd, qd, md = g.to(device), q.to(device), torch.from_numpy(mask).to(device)
    gf, qf = gd.float(), qd.float()
    index = S.GalleryIndex(gd)
    assert index.gallery.dtype == torch.float16 and index.gallery.data_ptr() == gd.data_ptr() and index._split is None
    for Q in (1, 33, 300):
        for k in (1, 10, 27, 64):
            what = (E, Q, k)
            w = tuple(x[:Q, :k] for x in want)
            got = S.cosine_topk(qd[:Q], gd, k, scale=100.0, return_dot64=True, return_status=True)
            assert_topk(got, w)
            if E <= 768 and k <= 10:
                assert int(got[3].sum()) == 0, ("tie-free rows certify on the fp16 scan", what, got[3].tolist())
            else:
                assert int(got[3].sum()) == Q, what               # no scan for this E / k: the exhaustive path, flagged
            gi = index.search(qd[:Q], k, scale=100.0, return_dot64=True, return_status=True)
            assert_topk(gi, w)
            assert torch.equal(gi[3], got[3]), what
            gm = S.cosine_topk(qd[:Q], gd, k, scale=100.0, return_dot64=True, row_mask=md)
            assert_topk(gm, tuple(x[:Q, :k] for x in want_m))
            packed = index.search_packed(qd[:Q], k, 100.0, 1000)
            assert packed.shape == (Q, k, 2) and packed.dtype == torch.int64
            assert torch.equal(packed[..., 0], torch.where(got[1] >= 0, got[1] + 1000, got[1])), what
            assert torch.equal(packed[..., 1], got[2].view(torch.int64)), what
            # the route fp16 data took before: widened to fp32 (status differs by design: other scans, other tiers)
            _same_topk(got, S.cosine_topk(qf[:Q], gf, k, scale=100.0, return_dot64=True), what)


@pytest.mark.parametrize("E", [512, 768])
def test_deep_topk(S, oracle, device, E):
    g = synth.synth_unit_rows(N_TOPK, E, seed=500 + E).half()
    q = synth.synth_unit_rows(5, E, seed=600 + E).half()
    mask = _mask_half_with_a_dead_tile(N_TOPK, E + 1)
    want = oracle.cosine_topk(q, g, 4096, scale=100.0)
    gd, qd = g.to(device), q.to(device)
    index = S.GalleryIndex(gd)
    for k in (100, 4096):
        w = tuple(x[:, :k] for x in want)
        got = S.cosine_topk_deep(qd, gd, k, scale=100.0, return_dot64=True)
        assert_topk(got, w)
        assert_topk(index.search_deep(qd, k, scale=100.0, return_dot64=True), w)
    gm = index.search_deep(qd, 100, scale=100.0, return_dot64=True, row_mask=torch.from_numpy(mask).to(device))
    assert_topk(gm, expect_topk(oracle, q, g, mask, 100, scale=100.0))
    _same_topk(S.cosine_topk_deep(qd, gd, 100, scale=100.0, return_dot64=True),
               S.cosine_topk_deep(qd.float(), gd.float(), 100, scale=100.0, return_dot64=True), E)


# ------------------------------------------------------------------ range search and self-join
def _check_pairs(a, b, score, d64, want, scale, what=""):
    wa, wb, wd = want
    assert np.array_equal(a.cpu().numpy().astype(np.int64), wa.astype(np.int64)), what
    assert np.array_equal(b.cpu().numpy().astype(np.int64), wb.astype(np.int64)), what
    assert np.array_equal(d64.cpu().numpy().view(np.int64), wd.view(np.int64)), what
    assert np.array_equal(score.cpu().numpy(), (wd * scale).astype(np.float32)), what


def _check_range(res, Q, want, scale, what=""):
    offsets, idx, score, d64 = res
    offsets = offsets.cpu().numpy()
    assert offsets.shape == (Q + 1,) and offsets[0] == 0 and np.all(np.diff(offsets) >= 0), what
    _check_pairs(torch.from_numpy(np.repeat(np.arange(Q), np.diff(offsets))), idx, score, d64, want, scale, what)


def _planted(E, seed):
    """3001 fp16 unit rows; row 77 / row 78 are row 1234 with its largest element one fp16 ulp up / down, and query 1 IS
    row 1234: dot(q1, row 1234) = tau exactly, the two neighbours sit one fp16 ulp of one element either side of it."""
    g = synth.synth_unit_rows(3001, E, seed=seed).half()
    q = synth.synth_unit_rows(7, E, seed=seed + 1).half()
    base = g[1234].clone()
    j = int(base.float().abs().argmax())
    for row, step in ((77, 1), (78, -1)):
        v = base.clone()
        v.view(torch.int16)[j] += step
        g[row] = v
    q[1] = base
    return g, q


@pytest.mark.parametrize("E", [128, 768])
def test_range_search_and_self_join(S, ref, device, E):
    g, q = _planted(E, 700 + E)
    gf, qf = np.ascontiguousarray(to_np(g)), np.ascontiguousarray(to_np(q))
    gd, qd = g.to(device), q.to(device)
    index = S.GalleryIndex(gd)
    mask = _mask_half_with_a_dead_tile(3001, E, keep=(1234, 77))
    mask[78] = False
    md = torch.from_numpy(mask).to(device)
    s = qf.astype(np.float64) @ gf.astype(np.float64).T
    d0 = dot64(ref, qf[1], gf[1234])
    near = sorted(dot64(ref, qf[1], gf[r]) for r in (77, 78))
    assert near[0] < d0 < near[1], "the planted rows straddle the threshold"
    for tau in (d0, float(np.quantile(s, 1 - 2000.0 / s.size))):
        for m, mdev in ((None, None), (mask, md)):
            want = oracle_range(ref, qf, gf, tau, m)
            what = (E, tau, m is not None)
            res = S.cosine_range(qd, gd, tau, scale=100.0, return_dot64=True, row_mask=mdev)
            _check_range(res, 7, want, 100.0, what)
            _check_range(index.range_search(qd, tau, scale=100.0, return_dot64=True, row_mask=mdev), 7, want, 100.0, what)
            rf = S.cosine_range(qd.float(), gd.float(), tau, scale=100.0, return_dot64=True, row_mask=mdev)
            assert all(torch.equal(x, y) for x, y in zip(res, rf)), what
            if tau == d0:       # the tie is in, exactly one neighbour is in (unmasked), row 78 is masked out
                rows = res[1][int(res[0][1]):int(res[0][2])].tolist()
                assert 1234 in rows and 78 not in rows if m is not None else (77 in rows) != (78 in rows), (what, rows)
    # self-join: thresholds on the planted pairs' exact dots, and a natural one with a few hundred pairs
    g64 = gf.astype(np.float64)
    ss = np.triu(g64 @ g64.T, 1)
    taus = [dot64(ref, gf[77], gf[1234]), dot64(ref, gf[78], gf[1234]), float(np.sort(ss[ss != 0])[-400])]
    for tau in taus:
        for m, mdev in ((None, None), (mask, md)):
            want = oracle_join(ref, gf, tau, m)
            what = (E, "join", tau, m is not None)
            res = S.gallery_self_join(gd, tau, scale=100.0, row_mask=mdev)
            _check_pairs(*res, want, 100.0, what)
            _check_pairs(*index.near_duplicates(tau, scale=100.0, row_mask=mdev), want, 100.0, what)
            rf = S.gallery_self_join(gd.float(), tau, scale=100.0, row_mask=mdev)
            assert all(torch.equal(x, y) for x, y in zip(res, rf)), what
    got = S.gallery_self_join(gd, taus[0])
    pairs = set(zip(got[0].tolist(), got[1].tolist()))
    assert (77, 1234) in pairs, "the pair that ties the threshold is a match"


# ------------------------------------------------------------------ threshold sweep
def test_threshold_sweep(S, ref, device):
    N, Q, E = 10007, 7, 512                     # 313 tiles: two tiles per scan task
    gal, labels, centres = H.labelled_gallery(N, E, seed=81, dtype=torch.float16)
    q, targets = H.labelled_queries(Q, E, centres, seed=82, dtype=torch.float16)
    gf, qf = H.f32(gal), H.f32(q)
    gd, qd, ld, td = gal.to(device), q.to(device), labels.to(device), targets.to(device)
    index = S.GalleryIndex(gd)
    mask = _mask_half_with_a_dead_tile(N, 83)
    _, _, d64 = S.cosine_topk(qd, gd, k=10, return_dot64=True)
    d = d64.cpu().numpy().reshape(-1)                       # the exact dots of 70 pairs: an uneven grid that sits on data
    on_data = np.unique(np.concatenate([d, np.nextafter(d, np.inf), np.nextafter(d, -np.inf)]))
    grids = {"even200": np.linspace(-0.2, 0.6, 200), "even1001": np.linspace(-0.2, 0.6, 1001), "on data": on_data}
    for name, thr in grids.items():
        want_ge, want_total, redecided = H.oracle_sweep(ref, qf, gf, labels.numpy(), targets.numpy(), thr)
        res = S.threshold_sweep(qd, gd, ld, td, thr)
        done, cands = res.counts
        print(f"{name}: oracle re-decided {redecided} pairs; candidates {cands} of {Q * N} pairs")
        H.check_sweep(res, want_ge, want_total)
        assert done == cands > 0 and cands < Q * N, (name, res.counts)      # both the decided and the ambiguous path ran
        H.check_sweep(index.threshold_sweep(qd, ld, td, thr), want_ge, want_total)
        rf = S.threshold_sweep(qd.float(), gd.float(), ld, td, thr)
        assert all(torch.equal(getattr(res, f), getattr(rf, f)) for f in ("tp", "fp", "pos", "neg")), name
    thr = grids["even200"]
    want_ge, want_total, _ = H.oracle_sweep(ref, qf, gf, labels.numpy(), targets.numpy(), thr, mask)
    H.check_sweep(index.threshold_sweep(qd, ld, td, thr, row_mask=torch.from_numpy(mask).to(device)), want_ge, want_total)


# ------------------------------------------------------------------ ties and crowded boundaries
def test_tie_rule_lowest_row_first(S, oracle, device):
    """40 copies of one row spread over the gallery's tiles; the query is that row, so ranks 1..41 tie and k = 10 cuts
    inside the tie: the ten lowest row ids, in order."""
    E, N = 512, 8192
    g = synth.synth_unit_rows(N, E, seed=91).half()
    q = synth.synth_unit_rows(3, E, seed=92).half()
    dup = sorted(np.random.default_rng(9).choice(np.arange(200, N), 40, replace=False).tolist())
    g[dup] = g[123].clone()
    q[0] = g[123]
    got = S.cosine_topk(q.to(device), g.to(device), 10, return_dot64=True, return_status=True)
    assert_topk(got, oracle.cosine_topk(q, g, 10))
    assert got[1][0].tolist() == [123] + dup[:9]
    _same_topk(got, S.cosine_topk(q.float().to(device), g.float().to(device), 10, return_dot64=True))


def test_crowded_boundary_goes_to_the_exact_path(S, oracle, device):
    """60 rows within a few fp16 ulps of one element of each other (their dots differ by ~1e-6, far inside the scan's
    margin) straddle rank k in 60 different tiles -- more than the KS - k = 6 spare candidate tiles: the certificate
    rejects the query, the exhaustive path answers it exactly, and the ordinary query next to it stays certified."""
    torch.manual_seed(0)
    E = 512
    g = synth.synth_unit_rows(8192, E, seed=21).half()
    base = g[5].clone()
    rows = torch.randperm(8192)[:60]
    for j, r in enumerate(rows.tolist()):
        v = base.clone()
        v.view(torch.int16)[j] += (j % 5) - 2
        g[r] = v
    q = base.unsqueeze(0).repeat(2, 1)
    q[1] = synth.synth_unit_rows(1, E, seed=22).half()[0]
    got = S.cosine_topk(q.to(device), g.to(device), 10, return_dot64=True, return_status=True)
    assert_topk(got, oracle.cosine_topk(q, g, 10))
    assert got[3].tolist() == [1, 0]
    gi = S.GalleryIndex(g.to(device)).search(q.to(device), 10, return_dot64=True, return_status=True)
    assert_topk(gi, oracle.cosine_topk(q, g, 10))
    assert gi[3].tolist() == [1, 0]


# ------------------------------------------------------------------ subnormal operands
def _subnormal_rows(n, E, seed):
    """every element in +-{2^-15, 2^-16, 2^-24}: all below fp16's smallest normal 2^-14"""
    rng = np.random.default_rng(seed)
    mag = np.array([2.0 ** -15, 2.0 ** -16, 2.0 ** -24])[rng.integers(0, 3, (n, E))]
    x = torch.from_numpy((mag * rng.choice([-1.0, 1.0], (n, E))).astype(np.float32)).half()
    assert torch.equal(x.float().abs().max(), torch.tensor(2.0 ** -15)) and bool((x != 0).all())
    return x


@pytest.mark.parametrize("role", ["subnormal gallery", "subnormal queries"])
def test_subnormal_operands_are_not_flushed(S, oracle, ref, device, role):
    """If the f16 MFMA flushed subnormal operands, every approximate dot here would be 0 while the margin
    8e-5 |q| G stays far below the exact dots: the scans would drop real matches and certify wrong lists."""
    E, N = 512, 4096
    if role == "subnormal gallery":
        g = _subnormal_rows(N, E, 1)
        q = torch.ones(2, E)
        q[1] = torch.from_numpy(np.random.default_rng(2).choice([-1.0, 1.0], E).astype(np.float32))
        q = q.half()
    else:
        g = synth.synth_unit_rows(N, E, seed=3).half()
        q = _subnormal_rows(2, E, 4)
    gf, qf = np.ascontiguousarray(to_np(g)), np.ascontiguousarray(to_np(q))
    s = qf.astype(np.float64) @ gf.astype(np.float64).T
    G = float(np.sqrt((gf.astype(np.float64) ** 2).sum(1)).max())
    gd, qd = g.to(device), q.to(device)
    want_top = oracle.cosine_topk(q, g, 10)
    for a in range(2):
        margin = 8e-5 * float(np.sqrt((qf[a].astype(np.float64) ** 2).sum())) * G
        tau = float(s[a].max()) / 2
        # on the CPU first: a flush cannot hide inside the margin
        assert margin < 0.1 * tau and margin < 0.1 * float(want_top[2][a, 9]), (role, a, margin, tau)
        want = oracle_range(ref, qf[a:a + 1], gf, tau, slack=1e-3 * tau)
        assert 10 < want[0].shape[0] < N // 4
        res = S.cosine_range(qd[a:a + 1], gd, tau, return_dot64=True)
        _check_range(res, 1, want, 1.0, (role, a))
    got = S.cosine_topk(qd, gd, 10, return_dot64=True, return_status=True)
    assert_topk(got, want_top)
    assert got[3].tolist() == [0, 0], "certified on the fp16 scan"
    assert float(S.gallery_norm_bound(gd)) == float(S.gallery_norm_bound(gd.float())) > 0.0


# ------------------------------------------------------------------ large values, Inf, NaN
def test_large_values_are_exact(S, oracle, device):
    E, N = 128, 4097
    rng = np.random.default_rng(11)
    g = torch.from_numpy(rng.uniform(-60000, 60000, (N, E)).astype(np.float32)).half()
    q = torch.from_numpy(rng.uniform(-60000, 60000, (3, E)).astype(np.float32)).half()
    q[0] = synth.synth_unit_rows(1, E, seed=12).half()[0]
    assert float(g.float().abs().max()) > 59000 and bool(torch.isfinite(g.float()).all())
    got = S.cosine_topk(q.to(device), g.to(device), 10, return_dot64=True, return_status=True)
    assert_topk(got, oracle.cosine_topk(q, g, 10))
    _same_topk(got, S.cosine_topk(q.float().to(device), g.float().to(device), 10, return_dot64=True))
    nb = float(S.gallery_norm_bound(g.to(device)))
    true_max = float(g.double().norm(dim=-1).max())
    assert true_max <= nb <= true_max * 1.001


def test_inf_element_and_nan_row(S, oracle, device):
    """As the bf16 cases of test_search_numeric_edges_gpu.py: +inf ranks first, NaN is absent, the measured bound is +inf
    and every query takes the exhaustive path and is still exact."""
    E, N, R, RN = 128, 4097, 2500, 3000
    g = synth.synth_unit_rows(N, E, seed=13).half()
    q = synth.synth_unit_rows(4, E, seed=14).half()
    g[R, 3] = float("inf")
    g[RN] = float("nan")
    q[0, 3], q[1, 3] = 0.25, -0.25
    gd, qd = g.to(device), q.to(device)
    assert float(S.gallery_norm_bound(gd)) == float("inf")
    got = S.cosine_topk(qd, gd, 10, scale=100.0, return_dot64=True, return_status=True)
    assert_topk(got, oracle.cosine_topk(q, g, 10, scale=100.0))
    idx, d64 = got[1].cpu().numpy(), got[2].cpu().numpy()
    assert idx[0, 0] == R and d64[0, 0] == np.inf and R not in idx[1] and RN not in idx
    assert (got[3] == 1).all(), "an infinite measured bound leaves no query on the fast path"
    few = np.zeros(N, bool)
    few[[3, 77, R, RN, N - 1]] = True                     # 4 live non-NaN rows: k = 10 reaches the -inf row, NaN stays out
    gm = S.cosine_topk(qd, gd, 10, return_dot64=True, row_mask=torch.from_numpy(few).to(device))
    assert_topk(gm, expect_topk(oracle, q, g, few, 10))
    im, dm = gm[1].cpu().numpy(), gm[2].cpu().numpy()
    assert im[1, 3] == R and dm[1, 3] == -np.inf and (im[1, 4:] == -1).all()
    # an fp32 query that overflows fp16 becomes an Inf query: wild, decided by the exact path on the fp16 values
    qbig = q.float()
    qbig[2, 5] = 1e6
    gb = S.cosine_topk(qbig.to(device), gd, 10, return_dot64=True)
    assert_topk(gb, oracle.cosine_topk(qbig.half(), g, 10))


# ------------------------------------------------------------------ index maintenance on an fp16 gallery
def test_index_update_delete_extent_and_dedup(S, oracle, device):
    E, N = 256, 5000
    g = synth.synth_unit_rows(N, E, seed=15).half()
    q = synth.synth_unit_rows(4, E, seed=16).half()
    index = S.GalleryIndex(g.to(device).clone())
    new = synth.synth_unit_rows(3, E, seed=17) * 3.0              # fp32 values: stored as fp16, the bound grows
    rows = torch.tensor([10, 2000, 4999])
    index.update_rows(rows, new)
    g2 = g.clone()
    g2[rows] = new.half()
    assert index.gallery.dtype == torch.float16 and torch.equal(index.gallery.cpu(), g2)
    assert abs(float(index.norm_bound_dev) - 3.0) < 0.01
    dead = [int(oracle.cosine_topk(q, g2, 1)[0][0, 0]), 7, 4096]
    index.delete_rows(dead)
    keep = np.ones(N, bool)
    keep[dead] = False
    assert_topk(index.search(q.to(device), 10, return_dot64=True), expect_topk(oracle, q, g2, keep, 10))
    lo, hi = index.score_extent(q.to(device))
    s = expect_topk(oracle, q, g2, keep, 1)[2][:, 0], -expect_topk(oracle, -q, g2, keep, 1)[2][:, 0]
    assert np.array_equal(hi.cpu().numpy(), s[0]) and np.array_equal(lo.cpu().numpy(), s[1])
    # dedup: later copies of a row are dropped, the first is kept
    index2 = S.GalleryIndex(g.to(device).clone())
    index2.update_rows(torch.tensor([600, 700]), g[[50, 50]])
    dropped, partner = index2.dedup(0.999)
    assert dropped.tolist() == [600, 700] and partner.tolist() == [50, 50]
    assert not bool(index2.live_mask[[600, 700]].any())


# ------------------------------------------------------------------ no copy, and the fp16 kernels are what ran
def test_no_widening_copy_and_the_fp16_scans_run(S, device):
    N, E = 131072, 512
    g = synth.synth_unit_rows(N, E, seed=18).half().to(device)
    q = synth.synth_unit_rows(4, E, seed=19).half().to(device)
    index = S.GalleryIndex(g)
    assert index.gallery.data_ptr() == g.data_ptr() and index.gallery.dtype == torch.float16
    S.cosine_topk(q, g, 10)                                 # warm: library load, attribute calls
    torch.cuda.synchronize(device)
    torch.cuda.reset_peak_memory_stats(device)
    before = torch.cuda.memory_allocated(device)
    S.cosine_topk(q, g, 10)
    torch.cuda.synchronize(device)
    growth = torch.cuda.max_memory_allocated(device) - before
    print(f"peak growth of one cosine_topk: {growth} B; gallery {g.numel() * 2} B")
    assert growth < g.numel() * 2, "a widened fp32 copy would be twice the gallery's bytes"

    labels = torch.zeros(N, dtype=torch.int32, device=device)
    targets = torch.zeros(4, dtype=torch.int32, device=device)
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        S.cosine_topk(q, g, 10)
        index.search(q, 10)
        index.range_search(q, 0.2)
        index.threshold_sweep(q, labels, targets, np.linspace(-0.2, 0.6, 200))
        torch.cuda.synchronize(device)
    names = {e.key for e in prof.key_averages()}
    kernels = sorted(n for n in names if "mmr::" in n or "_ZN3mmr" in n)
    print("\n".join(kernels))
    # the scans are kernel templates over the element type: the f16_t instantiations ran, the bf16_t ones did not.  A
    # profiler whose demangler does not know _Float16 (DF16_) reports the mangled name: both spellings are given.
    for kernel, mangled in (("scan_kernel", "11scan_kernel"), ("range_scan_kernel", "17range_scan_kernel"),
                            ("sweep_scan_kernel", "17sweep_scan_kernel")):
        needed = (f"mmr::{kernel}<_Float16,", f"_ZN3mmr{mangled}IDF16_")
        assert any(s in n for n in kernels for s in needed), (needed, kernels)
        absent = (f"mmr::{kernel}<unsigned short,", f"_ZN3mmr{mangled}It")
        assert not any(s in n for n in kernels for s in absent), (absent, kernels)
    for absent in ("scan_f32s_kernel", "scan_split_kernel", "range_split_hi_kernel", "range_queries_to_bf16_kernel",
                   "split_gallery_kernel"):
        assert not any(absent in n for n in kernels), (absent, kernels)


# ------------------------------------------------------------------ row kernels
def test_row_kernels(S, oracle, device):
    g = (synth.synth_unit_rows(777, 512, seed=3) * 3.0).half()
    r = (synth.synth_unit_rows(4, 512, seed=4) * 0.5).half()
    gd, rd = g.to(device), r.to(device)
    sim = S.similarity(gd, rd, 100.0)
    assert sim.shape == (777, 4)
    assert torch.equal(sim, S.similarity(gd.float(), rd.float(), 100.0))
    assert np.array_equal(sim.t().cpu().numpy(), oracle.similarity(r, g, 100.0))
    # l2_normalize: the fp32 quotient rounded once to fp16.  |y| <= 1, so the rounding is at most half an ulp of [0.5, 1):
    # 2^-12; the fp32 arithmetic in front of it adds ~1e-7 (the bf16 case of test_search_gpu.py: 1e-2 against 2^-9)
    x = (torch.randn(33, 512, generator=torch.Generator().manual_seed(5)) * 5).half()
    y = S.l2_normalize(x.to(device))
    assert y.dtype == torch.float16
    assert np.abs(y.float().cpu().numpy() - oracle.l2norm_rows(x)).max() <= 2.0 ** -12 + 1e-6
    nb = S.gallery_norm_bound(gd)
    assert torch.equal(nb, S.gallery_norm_bound(gd.float()))
    # Tip-Adapter logits: the existing test's expression and tolerance
    N, E, C, shots = 333, 512, 6, 16
    f = synth.synth_unit_rows(N, E, seed=41).half()
    W = synth.synth_unit_rows(C, E, seed=42).t().contiguous().half()
    Kc = synth.synth_unit_rows(C * shots, E, seed=43).t().contiguous().half()
    V = torch.nn.functional.one_hot(torch.arange(C * shots) % C, C).float()
    alpha, beta = 1.17, 5.5
    ff, Wf, Kf = f.float(), W.float(), Kc.float()
    clip_logits = 100.0 * ff @ Wf
    ref_tip = clip_logits + ((-1) * (beta - beta * (ff @ Kf))).exp() @ V * 10 * alpha
    tip, clip = S.tip_adapter_logits(f.to(device), W.to(device), Kc.to(device), V.to(device), alpha, beta, return_clip_logits=True)
    assert (clip.cpu() - clip_logits).abs().max().item() <= 2e-3
    assert (tip.cpu() - ref_tip).abs().max().item() <= 2e-3
    assert torch.equal(tip.cpu().topk(1, 1, True, True)[1], ref_tip.topk(1, 1, True, True)[1])


# ------------------------------------------------------------------ encoder outputs
def test_clip_half_returns_the_fp32_output_rounded_once(device):
    model, _ = mmr_amd.load("tiny-test", device=device, weights="synthetic")
    px = synth.synth_images(5, model.input_resolution, seed=1).to(device)
    ids = synth.synth_token_ids(6, model.context_length, model.vocab_size, seed=2).to(device)
    for normalize in (False, True):
        model.float()
        fi, ft = model.encode_image(px, normalize=normalize), model.encode_text(ids, normalize=normalize)
        assert fi.dtype == torch.float32
        assert model.half() is model and model.dtype == torch.float16
        hi, ht = model.encode_image(px, normalize=normalize), model.encode_text(ids, normalize=normalize)
        assert hi.dtype == ht.dtype == torch.float16
        assert torch.equal(hi, fi.half()) and torch.equal(ht, ft.half())
        out = torch.full((5, model.cfg.embed_dim), float("nan"), dtype=torch.float16, device=device)
        assert model.encode_image(px, normalize=normalize, out=out) is out and torch.equal(out, hi)
        with pytest.raises(ValueError):
            model.encode_image(px, out=torch.empty(5, model.cfg.embed_dim, dtype=torch.bfloat16, device=device))
    assert model.to(torch.float32).dtype == torch.float32 and model.to(torch.float16).dtype == torch.float16
    from mmr_amd import gallery
    feats = gallery.encode_gallery(model.float(), [px[:3], px[3:]], normalize=True, out_dtype=torch.float16)
    assert feats.dtype == torch.float16 and torch.equal(feats, model.encode_image(px, normalize=True).half())
    assert model.dtype == torch.float32


def test_bert_half_returns_the_fp32_output_rounded_once(device):
    from mmr_amd.config import get_bert_config
    cfg = get_bert_config("tiny-bert-test")
    enc = mmr_amd.load_text_encoder("tiny-bert-test", device=device, weights="synthetic")
    ids = torch.randint(1, cfg.vocab, (5, 12), generator=torch.Generator().manual_seed(3), dtype=torch.int32).to(device)
    for normalize in (False, True):
        f = enc.float().logits(ids, normalize=normalize)
        h = enc.half().logits(ids, normalize=normalize)
        assert f.dtype == torch.float32 and h.dtype == torch.float16 and enc.dtype == torch.float16
        assert torch.equal(h, f.half())
