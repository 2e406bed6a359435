"""The index model (tests/index_model.py) and the fixtures of test_index_lifecycle_gpu.py, checked on the CPU.

(1) Every model query, after every model mutation, against a brute-force fp64 evaluation written out here: the [Q, N]
    matrix of oracle/search_ref.c's dot64, a mask, and a sort by (-dot, +row).  The GPU tests compare an index with the
    model; this is what stands behind the model.
(2) The separations the GPU tests' floors and failing controls rely on, from the fixtures' fp64 values alone.
"""
import numpy as np
import pytest
import torch

import index_model as IM
import margin_helpers as M
from decide_helpers import pack_bits
from search_helpers import dot64

N, E, K = 300, 128, 5


@pytest.fixture(scope="module")
def oracle():
    from oracle import search_ref
    return search_ref


@pytest.fixture(scope="module")
def ref(oracle):
    return oracle._load()


def _dots(ref, q, g):
    return np.array([[dot64(ref, a, b) for b in g] for a in q], dtype=np.float64).reshape(len(q), len(g))


def _rank(d, mask, k):
    """brute-force top-k of one query: (-dot, +row) over the masked rows -> (idx [k], dot [k]) padded with -1 / -inf"""
    rows = np.flatnonzero(mask)
    order = rows[np.lexsort((rows, -d[rows]))][:k]
    idx = np.full(k, -1, dtype=np.int64)
    dd = np.full(k, -np.inf)
    idx[:order.size], dd[:order.size] = order, d[order]
    return idx, dd


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _check_queries(oracle, ref, m, q, labels, targets, cen, bias, rng, what):
    g = m.g
    qf = IM.seen(q, m.dtype)
    D = _dots(ref, qf, g)
    Q = qf.shape[0]
    row_mask = rng.random(N) < 0.7
    qmask = rng.random((Q, N)) < 0.6
    for rm in (None, row_mask):
        live = m.live if rm is None else m.live & rm
        # search / search_deep / search_packed
        for k, scale in ((1, 1.0), (7, 100.0), (N + 3, 1.0)):
            got = m.search(oracle, q, k, scale, rm)
            want = [_rank(D[a], live, k) for a in range(Q)]
            assert _eq(got["idx"], np.stack([w[0] for w in want])), (what, "search idx", k)
            assert _eq(got["dot64"], np.stack([w[1] for w in want])), (what, "search dot64", k)
            assert _eq(got["score"], (np.stack([w[1] for w in want]) * np.float64(np.float32(scale))).astype(np.float32))
        got = m.search(oracle, q, 4, 1.0, rm, row_masks=qmask)
        want = [_rank(D[a], live & qmask[a], 4) for a in range(Q)]
        assert _eq(got["idx"], np.stack([w[0] for w in want])) and _eq(got["dot64"], np.stack([w[1] for w in want])), (what, "row_masks")
        one = m.search(oracle, q[0], 3, 1.0, rm)
        assert one["idx"].shape == (3,) and _eq(one["idx"], _rank(D[0], live, 3)[0])
        p = m.search_packed(oracle, q, 3, 1.0, 1000, rm)["packed"]
        want = [_rank(D[a], live, 3) for a in range(Q)]
        assert _eq(p[..., 0], np.stack([np.where(w[0] >= 0, w[0] + 1000, -1) for w in want]))
        assert _eq(p[..., 1], np.stack([w[1] for w in want]).view(np.int64))
        # range search
        tau = float(np.sort(D[:, live].ravel())[-25]) if live.any() else 0.0           # ON a dot: the rule is inclusive
        got = m.range_search(ref, q, tau, 1.0, rm)
        hit = (D >= tau) & live[None, :]
        qs, rs = np.nonzero(hit)
        assert _eq(got["idx"], rs) and _eq(got["dot64"], D[qs, rs]), (what, "range")
        assert _eq(got["offsets"], np.concatenate([[0], np.cumsum(hit.sum(1))]))
        # decide, one threshold per query
        thr = np.array([np.sort(D[a, live])[-10] if live.sum() >= 10 else 0.0 for a in range(Q)])
        assert _eq(m.decide(ref, q, thr, rm)["words"], pack_bits((D >= thr[:, None]) & live[None, :])), (what, "decide")
        # sweep, with and without a mask per query
        grid = np.array([-0.1, 0.0, float(thr[0]), 0.3])
        grid = np.unique(grid)
        for qm in (None, qmask):
            got = m.threshold_sweep(ref, q, labels, targets, grid, rm, qm)
            for a in range(Q):
                keep = live if qm is None else live & qm[a]
                pos = labels == targets[a]
                assert _eq(got["tp"][a], [(keep & pos & (D[a] >= t)).sum() for t in grid]), (what, "tp")
                assert _eq(got["fp"][a], [(keep & ~pos & (D[a] >= t)).sum() for t in grid]), (what, "fp")
                assert got["pos"][a] == (keep & pos).sum() and got["neg"][a] == (keep & ~pos).sum()
        # score extent
        got = m.score_extent(oracle, q, rm)
        if live.any():
            assert _eq(got["hi"], D[:, live].max(1)) and _eq(got["lo"], D[:, live].min(1)), (what, "extent")
        # assign with a bias: the largest dot64 + bias, ties to the lowest centroid, dead rows -1
        cf = IM.seen(cen, m.dtype)
        S = _dots(ref, g, cf) + bias[None, :]
        got = m.assign(ref, cen, bias, rm)
        assert _eq(got["labels"], np.where(live, S.argmax(1), -1)), (what, "assign")
        assert _eq(got["best64"], np.where(live, S.max(1), np.nan))
        # trimmed centres, cosine: d = 1 - dot64(row, fp32 centre), kept iff d <= np.percentile of the class
        c64 = cf.astype(np.float64) * 0.7
        dist = 1.0 - _dots(ref, g, c64.astype(np.float32))
        lab = np.where(live, labels, -1)
        got = m.trimmed_centers(labels, K, c64, "cosine", 95.0, rm)
        keep = np.zeros(N, dtype=bool)
        for c in range(K):
            rows = np.flatnonzero(lab == c)
            assert got["sizes"][c] == rows.size
            if rows.size:
                t = np.percentile(dist[rows, c], 95.0)
                assert got["thresholds"][c] == t
                keep[rows] = dist[rows, c] <= t
        assert _eq(got["keep"], keep) and _eq(got["kept"], np.bincount(lab[keep], minlength=K)), (what, "trim")
    # scores: every row, deleted or not (the index method takes no mask)
    got = m.scores(oracle, q, 100.0)["scores"]
    assert got.shape == (N, Q) and _eq(got, (D.T * 100.0).astype(np.float32))
    assert _eq(m.scores(oracle, q[0], 100.0)["scores"], (D[0] * 100.0).astype(np.float32))


def _join(ref, g, live, tau):
    G = _dots(ref, g, g)
    i, j = np.nonzero(np.triu((G >= tau) & live[:, None] & live[None, :], 1))
    return i, j, G[i, j]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_model_queries_equal_brute_force_after_every_mutation(oracle, ref, dtype):
    from mmr_amd import synth
    rng = np.random.default_rng(11)
    g = synth.synth_unit_rows(N, E, seed=5) * torch.from_numpy(rng.uniform(0.5, 3.0, N).astype(np.float32))[:, None]
    g[17] *= 2.5 / g[17].norm()                                 # the duplicate groups clear tau = 4, no random pair does
    g[98] *= 2.2 / g[98].norm()
    g[40] = g[17]
    g[41] = g[17] * 1.0001
    g[250] = g[17]
    g[99] = g[98]
    q = synth.synth_unit_rows(4, E, seed=6)
    q[1] = g[17]                                                # a query equal to a gallery row
    labels = rng.integers(0, K, N).astype(np.int32)
    targets = np.array([0, 1, 2, 9], dtype=np.int32)
    cen = synth.synth_unit_rows(K, E, seed=7)
    cen[3] = cen[2]                                             # a tie between two centroids: the lower wins
    bias = -0.5 * (IM.seen(cen, dtype).astype(np.float64) ** 2).sum(1)
    m = IM.IndexModel(g.to(dtype))
    assert not m.ever_deleted and m.live.all()
    _check_queries(oracle, ref, m, q, labels, targets, cen, bias, rng, "built")
    # the join and the greedy pass, written out
    tau = 4.0
    i, j, d = m.near_duplicates(ref, tau, prefilter=IM.pair_rows)
    wi, wj, wd = _join(ref, m.g, m.live, tau)
    assert len(wi) >= 4 and _eq(i, wi) and _eq(j, wj) and _eq(d, wd)
    assert all(_eq(a, b) for a, b in zip(m.near_duplicates(ref, tau), (wi, wj, wd)))          # without the prefilter too

    m.delete_rows([0, N - 1, 17] + list(range(64, 96)))
    assert m.ever_deleted and not m.live[[0, N - 1, 17, 64, 95]].any() and m.live[96]
    _check_queries(oracle, ref, m, q, labels, targets, cen, bias, rng, "delete_rows")
    wi, wj, wd = _join(ref, m.g, m.live, tau)
    assert 17 not in wi and all(_eq(a, b) for a, b in zip(m.near_duplicates(ref, tau, prefilter=IM.pair_rows), (wi, wj, wd)))

    new = synth.synth_unit_rows(3, E, seed=8) * 12.0
    m.update_rows([5, 17, 5], new)                              # a deleted row among them; a repeated id: the last write
    assert _eq(m.g[5], IM.seen(new[2], dtype)) and _eq(m.g[17], IM.seen(new[1], dtype)) and not m.live[17]
    assert abs(m.max_norm() - 12.0) < 0.1
    _check_queries(oracle, ref, m, q, labels, targets, cen, bias, rng, "update_rows")

    m.restore_rows([17, 64, 65])
    assert m.live[[17, 64, 65]].all() and not m.live[66]
    _check_queries(oracle, ref, m, q, labels, targets, cen, bias, rng, "restore_rows")

    m.write_refresh([5, 17], g[[5, 17]])
    assert m.max_norm() <= 3.0 + 1e-2
    _check_queries(oracle, ref, m, q, labels, targets, cen, bias, rng, "write_refresh")

    # dedup: rows in id order, a row is dropped for the first KEPT earlier row it pairs with
    wi, wj, _ = _join(ref, m.g, m.live, tau)
    kept = np.ones(N, dtype=bool)
    partner = {}
    for r in range(N):
        for u in sorted(wi[wj == r].tolist()):
            if kept[u]:
                kept[r] = False
                partner[r] = u
                break
    before = m.live.copy()
    dropped, part = m.dedup(ref, tau, prefilter=IM.pair_rows)
    assert dropped.tolist() == sorted(partner) and part.tolist() == [partner[r] for r in sorted(partner)] and len(partner) >= 3
    assert _eq(m.live, before & kept)
    assert m.near_duplicates(ref, tau)[0].size == 0
    _check_queries(oracle, ref, m, q, labels, targets, cen, bias, rng, "dedup")

    m.restore_rows(np.arange(N))
    assert m.live.all() and m.ever_deleted
    _check_queries(oracle, ref, m, q, labels, targets, cen, bias, rng, "restore all")


def test_same_and_against_model_name_the_field():
    a = {"idx": torch.tensor([[1, 2]]), "dot64": torch.tensor([[0.5, 0.25]], dtype=torch.float64), "counts": (3, 4)}
    assert IM.same(a, {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in a.items()}) is None
    assert IM.same(a, dict(a, counts=(3, 5))) == "counts"
    assert IM.same(a, dict(a, dot64=torch.tensor([[0.5, np.nextafter(0.25, 1)]], dtype=torch.float64))) == "dot64"
    assert IM.same(a, dict(a, idx=torch.tensor([[1, 2]], dtype=torch.int32))) == "idx"            # dtype is part of the return
    assert IM.same(a, {"idx": a["idx"]}) == "fields"
    assert IM.against_model(a, {"idx": np.array([[1, 2]]), "dot64": np.array([[0.5, 0.25]])}) is None
    assert IM.against_model(a, {"idx": np.array([[1, 3]])}) == "idx"
    assert IM.against_model(a, {"idx": np.array([[1, 2, 3]])}) == "idx"
    assert IM.against_model(a, {"score": np.zeros(1)}) == "score"
    assert IM.against_model({"words": torch.tensor([[-1]], dtype=torch.int32)}, {"words": np.array([[0xFFFFFFFF]], dtype=np.uint32)}) is None
    nan = {"best64": torch.tensor([float("nan")], dtype=torch.float64)}
    assert IM.against_model(nan, {"best64": np.array([-np.nan])}) is None


# ------------------------------------------------------------------ (2) the separations of the crowd fixture
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_crowd_floor_holds_the_whole_crowd_and_a_stale_bound_misses_it(ref, dtype):
    c = IM.LifecycleCrowd(dtype)
    rng = np.random.default_rng(3)
    gf = M.f32(c.g)
    for a, r in zip(rng.integers(0, IM.CROWD_Q, 30), rng.integers(0, IM.CROWD_N, 30)):
        assert abs(c.dots[a, r] - dot64(ref, c.qf[a], gf[r])) <= 1e-15
    assert not gf[c.row].any() and gf.shape[0] == 20011
    assert 0.99 < c.G0 < 1.01 and abs(c.G1 / c.G0 - c.factor) < 0.01 * c.factor
    crowd_pairs = int(c.own.sum())
    assert crowd_pairs == IM.CROWD_N
    for what in ("decide", "sweep"):
        floor, narrow = c.floor(what), c.narrow(what)
        print(f"{what} {str(dtype)[6:]}: crowd {crowd_pairs}, floor {floor}, within 1.5 eps(G0) {narrow}")
        assert floor >= 0.99 * crowd_pairs
        assert narrow <= 0.6 * floor
    # nobody but a query's own crowd comes near tau, and the long row matches nothing
    # (the sweep's floor likewise, at all three grid points: every pair it counts is a crowd pair round 0.5)
    assert not ((c.near["decide"] <= 0.9 * c.eps1) & ~c.own).any()
    assert not ((c.near["sweep"] <= 0.9 * c.eps1) & ~c.own).any()
    assert (c.long_dots < IM.CROWD_TAU - c.eps1[:, 0]).all() and (c.long_dots < IM.CROWD_GRID.min() - c.eps1[:, 0]).all()
    assert (np.abs(c.long_dots) < 1e-2).all()
    # with the zero row in place every count is the fresh crowd's: the zero row's dots are 0, far from every threshold
    assert IM.CROWD_GRID.min() - 0.0 > 10 * c.eps1.max()


# ------------------------------------------------------------------ (2) the aligned fixture across an update
def test_aligned_fixture_is_bf16_exact_before_the_update_and_planted_first_after(oracle, ref):
    a = IM.LifecycleAligned(128)
    fx = a.fx
    assert np.array_equal(M.bf16_round(a.before), a.before), "every row bf16-exact: the residual bound is exactly 0"
    assert np.array_equal(a.before[fx.planted], np.repeat(fx.gh[None, :], 4, 0))
    assert np.array_equal(a.before[fx.anti], np.repeat(fx.gh[None, :], 2, 0))
    assert M.max_norm(a.before - M.bf16_round(a.before)) == 0.0
    changed = np.flatnonzero((a.before != a.after).any(1))
    assert sorted(changed.tolist()) == sorted(np.concatenate([fx.planted, fx.anti]).tolist())
    R = M.max_norm(a.after - M.bf16_round(a.after))
    assert abs(R - M.DELTA * np.sqrt(fx.E)) <= 1e-15 * R
    oi, _, od = oracle.cosine_topk(a.q[:1], a.after, 10)
    assert oi[0, :4].tolist() == sorted(fx.planted.tolist()) and np.all(od[0, :4] == fx.base + fx.D)
    # before the update the six rows tie at base, under the decoys: none of the planted rows is in the top 4
    bi, _, _ = oracle.cosine_topk(a.q[:1], a.before, 4)
    assert not set(bi[0].tolist()) & set(fx.planted.tolist())
    # the hi half does not change with the update, so a stale split differs in lo and in the residual bound alone
    assert np.array_equal(M.bf16_round(a.after), a.before)
    # the margin a stale residual bound (0) leaves is far under the planted error: fixtures' own arithmetic
    qh = M.bf16_round(a.q)
    weak = M.doc_margin("split", qh[:1], M.max_norm(a.after), R=0.0, qr=[0.0])[0]
    assert fx.D > 2 * weak
