"""GPU: a GalleryIndex that was mutated equals a fresh one and the host model (tests/index_model.py).

The rest of the suite tests every GalleryIndex method on an index that was just built.  The methods share cached state
-- the measured norm bound, the fp32 split and its residual bound, the lazily built split of the row_masks= calls, the
packed live words, one packed mask and one workspace per lane key -- that only update_rows, refresh_norm_bound,
delete_rows, restore_rows and dedup keep current.  Here one index lives through a scripted program of mutations and a
seeded tail, and after every step a battery of its methods must return, bit for bit, what ``fresh(index)`` returns (a
new index over the same gallery, the same rows deleted: every tensor, status and candidate count) and what the model
computes from the state of the moment with the brute-force fp64 references.  A coverage table records which
(mutation kind, method) pairs were exercised and must have no empty cell.

Next to that program:
  * fixtures from margin_helpers whose answers or candidate counts change with the margin, run through update_rows, show
    that the margin follows the state;
  * failing controls: with one piece of cache upkeep patched out (Python only; every buffer stays valid and of the same
    size, so the outcome is a wrong number) the comparisons above must name a mismatch.

Not covered here: a search or a decide captured in a hipGraph and replayed across these mutations.

tests/test_index_model_host.py checks the model and the fixtures' arithmetic without a GPU.
"""
import numpy as np
import pytest
import torch

import index_model as IM
import margin_helpers as MH
from decide_helpers import oracle_decide, words_np
from search_helpers import oracle_range
from sweep_helpers import NCLASS, labelled_gallery, oracle_sweep

pytestmark = pytest.mark.gpu

N = 20011                 # aligned_gallery_fixture's size: a ragged last tile, a partly used last mask word
TAU_DUP = 6.0             # planted duplicates have norm 3 (dot 9); two random rows of norm <= 3 stay under 9 * 0.56
TAU_RANGE = 0.55
GRID = np.array([0.2, 0.35, 0.5, 0.65, 0.8])
METHODS = ("search", "search@lane1", "search_packed", "search_deep", "search_deep+row_masks", "range_search",
           "near_duplicates", "threshold_sweep", "threshold_sweep+row_masks", "decide", "assign", "score_extent",
           "trimmed_centers", "scores")


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


# ------------------------------------------------------------------ the data
class World:
    """One labelled gallery per E (fp32 on the host, cast per index kind): unit rows with class structure, norms varied over
    0.5 .. 3, twelve planted duplicate groups of norm 3, and queries: the 7 class centres, two gallery rows, noise"""

    def __init__(self, E):
        from mmr_amd import synth
        self.E = E
        rng = np.random.default_rng(100 + E)
        g, labels, centres = labelled_gallery(N, E, seed=300 + E)
        g = g * torch.from_numpy(rng.uniform(0.5, 3.0, N).astype(np.float32))[:, None]
        noise = synth.synth_unit_rows(12, E, seed=301 + E)
        self.groups = []
        for grp in range(12):
            r0 = 37 + grp * 1601
            g[r0] *= 3.0 / g[r0].norm()
            g[r0 + 64] = g[r0]                                   # an exact copy in another tile
            g[r0 + 801] = g[r0] + 0.02 * noise[grp]
            self.groups.append((r0, r0 + 64, r0 + 801))
        g[N - 1] *= 2.9 / g[N - 1].norm()
        self.g = g.contiguous()
        self.labels = labels.numpy().astype(np.int32)
        self.centres = centres
        q = synth.synth_unit_rows(131, E, seed=302 + E)
        q[:NCLASS] = centres
        q[7] = g[self.groups[0][0]]                              # queries equal to gallery rows
        q[8] = g[N - 1]
        self.q = q.contiguous()
        self.targets = (np.arange(9) % NCLASS).astype(np.int32)
        self.thr = np.array([0.5, 0.45, 0.55, 0.5, 0.6, 0.4, 0.5, 6.0, 5.0])
        self.row_mask = rng.random(N) < 0.7
        self.rng_seed = 900 + E


_worlds = {}


def world(E):
    if E not in _worlds:
        _worlds[E] = World(E)
    return _worlds[E]


# ------------------------------------------------------------------ an index, its model and the battery
class Lifecycle:
    def __init__(self, S, oracle, ref, device, E, dtype, presplit, batches=(3, 131)):
        self.S, self.oracle, self.ref, self.dev = S, oracle, ref, device
        self.w = w = world(E)
        self.dtype = dtype
        self.M = S.GalleryIndex(w.g.to(dtype).to(device), presplit=presplit)
        self.m = IM.IndexModel(w.g.to(dtype))
        assert (self.M._split is not None) == bool(presplit and dtype == torch.float32)
        self.q = w.q.to(dtype)
        self.qd = self.q.to(device)
        self.small, self.big = batches[0], batches[-1]
        self.batches = batches
        self.labels_d = torch.from_numpy(w.labels).to(device)
        self.targets_d = torch.from_numpy(w.targets).to(device)
        self.row_mask_d = torch.from_numpy(w.row_mask).to(device)
        self.cen = w.centres.to(dtype)
        self.c64 = IM.seen(self.cen, dtype).astype(np.float64)
        self.bias = -0.5 * (self.c64 ** 2).sum(1)
        self.methods = tuple(x for x in METHODS if x != "assign" or dtype != torch.float32)     # assign: 16-bit galleries only
        self.table = set()
        self.kind = "none"
        self.prev_masks = None          # (DecisionMasks of M, of the fresh index): an EARLIER decide result, for row_masks=
        self.side = torch.cuda.Stream(device)

    # -------------------------------------------------------------- mutations: the index and the model together
    def _t(self, rows):
        return torch.as_tensor(np.asarray(rows, dtype=np.int64))

    def delete(self, rows):
        self.M.delete_rows(self._t(rows))
        self.m.delete_rows(rows)
        self.kind = "delete_rows"

    def restore(self, rows):
        self.M.restore_rows(self._t(rows))
        self.m.restore_rows(rows)
        self.kind = "restore_rows"

    def update(self, rows, values):
        self.M.update_rows(self._t(rows), values)
        self.m.update_rows(rows, values)
        self.kind = "update_rows"

    def write_refresh(self, rows, values):
        self.M.gallery[self._t(rows).to(self.dev)] = values.to(device=self.dev, dtype=self.dtype)
        self.M.refresh_norm_bound()
        self.m.write_refresh(rows, values)
        self.kind = "write_refresh"

    def dedup(self):
        F = self.m.fresh(self.M)
        got, fr = IM.run(self.M, "dedup", TAU_DUP), IM.run(F, "dedup", TAU_DUP)
        dropped, partner = self.m.dedup(self.ref, TAU_DUP, prefilter=IM.pair_rows)
        assert IM.same(got, fr) is None, ("dedup", IM.same(got, fr))
        assert IM.against_model(got, {"dropped": dropped, "partner": partner}) is None
        self.kind = "dedup"
        return dropped

    # -------------------------------------------------------------- the battery
    def _check(self, F, label, want, method, *args, fresh_kw=None, runner=IM.run, **kw):
        """``method`` on the mutated index and on the fresh one (``fresh_kw``: the keyword arguments that differ for it),
        compared bit for bit, then against the model's ``want()``; the pair goes into the coverage table.
        -> (the mutated index's return, the fresh index's)"""
        got = runner(self.M, method, *args, **kw)
        fr = runner(F, method, *args, **{**kw, **(fresh_kw or {})})
        d = IM.same(got, fr)
        assert d is None, f"after {self.kind}: {label}: '{d}' differs from the fresh index's"
        d = IM.against_model(got, want())
        assert d is None, f"after {self.kind}: {label}: '{d}' differs from the model's"
        self.table.add((self.kind, label))
        self.results.setdefault(label, []).append(got)
        return got, fr

    def _on_side_stream(self, ix, method, *args, **kw):
        """``method`` on lane 1 on a side stream while a lane-0 search of the large batch is in flight on the current one"""
        cur = torch.cuda.current_stream(self.dev)
        self.side.wait_stream(cur)
        ix.search(self.qd[:self.big], 64, return_dot64=True)
        with torch.cuda.stream(self.side):
            out = IM.run(ix, method, *args, lane=1, **kw)
        cur.wait_stream(self.side)
        return out

    def _state(self, F):
        """the caches themselves: the measured bound and the residual bound against the fresh index's, the live rows"""
        st = lambda ix: {"norm_bound": ix.norm_bound_dev, "resid": None if ix._split is None else ix._split[2], "live": ix.live_mask}
        d = IM.same(st(self.M), st(F))
        assert d is None, f"after {self.kind}: the index's {d} differs from the fresh index's"
        assert np.array_equal(self.M.live_mask.cpu().numpy(), self.m.live)

    def call(self, label, F):
        """one method of the battery on the mutated index, the fresh one and the model"""
        m, o, r, q, qd = self.m, self.oracle, self.ref, self.q, self.qd
        w = self.w
        if label == "search":
            # Q and k go up and come down again on lane 0: a workspace grown by the large call serves the small ones
            for Q in self.batches[:-1]:
                self._check(F, label, lambda: m.search(o, q[:Q], 10), "search", qd[:Q], 10, return_dot64=True, return_status=True)
            B = self.big
            self._check(F, label, lambda: m.search(o, q[:B], 64, 100.0, w.row_mask), "search", qd[:B], 64, 100.0, return_dot64=True,
                        return_status=True, row_mask=self.row_mask_d)
            self._check(F, label, lambda: m.search(o, q[7], 1), "search", qd[7], 1, return_dot64=True, return_status=True)
        elif label == "search@lane1":
            self._check(F, label, lambda: m.search(o, q[:self.small], 10), "search", qd[:self.small], 10, return_dot64=True,
                        return_status=True, runner=self._on_side_stream)
        elif label == "search_packed":
            self._check(F, label, lambda: m.search_packed(o, q[:9], 5, 100.0, 1 << 20), "search_packed", qd[:9], 5, 100.0, 1 << 20)
        elif label == "search_deep":
            self._check(F, label, lambda: m.search(o, q[:3], 300), "search_deep", qd[:3], 300, return_dot64=True)
        elif label == "search_deep+row_masks":
            pm, pf = self.prev_masks
            self._check(F, label, lambda: m.search(o, q[:9], 5, row_masks=pm), "search_deep", qd[:9], 5, return_dot64=True,
                        row_masks=pm, fresh_kw={"row_masks": pf})
        elif label == "range_search":
            self._check(F, label, lambda: m.range_search(r, q[:9], TAU_RANGE), "range_search", qd[:9], TAU_RANGE, return_dot64=True)
        elif label == "near_duplicates":
            def want():
                i, j, d = m.near_duplicates(r, TAU_DUP, prefilter=IM.pair_rows)
                return {"i": i, "j": j, "dot64": d}
            self._check(F, label, want, "near_duplicates", TAU_DUP)
        elif label == "threshold_sweep":
            self._check(F, label, lambda: m.threshold_sweep(r, q[:9], w.labels, w.targets, GRID, w.row_mask), "threshold_sweep",
                        qd[:9], self.labels_d, self.targets_d, GRID, row_mask=self.row_mask_d)
        elif label == "threshold_sweep+row_masks":
            pm, pf = self.prev_masks
            self._check(F, label, lambda: m.threshold_sweep(r, q[:9], w.labels, w.targets, GRID, row_masks=pm), "threshold_sweep",
                        qd[:9], self.labels_d, self.targets_d, GRID, row_masks=pm, fresh_kw={"row_masks": pf})
        elif label == "decide":
            got, fr = self._check(F, label, lambda: m.decide(r, q[:9], w.thr), "decide", qd[:9], w.thr)
            self.new_masks = (self.S.DecisionMasks(got["words"], N), self.S.DecisionMasks(fr["words"], N))
        elif label == "assign":
            self._check(F, label, lambda: m.assign(r, self.cen, self.bias), "assign", self.cen.to(self.dev),
                        torch.from_numpy(self.bias).to(self.dev), return_score=True)
        elif label == "score_extent":
            self._check(F, label, lambda: m.score_extent(o, q[:9], w.row_mask), "score_extent", qd[:9], row_mask=self.row_mask_d)
        elif label == "trimmed_centers":
            c32 = torch.from_numpy(self.c64.astype(np.float32)).to(self.dev)
            self._check(F, label, lambda: m.trimmed_centers(w.labels, NCLASS, self.c64), "trimmed_centers", self.labels_d, NCLASS,
                        centers=c32)
        elif label == "scores":
            self._check(F, label, lambda: m.scores(o, q[:3], 100.0), "scores", qd[:3], 100.0)
        else:
            raise KeyError(label)

    def battery(self, labels):
        """``labels`` of METHODS on M, fresh(M) and the model; decide always runs, first (its masks feed the row_masks= calls
        of the NEXT battery, so those are an earlier result of the same index)"""
        F = self.m.fresh(self.M)
        self.results = {}
        self._state(F)
        for label in ["decide"] + [x for x in labels if x != "decide" and x in self.methods]:
            self.call(label, F)
            if self.prev_masks is None:                      # the very first battery: its own decide, run before the rest
                self.prev_masks = self.first_masks = self.new_masks
        self.prev_masks = self.new_masks
        return self.results


LIGHT = ("search", "decide")


def _unit(n, E, seed):
    from mmr_amd import synth
    return synth.synth_unit_rows(n, E, seed=seed)


def run_scripted(L: Lifecycle):
    """steps 1 to 8, a battery after each, and the coverage table"""
    w, m = L.w, L.m
    E = w.E
    full = L.methods
    # 1. nothing: the baseline
    first = L.battery(full)
    gmax = m.max_norm()
    # 2. delete ~30 %: row 0, row N - 1, a whole mask word, a whole tile, the current top-1 of a query (the planted
    # duplicate groups stay, for step 7)
    rng = np.random.default_rng(w.rng_seed)
    top1 = int(m.search(L.oracle, L.q[0], 1)["idx"][0])
    planted = np.array(w.groups).ravel()
    dead = np.setdiff1d(np.concatenate([rng.choice(N, int(0.3 * N), replace=False), [0, N - 1, top1], np.arange(4096, 4128),
                                        np.arange(9600, 9632)]), planted)
    L.delete(dead)
    assert not m.live[[0, N - 1, top1]].any() and not m.live[4096:4128].any()
    L.battery(full)
    live_rows, dead_rows = np.flatnonzero(m.live), np.flatnonzero(m.dead)
    up = np.concatenate([rng.choice(np.setdiff1d(live_rows, planted), 16, replace=False), rng.choice(dead_rows, 8, replace=False), [N - 1]])
    direct_rows = np.array([5, 4100, top1, N - 2])
    original = {int(r): w.g[int(r)].clone() for r in np.concatenate([up, direct_rows])}

    def step3():
        """update live and deleted rows to 4x the largest norm; an updated deleted row stays deleted"""
        L.update(up, _unit(up.size, E, 11) * (4.0 * gmax))
        assert abs(m.max_norm() / gmax - 4.0) < 0.05 and not m.live[up[16:]].any()
        L.battery(full)

    def step4():
        """restore part of the deleted set, updated (long) rows among it"""
        L.restore(np.concatenate([dead_rows[::3], up[16:20], [0]]))
        L.battery(full)

    def step5():
        """a direct write into the gallery (a deleted row among the four), then refresh_norm_bound"""
        L.write_refresh(direct_rows, _unit(direct_rows.size, E, 12) * (6.0 * gmax))
        assert abs(m.max_norm() / gmax - 6.0) < 0.08
        L.battery(full)

    def step6():
        """the long rows go back to what they were: the bound shrinks again; state, counts and status against fresh"""
        rows = np.array(sorted(original))
        L.update(rows, torch.stack([original[int(r)] for r in rows]))
        assert m.max_norm() == gmax
        L.battery(LIGHT + ("range_search", "threshold_sweep", "search_deep"))

    def step7():
        """dedup: (dropped, partner) equal the fresh index's and the model's (Lifecycle.dedup)"""
        dropped = L.dedup()
        assert dropped.size >= 24
        L.battery(full)

    def step8():
        """restore everything: bit-identical to step 1, status and counts included"""
        L.restore(np.arange(N))
        L.prev_masks = L.first_masks                         # the row_masks= calls of step 1 used these
        again = L.battery(full)
        for label, gots in first.items():
            assert len(gots) == len(again[label])
            for got, now in zip(gots, again[label]):
                d = IM.same(got, now)
                assert d is None, f"after restoring everything, {label}: '{d}' differs from the index that never changed"

    for step in (step3, step4, step5, step6, step7, step8):
        step()
    # The coverage table: no empty cell.  Checked here, at the end of the scripted part, because that part alone must fill
    # it: the seeded tail runs a light battery and only adds to cells that are already full.  A mutation kind or a method
    # that is added belongs in the steps above, or this check says nothing about it.
    missing = [(k, x) for k in IM.MUTATIONS for x in L.methods if (k, x) not in L.table]
    assert not missing, f"(mutation, method) pairs never exercised: {missing}"


def run_tail(L: Lifecycle, steps: int = 12):
    """9. ``steps`` further mutations drawn from a seeded generator over the same kinds, a light battery after each"""
    w, m = L.w, L.m
    E = w.E
    rng = np.random.default_rng(w.rng_seed + 1)
    gmax = 3.0                                               # World: the planted duplicates' norm, the largest there is
    kinds = ["delete_rows", "update_rows", "restore_rows", "write_refresh", "dedup"]
    others = [x for x in L.methods if x not in LIGHT]
    for t in range(steps):
        kind = kinds[int(rng.integers(0, len(kinds)))]
        if kind == "delete_rows":
            L.delete(rng.choice(N, int(rng.integers(1, 3000)), replace=False))
        elif kind == "restore_rows":
            d = np.flatnonzero(m.dead)
            L.restore(rng.choice(d, d.size // 2, replace=False) if d.size else np.array([3]))
        elif kind == "dedup":
            L.dedup()
        else:
            rows = rng.choice(N, int(rng.integers(1, 40)), replace=False)
            vals = _unit(rows.size, E, 50 + t) * float(rng.choice([0.25, 1.0, 3.0, 5.0])) * gmax / 3.0
            (L.update if kind == "update_rows" else L.write_refresh)(rows, vals)
        L.battery(LIGHT + (others[t % len(others)], others[(t + 5) % len(others)]))


KINDS = [("fp32-presplit", torch.float32, True), ("fp32", torch.float32, False), ("bf16", torch.bfloat16, False),
         ("fp16", torch.float16, False)]


@pytest.mark.parametrize("name,dtype,presplit", KINDS, ids=[k[0] for k in KINDS])
def test_mutated_index_equals_fresh_index_and_model(S, oracle, ref, device, name, dtype, presplit):
    """E = 128: the scripted program, then the seeded tail on the same index"""
    L = Lifecycle(S, oracle, ref, device, 128, dtype, presplit)
    run_scripted(L)
    run_tail(L)


# E = 768, fp32 with a split, query batches on either side of the fp32 pass boundary and of the split / bf16 tier plans'
# (64 vs 128 resident queries).  The host oracles cost six times as much there, so the program is two functions, one per
# step group; the tail starts from a newly built index (its first mutations meet an index that never deleted a row).
E768_BATCHES = (64, 65, 128, 129)


def test_mutated_index_equals_fresh_index_and_model_e768_scripted(S, oracle, ref, device):
    run_scripted(Lifecycle(S, oracle, ref, device, 768, torch.float32, True, batches=E768_BATCHES))


def test_mutated_index_equals_fresh_index_and_model_e768_tail(S, oracle, ref, device):
    run_tail(Lifecycle(S, oracle, ref, device, 768, torch.float32, True, batches=E768_BATCHES))


# ------------------------------------------------------------------ (c) the margin follows the state
def _crowd_counts(index, c, device):
    thr = IM.CROWD_TAU
    labels = (torch.arange(N, dtype=torch.int32) % 5).to(device)
    targets = (torch.arange(IM.CROWD_Q, dtype=torch.int32) % 5).to(device)
    dec = IM.run(index, "decide", c.q.to(device), thr)
    swp = IM.run(index, "threshold_sweep", c.q.to(device), labels, targets, IM.CROWD_GRID)
    return dec, swp


_crowds = {}


def _crowd(dtype):
    if dtype not in _crowds:
        _crowds[dtype] = IM.LifecycleCrowd(dtype)
    return _crowds[dtype]


def _crowd_program(S, device, dtype):
    """-> per state ("zero", "long", "zero again"): (decide, sweep) returns of the mutated index and of a fresh one"""
    c = _crowd(dtype)
    index = S.GalleryIndex(c.g.to(device))
    m = IM.IndexModel(c.g)
    row = torch.tensor([c.row])
    out = {}
    for state, value in (("zero", None), ("long", c.long), ("zero again", torch.zeros_like(c.long))):
        if value is not None:
            index.update_rows(row, value[None, :])
            m.update_rows([c.row], value[None, :])
        out[state] = (_crowd_counts(index, c, device), _crowd_counts(m.fresh(index), c, device))
    return c, out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_candidate_counts_follow_the_norm_bound(S, ref, device, dtype):
    """A row of norm 4 G0 (8 G0 for bf16: index_model.CROWD_LONG) written by update_rows widens every margin: counts[1] of
    decide and of the sweep must reach the pairs within 0.9 eps(G1) of a threshold (test_index_model_host.py: that is the
    whole crowd), and writing zeros back must return them to the fresh index's"""
    c, out = _crowd_program(S, device, dtype)
    for state, ((dec, swp), (fdec, fswp)) in out.items():
        assert IM.same(dec, fdec) is None and IM.same(swp, fswp) is None, (state, IM.same(dec, fdec), IM.same(swp, fswp))
    for what, i in (("decide", 0), ("sweep", 1)):
        cands, floor = out["long"][0][i]["counts"][1], c.floor(what)
        print(f"{what} {str(dtype)[6:]}: counts[1] = {out['zero'][0][i]['counts'][1]} -> {cands} -> {out['zero again'][0][i]['counts'][1]}, "
              f"floor = {floor}")
        assert cands >= floor, f"{what}: {cands} candidates after the update, but {floor} pairs lie within 0.9 eps(G1) of a threshold"
        assert out["zero again"][0][i]["counts"] == out["zero"][0][i]["counts"]
        assert out["zero"][0][i]["counts"][1] < floor, "before the update the count is under the floor: the update is what reaches it"
    # the answers never move: the long row matches nothing
    want = oracle_decide(ref, c.qf, MH.f32(c.g), np.full(IM.CROWD_Q, IM.CROWD_TAU))
    for state in out:
        assert np.array_equal(words_np(out[state][0][0]["words"]), want), state


_aligned = {}


def _aligned_fx():
    if "a" not in _aligned:
        _aligned["a"] = IM.LifecycleAligned(128)
    return _aligned["a"]


def _aligned_index(S, device, presplit):
    """an fp32 index built over the bf16-exact gallery (residual bound 0), then the planted and anti rows written"""
    a = _aligned_fx()
    index = S.GalleryIndex(torch.from_numpy(a.before).to(device), presplit=presplit)
    if presplit:
        assert float(index._split[2].item()) == 0.0
    return a, index


def _aligned_update(a, index):
    fx = a.fx
    index.update_rows(torch.from_numpy(fx.planted), torch.from_numpy(a.after[fx.planted]))
    index.update_rows(torch.from_numpy(fx.anti), torch.from_numpy(a.after[fx.anti]))


def _taus(fx):
    return [fx.base + fx.D / 2, fx.base + fx.D]                        # test_margin_floor_gpu._taus, query 0


def _grid(fx):
    pts = {fx.base - 2.5 * fx.D, fx.base - fx.D, fx.base - fx.D / 2, fx.base + fx.D / 2, fx.base + fx.D, fx.base + 2.5 * fx.D}
    return np.array(sorted(pts), dtype=np.float64)                     # test_margin_floor_gpu._grid


def _top4(oracle, a):
    """the oracle's ranks 1 to 4 of query 0 over the updated gallery: the planted rows"""
    oi, _, od = oracle.cosine_topk(a.q[:1], a.after, 4)
    assert oi[0].tolist() == sorted(a.fx.planted.tolist())
    return {"idx": oi, "dot64": od}


def _planted_first(top4, got):
    """None, or what is wrong: the planted rows must be ranks 1 to 4 with the oracle's bits"""
    return IM.against_model({k: v[..., :4] for k, v in got.items() if k in ("idx", "dot64")}, top4)


def test_residual_bound_and_split_follow_update_rows(S, oracle, ref, device):
    a, index = _aligned_index(S, device, True)
    fx = a.fx
    _aligned_update(a, index)
    assert float(index._split[2].item()) > 0.0
    qd = torch.from_numpy(a.q).to(device)
    oi, _, od = oracle.cosine_topk(a.q[:1], a.after, 10)
    top4 = _top4(oracle, a)
    for method, kw in (("search", dict(k=10)), ("search_deep", dict(k=10))):
        got = IM.run(index, method, qd, return_dot64=True, **kw)
        assert IM.against_model(got, {"idx": oi, "dot64": od}) is None, method
        assert _planted_first(top4, got) is None
    for tau in _taus(fx):
        wq, wr, wd = oracle_range(ref, a.q, a.after, tau, slack=1e-9)
        got = IM.run(index, "range_search", qd, tau, return_dot64=True)
        assert IM.against_model(got, {"idx": wr, "dot64": wd}) is None, tau
        want = oracle_decide(ref, a.q, a.after, [tau], slack=1e-9)
        assert np.array_equal(words_np(index.decide(qd, tau)), want), tau
    labels = (np.arange(fx.N) % 3).astype(np.int32)
    targets = np.zeros(1, dtype=np.int32)
    ge, total, _ = oracle_sweep(ref, a.q, a.after, labels, targets, _grid(fx))
    res = IM.run(index, "threshold_sweep", qd, torch.from_numpy(labels).to(device), torch.from_numpy(targets).to(device), _grid(fx))
    assert IM.against_model(res, {"tp": ge[:, 1], "fp": ge[:, 0], "pos": total[:, 1], "neg": total[:, 0]}) is None


# ------------------------------------------------------------------ (d) failing controls
def test_control_stale_norm_bound(S, device, monkeypatch):
    """refresh_norm_bound reduced to its _refresh_split() call: the counts stay those of G0 and fall under the floor, and
    the comparison with the fresh index names them"""
    monkeypatch.setattr(S.GalleryIndex, "refresh_norm_bound", lambda self: self._refresh_split())
    dtype = torch.bfloat16
    c = _crowd(dtype)
    index = S.GalleryIndex(c.g.to(device))
    index.update_rows(torch.tensor([c.row]), c.long[None, :])
    monkeypatch.undo()
    fresh = S.GalleryIndex(index.gallery.clone())
    (dec, swp), (fdec, fswp) = _crowd_counts(index, c, device), _crowd_counts(fresh, c, device)
    for what, got, fr in (("decide", dec, fdec), ("sweep", swp, fswp)):
        control, floor = got["counts"][1], c.floor(what)
        print(f"control {what}: counts[1] = {control} on the stale bound, {fr['counts'][1]} fresh, floor = {floor}")
        assert fr["counts"][1] >= floor
        assert control < floor, f"{what}: the stale bound still reaches the floor -- the floor has no teeth"
        assert IM.same(got, fr) == "counts"


def _noop_refresh(monkeypatch, S):
    monkeypatch.setattr(S.GalleryIndex, "_refresh_split", lambda self: None)


def test_control_stale_split(S, oracle, device, monkeypatch):
    """_refresh_split a no-op after construction: lo and the residual bound (0) stay those of the bf16-exact gallery, and
    the planted rows are missing from search and search_deep"""
    a, index = _aligned_index(S, device, True)
    fx = a.fx
    _noop_refresh(monkeypatch, S)
    _aligned_update(a, index)
    monkeypatch.undo()
    top4 = _top4(oracle, a)
    qd = torch.from_numpy(a.q).to(device)
    for method in ("search", "search_deep"):
        got = IM.run(index, method, qd, k=10, return_dot64=True)
        assert _planted_first(top4, got) == "idx", f"control: {method} on a stale split still ranks the planted rows first"
        assert fx.planted[0] not in got["idx"].cpu().numpy()[0]
        fr = IM.run(S.GalleryIndex(index.gallery.clone(), presplit=True), method, qd, k=10, return_dot64=True)
        assert IM.same({k: got[k] for k in ("idx", "dot64")}, {k: fr[k] for k in ("idx", "dot64")}) == "idx"


def test_control_stale_qsplit(S, oracle, device, monkeypatch):
    """_qsplit not cleared: the row_masks= search of the un-split fp32 index scans the split of the gallery as it was"""
    a, index = _aligned_index(S, device, False)
    fx = a.fx
    qd = torch.from_numpy(a.q).to(device)
    keep = torch.ones(1, fx.N, dtype=torch.bool, device=device)
    keep[0, 5] = False
    index.search(qd, 10, row_masks=keep)                        # builds _qsplit
    assert index._qsplit is not None and index._split is None
    top4 = _top4(oracle, a)
    # the honest index first: the update clears _qsplit and the next call finds the planted rows
    honest = S.GalleryIndex(index.gallery.clone(), presplit=False)
    honest.search(qd, 10, row_masks=keep)
    _aligned_update(a, honest)
    assert honest._qsplit is None
    assert _planted_first(top4, IM.run(honest, "search", qd, 10, return_dot64=True, row_masks=keep)) is None
    _noop_refresh(monkeypatch, S)
    _aligned_update(a, index)
    monkeypatch.undo()
    assert index._qsplit is not None
    got = IM.run(index, "search", qd, 10, return_dot64=True, row_masks=keep)
    assert _planted_first(top4, got) == "idx", "control: a stale _qsplit still ranks the planted rows first"
    assert fx.planted[0] not in got["idx"].cpu().numpy()[0]


def test_control_stale_live_words(S, oracle, ref, device, monkeypatch):
    """the in-place repack skipped on restore_rows: restored rows stay invisible, and the comparison names the ids"""
    real = S.GalleryIndex._set_live

    def skip_on_restore(self, rows, value):
        if not value:
            return real(self, rows, value)
        self._live[self._rows_arg(rows)] = value                # the bool mask moves, the packed words do not

    L = Lifecycle(S, oracle, ref, device, 128, torch.bfloat16, False)
    top1 = int(L.m.search(oracle, L.q[0], 1)["idx"][0])
    L.delete([top1, 0, N - 1])
    monkeypatch.setattr(S.GalleryIndex, "_set_live", skip_on_restore)
    L.restore([top1, 0, N - 1])
    monkeypatch.undo()
    assert bool(L.M.live_mask[top1])
    got = IM.run(L.M, "search", L.qd[:3], 10, return_dot64=True, return_status=True)
    fr = IM.run(L.m.fresh(L.M), "search", L.qd[:3], 10, return_dot64=True, return_status=True)
    assert IM.against_model(got, L.m.search(oracle, L.q[:3], 10)) in ("idx", "score"), "control: the restored row is visible"
    assert IM.same(got, fr) in ("score", "idx")
    assert top1 not in got["idx"].cpu().numpy().ravel().tolist() and top1 in fr["idx"].cpu().numpy().ravel().tolist()
