"""GPU: every clamped 1-D launch driven past its grid clamp at a small shape.

Some thirty launches size their grid as min(ceil(items / per_block), cap) and rely on the kernel striding over the rest by
gridDim.x (grid_1d / grid_cap, csrc/mmr_common.h).  The built-in caps bind only at a million rows or hundreds of thousands of
candidates, so mmr_debug_grid_cap lowers them: with 1 or 3 workgroups a 4 099-row problem wraps many times, the last pass
ragged, and "the clamp does not change what the kernel computes" becomes a bit-for-bit invariance.

Every test runs its public call three times:
  1. with the built-in caps, compared with the reference the call's own test uses, under that test's exactness rule;
  2. under cap = 1 and cap = 3: every output buffer -- counts, status words and documented padding included -- must hold
     the bits of run 1 (all of these calls sort or reduce deterministically);
  3. under cap = 3 the hook must report exactly the CALLS[call] clamped launches the code makes, so that no test passes
     because its shape was too small for the cap to bind or because a launch it names did not run.

SITES is the table of launch sites; tests/test_grid_clamp_host.py holds it against the text of csrc/*.hip.
"""
import collections
import contextlib
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# One row per clamped launch site.  expr: the sizing expression as it stands in the file (the host test greps for it);
# per_block / cap: the built-in rule; call: the public call whose test below drives the site past the lowered cap.
Site = collections.namedtuple("Site", "file kernel expr per_block cap call")
SITES = [
    Site("search.hip", "rownorm_max_kernel", "grid_1d(N, 4)", 4, 4096, "mmr_gallery_norm_bound"),
    Site("search.hip", "split_resid_max_kernel", "grid_1d(N, 4)", 4, 4096, "mmr_gallery_split_bf16"),
    Site("range.hip", "range_split_hi_kernel", "grid_1d(N, 4)", 4, 4096, "mmr_cosine_range"),
    Site("range.hip", "range_recheck_kernel", "grid_1d(cand_cap, 16, 8192)", 16, 8192, "mmr_cosine_range"),
    Site("range.hip", "range_emit_kernel", "grid_1d(cap)", 256, 4096, "mmr_cosine_range"),
    Site("row_lists.hip", "fill_u64_kernel", "grid_1d(n)", 256, 4096, "mmr_cosine_range"),
    Site("row_lists.hip", "label_keys_kernel", "grid_1d(N)", 256, 4096, "mmr_cluster_sums"),
    Site("sweep.hip", "sweep_recheck_kernel", "grid_1d(cand_cap, 16, 8192)", 16, 8192, "mmr_threshold_sweep"),
    Site("decide.hip", "decide_recheck_kernel", "grid_1d(cand_cap, 16, 8192)", 16, 8192, "mmr_cosine_decide"),
    Site("decide.hip", "row_mask_combine_kernel", "grid_1d(words)", 256, 4096, "mmr_row_mask_combine"),
    Site("decide.hip", "decision_counts_kernel", "grid_1d(N, 256, 1024)", 256, 1024, "mmr_decision_counts"),
    Site("assign.hip", "assign_merge_kernel", "grid_1d(N)", 256, 4096, "mmr_cosine_assign"),
    Site("assign.hip", "assign_recheck_kernel", "grid_1d(amb_cap, 16, 8192)", 16, 8192, "mmr_cosine_assign"),
    Site("assign.hip", "assign_score_kernel", "grid_1d(N, 16, 8192)", 16, 8192, "mmr_cosine_assign"),
    Site("cluster.hip", "cluster_final_kernel", "grid_1d((int64_t)K * E)", 256, 4096, "mmr_cluster_sums"),
    Site("cluster_rank.hip", "rank_order_kernel", "grid_1d(N)", 256, 4096, "mmr_cluster_rank"),
    Site("cluster_rank.hip", "trim_labels_kernel", "grid_1d(N)", 256, 4096, "mmr_cluster_percentile_trim"),
    Site("silhouette.hip", "silhouette_keys_kernel", "grid_1d(N)", 256, 4096, "mmr_silhouette_sums"),
    Site("silhouette.hip", "silhouette_samples_kernel", "grid_1d(N)", 256, 4096, "mmr_silhouette_samples"),
    Site("hash_join.hip", "hash_fill_kernel", "grid_1d(cap)", 256, 4096, "mmr_hash_self_join"),
    Site("hash_join.hip", "hash_join_kernel", "grid_1d(ntiles, 1, HJ_MAX_GRID)", 1, 1 << 20, "mmr_hash_self_join"),
    Site("hash_join.hip", "hash_emit_kernel", "grid_1d(cap)", 256, 4096, "mmr_hash_self_join"),
    # per_block: 256 * DL_PER / qpad tiles, 64 at qpad = 32 and 8 at qpad = 256
    Site("deep_topk.hip", "deep_list_kernel", "grid_1d(p.geom.ntiles, 256 * DL_PER / qpad, 2048)", 64, 2048, "mmr_cosine_topk_deep"),
    Site("deep_topk.hip", "deep_rescore_kernel", "grid_1d(tile_cap, 4, 8192)", 4, 8192, "mmr_cosine_topk_deep"),
    Site("deep_qmask.hip", "deep_rescore_qm_kernel", "grid_1d(tile_cap, 4, 8192)", 4, 8192, "mmr_cosine_topk_deep_qmasked"),
    Site("vit_ops.hip", "im2col_kernel", "grid_1d(total, 256, 8192)", 256, 8192, "mmr_tower_forward"),
    # hand-written rules: grid_cap() applies the override to the grid the file's own expression gives
    Site("jpeg.hip", "jpeg_idct_kernel", "grid_cap((unsigned)(g1 < 1 ? 1 : (g1 > JP_MAX_GRID ? JP_MAX_GRID : g1)))", 32, 2048,
         "mmr_jpeg_decode_device"),
    Site("jpeg.hip", "jpeg_color_kernel", "grid_cap((unsigned)(g2 < 1 ? 1 : (g2 > JP_MAX_GRID ? JP_MAX_GRID : g2)))", 256, 2048,
         "mmr_jpeg_decode_device"),
    # gridDim.y: groups of TG_BB = 4 betas, at most 2048 / gridDim.x of them
    Site("tip_grid.hip", "tip_grid_cache_kernel", "grid_cap(std::min(groups, std::max(1u, 2048u / gx)))", 4, 2048, "mmr_tip_adapter_grid"),
]
# No clamped launch was left off the hook: every kernel above strides by gridDim (or, the JPEG pair, cuts its list into
# gridDim.x spans) and none waits for another workgroup.

# The clamped launches each public call makes under cap = 3 at the shape its test uses, counted from the code: the launches
# of SITES it reaches, plus, for the search calls, which are given no norm bound here and measure it first,
# rownorm_max_kernel (1025 workgroups of 4 rows at N = 4099).  The tests assert EQUALITY, so a launch that did not clamp,
# or did not run, is noticed; the capacities are chosen so that no call is repeated at a larger one.
CALLS = {
    "mmr_gallery_norm_bound": 1,
    "mmr_gallery_split_bf16": 1,
    "mmr_cosine_range": 4,                  # norm bound, fill, recheck, emit; fp32 without a hi half: + range_split_hi
    "mmr_gallery_self_join": 4,             # the same
    "mmr_threshold_sweep": 2,               # norm bound, recheck; fp32: + range_split_hi
    "mmr_threshold_sweep_qmasked": 2,
    "mmr_cosine_decide": 2,                 # norm bound, recheck; fp32: + range_split_hi
    "mmr_row_mask_combine": 1,
    "mmr_decision_counts": 1,
    "mmr_cosine_assign": 4,                 # norm bound, merge (one pass at K = 33), recheck, score
    "mmr_cluster_sums": 2,                  # label keys, final
    "mmr_cluster_rank": 1,
    "mmr_cluster_percentile_trim": 1,
    "mmr_silhouette_sums": 1,
    "mmr_silhouette_samples": 1,            # the Python call computes the sums first: one more
    "mmr_hash_self_join": 3,                # fill, join, emit
    "mmr_hash_cross_join": 3,
    "mmr_cosine_topk_deep": 4,              # survivor padding fill, norm bound, list (one query chunk), rescore
    "mmr_cosine_topk_deep_qmasked": 4,
    "mmr_jpeg_decode_device": 2,
    "mmr_tower_forward": 1,                 # the im2col route of the vision embedding
    "mmr_tip_adapter_grid": 1,
}
CAPS = (3, 1)          # the ragged three first: a failure names the cap it was seen under


def blocks(items, per_block):
    return -(-items // per_block)


# ------------------------------------------------------------------ the hook
_SET = [0]          # the override this module has in force (the library reports clamped launches, not the override)


@contextlib.contextmanager
def grid_cap(cap):
    """The override for the body; always restored.  .clamped: the launches the override made smaller.
    The library reports clamped launches, not the override in force, so the exit check (the override at exit is the one
    this block set) is local to this module: it sees a nested or leaked use of grid_cap(), not an override that other
    code set through the C call."""
    from mmr_amd import _lib
    L = _lib.lib()
    assert cap >= 1 and _SET[0] == 0, "nested override"
    assert L.mmr_debug_grid_cap(cap) >= 0
    _SET[0] = cap
    box = types.SimpleNamespace(clamped=None)
    try:
        yield box
        torch.cuda.synchronize()
    finally:
        mine = _SET[0] == cap
        _SET[0] = 0
        box.clamped = L.mmr_debug_grid_cap(0)
    assert mine, "the override in force at exit was not the one this block set"


def _bits(t):
    """A tensor as integers of its element size on the host: NaN payloads and signed zeros count"""
    t = t.detach().contiguous().cpu()
    if t.is_floating_point():
        t = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def assert_same_bits(base, got, what):
    assert len(base) == len(got), what
    for i, (a, b) in enumerate(zip(base, got)):
        if isinstance(a, torch.Tensor):
            assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, i, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
            x, y = _bits(a), _bits(b)
            if not torch.equal(x, y):
                bad = torch.nonzero((x != y).reshape(-1)).reshape(-1)
                raise AssertionError(f"{what}: output {i} differs in {bad.numel()} of {x.numel()} elements, first at {bad[:8].tolist()}")
        else:
            assert a == b, (what, i, a, b)


def three_runs(call, run, check, extra=0, same=None, check_all=False):
    """run() -> tuple of output tensors (and plain values).  Run 1 against the reference, then cap 3 and cap 1.
    same: the comparison of a capped run with run 1 (default: every output bit for bit); check_all: the capped runs are
    held to `check` as well (for an output the call leaves partly unspecified)."""
    same = same or assert_same_bits
    from mmr_amd import _lib
    assert _lib.lib().mmr_debug_grid_cap(0) >= 0            # counter cleared, built-in caps
    base = run()
    torch.cuda.synchronize()
    assert _lib.lib().mmr_debug_grid_cap(0) == 0, "a launch was clamped with no override set"
    check(base)
    for cap in CAPS:
        with grid_cap(cap) as g:
            got = run()
        print(f"{call}: cap {cap}: {g.clamped} clamped launches ({CALLS[call] + extra} expected at cap 3)")
        same(base, got, f"{call} under a cap of {cap} workgroups")
        if check_all:
            check(got)
        if cap == 3:
            assert g.clamped == CALLS[call] + extra, (call, g.clamped, CALLS[call] + extra)
    return base


# ------------------------------------------------------------------ shared fixtures
N_ROWS, E_DIM = 4099, 128


@pytest.fixture(scope="module")
def S(device):
    from mmr_amd import search
    return search


@pytest.fixture(scope="module")
def C(device):
    from mmr_amd import cluster
    return cluster


@pytest.fixture(scope="module")
def L(device):
    from mmr_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def oracle():
    from oracle import search_ref
    return search_ref


@pytest.fixture(scope="module")
def ref(oracle):
    return oracle._load()


def _f32(x):
    return np.ascontiguousarray(x.detach().float().cpu().numpy())


# ------------------------------------------------------------------ norm bound and split residual
@pytest.mark.parametrize("where", ["last three rows", "row 0"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_norm_bound(L, device, dtype, where):
    import margin_helpers as M
    import test_margin_inputs_gpu as MI
    N, E = 1003, E_DIM
    assert blocks(N, 4) == 251 > 3
    gen = torch.Generator().manual_seed(17)
    base = ((2 * torch.rand(N, E, generator=gen) - 1) * (1.2 / E ** 0.5)).to(dtype)
    row = (1 + torch.rand(E, generator=gen)).to(dtype)
    base[N - 2 if where == "last three rows" else 0] = row
    exact = float(M.exact_norm2(row[None, :])[0])
    gd = base.to(device)

    def run():
        out = torch.full((1,), -1.0, dtype=torch.float32, device=device)
        L.check(L.lib().mmr_gallery_norm_bound(gd.data_ptr(), L.dtype_code(dtype), N, E, out.data_ptr(), L.stream_ptr(device)))
        return (out,)

    three_runs("mmr_gallery_norm_bound", run, lambda o: MI._pin(float(o[0]), exact, MI.UP_G, f"{dtype} {where}"))


@pytest.mark.parametrize("where", ["last three rows", "row 0"])
def test_split_residual_bound(L, device, where):
    import margin_helpers as M
    import test_margin_inputs_gpu as MI
    N, E = 1003, E_DIM
    gen = torch.Generator().manual_seed(23)
    base = (2 * torch.rand(N, E, generator=gen) - 1) * 2.0 ** -5          # residuals under 2^-14 per element
    v = (1 + torch.rand(E, generator=gen)).bfloat16().float()
    row = v + (0.3 + 0.19 * torch.rand(E, generator=gen)) * 2.0 ** -7      # 0.3 .. 0.49 ulp above a bf16 value
    assert torch.equal(row.bfloat16().float(), v)
    r = N - 1 if where == "last three rows" else 0
    base[r] = row
    exact = float(M.exact_norm2((row - row.bfloat16().float())[None, :])[0])
    gd = base.to(device)

    def run():
        hi = torch.full((N, E), 0x7fc1, dtype=torch.int16, device=device).view(torch.bfloat16)
        lo = hi.clone()
        resid = torch.full((1,), -1.0, dtype=torch.float32, device=device)
        L.check(L.lib().mmr_gallery_split_bf16(gd.data_ptr(), N, E, hi.data_ptr(), lo.data_ptr(), resid.data_ptr(), L.stream_ptr(device)))
        return hi, lo, resid

    def check(o):
        hi, lo, resid = o
        MI._pin(float(resid), exact, MI.UP_R, where)
        want_hi = base.bfloat16()
        assert torch.equal(_bits(hi), _bits(want_hi)) and torch.equal(_bits(lo), _bits((base - want_hi.float()).bfloat16()))

    three_runs("mmr_gallery_split_bf16", run, check)


# ------------------------------------------------------------------ range search and self-join
RANGE_CAP = 1100            # 5 workgroups of 256 for the fill and emit kernels, 69 of 16 for the recheck
assert blocks(RANGE_CAP, 256) == 5 and blocks(RANGE_CAP, 16) == 69 and blocks(N_ROWS, 4) == 1025


def _range_inputs(dtype):
    from mmr_amd import synth
    gal = synth.synth_unit_rows(N_ROWS, E_DIM, seed=811).to(dtype)
    q = synth.synth_unit_rows(5, E_DIM, seed=812).to(dtype)
    return q, gal


def _tau_for(s, matches):
    flat = np.sort(np.asarray(s).reshape(-1))
    return float(0.5 * (flat[-matches] + flat[-matches - 1]))


def _assert_range(res, Q, want, scale):
    offsets, idx, score, d64 = res
    offsets = offsets.cpu().numpy()
    assert offsets.shape == (Q + 1,) and offsets[0] == 0 and np.all(np.diff(offsets) >= 0)
    qids = np.repeat(np.arange(Q), np.diff(offsets))
    wq, wr, wd = want
    assert np.array_equal(qids, wq) and np.array_equal(idx.cpu().numpy(), wr)
    assert np.array_equal(d64.cpu().numpy().view(np.int64), wd.view(np.int64)), "dot64 bits differ from the oracle"
    assert np.array_equal(score.cpu().numpy(), (wd * scale).astype(np.float32))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_cosine_range(S, L, ref, device, dtype):
    import search_helpers as SH
    q, gal = _range_inputs(dtype)
    qf, gf = _f32(q), _f32(gal)
    s = qf.astype(np.float64) @ gf.astype(np.float64).T
    qd, gd = q.to(device), gal.to(device)
    extra = 1 if dtype == torch.float32 else 0          # no caller-supplied hi half: range_split_hi_kernel runs

    tau = _tau_for(s, 300)
    want = SH.oracle_range(ref, qf, gf, tau)
    assert 100 <= len(want[0]) <= RANGE_CAP
    three_runs("mmr_cosine_range", lambda: S.cosine_range(qd, gd, tau, scale=100.0, return_dot64=True, cap=RANGE_CAP, cand_cap=RANGE_CAP),
               lambda o: _assert_range(o, 5, want, 100.0), extra)

    # more matches than cap: counts keep counting, nothing is written past cap (the C call; the Python layer would retry)
    tau2 = _tau_for(s, 1500)
    want2 = SH.oracle_range(ref, qf, gf, tau2)
    total, cap, cand_cap, guard = len(want2[0]), RANGE_CAP, 4096, 64
    assert cap < total < cand_cap - 500
    code = L.dtype_code(dtype)

    def run():
        ws = torch.full((L.lib().mmr_range_workspace_bytes(N_ROWS, E_DIM, 5, cand_cap, code, 0),), 0xFF, dtype=torch.uint8, device=device)
        oq = torch.full((cap + guard,), -7, dtype=torch.int32, device=device)
        orow = torch.full((cap + guard,), -7, dtype=torch.int32, device=device)
        osc = torch.full((cap + guard,), -7.0, dtype=torch.float32, device=device)
        od = torch.full((cap + guard,), -7.0, dtype=torch.float64, device=device)
        counts = torch.full((2,), -7, dtype=torch.int64, device=device)
        L.check(L.lib().mmr_cosine_range(qd.data_ptr(), gd.data_ptr(), None, code, 5, N_ROWS, E_DIM, tau2, 1.0, 0.0, None, None, cap,
                                         cand_cap, oq.data_ptr(), orow.data_ptr(), osc.data_ptr(), od.data_ptr(), counts.data_ptr(),
                                         ws.data_ptr(), ws.numel(), L.stream_ptr(device)))
        return oq, orow, osc, od, counts

    def check(o):
        oq, orow, osc, od, counts = (t.cpu().numpy() for t in o)
        assert counts[0] == total and total <= counts[1] <= cand_cap
        assert np.array_equal(oq[:cap], want2[0][:cap]) and np.array_equal(orow[:cap], want2[1][:cap])
        assert np.array_equal(od[:cap].view(np.int64), want2[2][:cap].view(np.int64))
        assert (oq[cap:] == -7).all() and (orow[cap:] == -7).all() and (osc[cap:] == -7).all() and (od[cap:] == -7).all()

    three_runs("mmr_cosine_range", run, check, extra)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_gallery_self_join(S, ref, device, dtype):
    import search_helpers as SH
    _, gal = _range_inputs(dtype)
    gf = _f32(gal)
    g64 = gf.astype(np.float64)
    s = g64 @ g64.T
    tau = _tau_for(s[np.triu_indices(N_ROWS, 1)], 300)
    want = SH.oracle_join(ref, gf, tau)
    assert 100 <= len(want[0]) <= RANGE_CAP
    gd = gal.to(device)

    def check(o):
        i, j, score, d64 = o
        assert np.array_equal(i.cpu().numpy(), want[0]) and np.array_equal(j.cpu().numpy(), want[1])
        assert np.array_equal(d64.cpu().numpy().view(np.int64), want[2].view(np.int64))
        assert np.array_equal(score.cpu().numpy(), (want[2] * 100.0).astype(np.float32))

    three_runs("mmr_gallery_self_join", lambda: S.gallery_self_join(gd, tau, scale=100.0, cap=RANGE_CAP, cand_cap=RANGE_CAP), check,
               1 if dtype == torch.float32 else 0)


# ------------------------------------------------------------------ threshold sweep
def _sweep_outputs(res):
    return res.tp, res.fp, res.pos, res.neg, tuple(res.counts)


# the per-query form of an fp32 gallery needs a caller's split; fp16 is its other recheck kernel
@pytest.mark.parametrize("dtype,masked", [(torch.bfloat16, False), (torch.float32, False), (torch.bfloat16, True), (torch.float16, True)],
                         ids=["bf16", "fp32", "qmasked-bf16", "qmasked-fp16"])
def test_threshold_sweep(S, ref, device, dtype, masked):
    import sweep_helpers as H
    Q, T = 5, 25
    gal, labels, centres = H.labelled_gallery(N_ROWS, E_DIM, seed=61, dtype=dtype)
    q, targets = H.labelled_queries(Q, E_DIM, centres, seed=62, dtype=dtype)
    thr = np.linspace(-0.2, 0.3, T)                 # where the scores are dense: some 140 pairs lie within a margin of a point
    keep = np.random.default_rng(63).random((Q, N_ROWS)) < 0.9 if masked else None
    gf, qf = H.f32(gal), H.f32(q)
    if masked:
        ge, total = np.zeros((Q, 2, T), np.int64), np.zeros((Q, 2), np.int64)
        for i in range(Q):
            a, b, _ = H.oracle_sweep(ref, qf[i:i + 1], gf, labels.numpy(), targets.numpy()[i:i + 1], thr, mask=keep[i])
            ge[i], total[i] = a[0], b[0]
    else:
        ge, total, _ = H.oracle_sweep(ref, qf, gf, labels.numpy(), targets.numpy(), thr)
    gd, qd, ld, td = gal.to(device), q.to(device), labels.to(device), targets.to(device)
    masks = torch.from_numpy(keep).to(device) if masked else None

    def check(o):
        assert np.array_equal(o[0].cpu().numpy(), ge[:, 1]) and np.array_equal(o[1].cpu().numpy(), ge[:, 0])
        assert np.array_equal(o[2].cpu().numpy(), total[:, 1]) and np.array_equal(o[3].cpu().numpy(), total[:, 0])
        done, cands = o[4]
        assert 100 <= done == cands <= 1 << 14, (done, cands)      # three passes of 48 candidates at cap = 3, and more

    three_runs("mmr_threshold_sweep_qmasked" if masked else "mmr_threshold_sweep",
               lambda: _sweep_outputs(S.threshold_sweep(qd, gd, ld, td, thr, cand_cap=1 << 14, row_masks=masks)), check,
               1 if dtype == torch.float32 else 0)           # no caller-supplied hi half: range_split_hi_kernel runs


# ------------------------------------------------------------------ decide, combine, decision counts
def _decide_inputs(dtype):
    """Unit rows and one row 64 times as long: the margin follows the longest row, so some hundred pairs are candidates"""
    from mmr_amd import synth
    gal = synth.synth_unit_rows(N_ROWS, E_DIM, seed=71).to(dtype)
    gal[N_ROWS - 2] = gal[N_ROWS - 2] * 64.0
    q = synth.synth_unit_rows(3, E_DIM, seed=72).to(dtype)
    return q, gal, np.array([0.05, 0.1, 0.0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_cosine_decide(S, ref, device, dtype):
    import decide_helpers as D
    q, gal, thr = _decide_inputs(dtype)
    want = D.oracle_decide(ref, D.f32(q), D.f32(gal), thr, slack=1e-6 * 64.0 * 1.01)
    qd, gd = q.to(device), gal.to(device)

    def run():
        res = S.cosine_decide(qd, gd, thr, cand_cap=1 << 14)
        return res.words, tuple(res.counts)

    def check(o):
        assert np.array_equal(D.words_np(o[0]), want)
        done, cands = o[1]
        assert 100 <= done == cands <= 1 << 14, (done, cands)

    three_runs("mmr_cosine_decide", run, check, 1 if dtype == torch.float32 else 0)


def test_row_mask_combine(S, device):
    """The Q x N masks mmr_cosine_decide produced, padded to 1 161 words by stacking them three times (Q = 3 gives 387),
    combined with random masks of the same shape under every op"""
    import decide_helpers as D
    q, gal, thr = _decide_inputs(torch.bfloat16)
    decided = S.cosine_decide(q.to(device), gal.to(device), thr)
    ma = S.DecisionMasks(decided.words.repeat(3, 1).contiguous(), N_ROWS)
    wa = D.words_np(ma)
    assert wa.shape == (9, 129) and wa.size == 1161 >= 1100 and blocks(wa.size, 256) == 5 and wa.any()
    b = np.random.default_rng(81).random((9, N_ROWS)) < 0.3
    wb = D.pack_bits(b)
    mb = S.DecisionMasks.from_bool(torch.from_numpy(b).to(device))
    assert np.array_equal(D.words_np(mb), wb)
    for name, fn, want in (("or", lambda: ma | mb, wa | wb), ("and", lambda: ma & mb, wa & wb), ("and-not", lambda: ma.andnot(mb), wa & ~wb)):
        three_runs("mmr_row_mask_combine", lambda: (fn().words,), lambda o: np.testing.assert_array_equal(D.words_np(o[0]), want, name))


def test_decision_counts(S, device):
    """The masks mmr_cosine_decide produced, counted against labels, targets and a row mask"""
    q, gal, thr = _decide_inputs(torch.bfloat16)
    masks = S.cosine_decide(q.to(device), gal.to(device), thr)
    bits = masks.to_bool().cpu().numpy()
    rng = np.random.default_rng(91)
    labels = rng.integers(0, 4, N_ROWS).astype(np.int32)
    targets = np.array([0, 3, 7], dtype=np.int32)                  # the last one no row carries
    live = rng.random(N_ROWS) < 0.8
    live[N_ROWS - 2:] = [False, True]                              # the ragged last block: one row dead, one live
    assert blocks(N_ROWS, 256) == 17
    ld, td, md = torch.from_numpy(labels).to(device), torch.from_numpy(targets).to(device), torch.from_numpy(live).to(device)

    def run():
        c = masks.confusion(ld, td, row_mask=md)
        return c.tp, c.fp, c.pos, c.neg

    def check(o):
        same = labels[None, :] == targets[:, None]
        want = ((bits & live & same).sum(1), (bits & live & ~same).sum(1), (live & same).sum(1), (live & ~same).sum(1))
        for got, w in zip(o, want):
            assert np.array_equal(got.cpu().numpy(), w)
        assert int(o[0].sum() + o[1].sum()) >= 100

    three_runs("mmr_decision_counts", run, check)


# ------------------------------------------------------------------ nearest-centroid assignment
@pytest.mark.parametrize("twins", [False, True], ids=["plain", "twins"])
@pytest.mark.parametrize("euclid", [False, True], ids=["nobias", "euclid"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_cosine_assign(S, ref, device, dtype, euclid, twins):
    import assign_helpers as A
    K, AMB_CAP = 33, 1100
    g, c = A.parity_fixture(E_DIM, K, N_ROWS, dtype)
    g, c = g.clone(), c.clone()
    if twins:               # last-bit twins as in test_assign_gpu.test_last_bit_twins: rows that tie between two centroids
        for a, b in ((3, 20), (5, 32)):
            c[b] = c[a]
        rows = [11 + 31 * i for i in range(128)]
        for i, r in enumerate(rows):
            g[r] = c[3 if i % 2 else 5]
    gf, cf = A.f32(g), A.f32(c)
    bias = A.euclid_bias(cf) if euclid else None
    mask = np.ones(N_ROWS, dtype=bool)
    mask[[5, 4000, 4095, 4097]] = False                            # 4096 .. 4098 are the ragged last block of 256
    mask[2000:2040] = False
    want_labels, want_best, _ = A.oracle_assign(ref, gf, cf, bias, mask)
    gd, cd, md = g.to(device), c.to(device), torch.from_numpy(mask).to(device)
    bd = None if bias is None else torch.from_numpy(bias)
    assert blocks(N_ROWS, 256) == 17 and blocks(N_ROWS, 16) == 257 and blocks(AMB_CAP, 16) == 69

    def run():
        labels, best, counts = S.cosine_assign(gd, cd, bd, row_mask=md, return_score=True, amb_cap=AMB_CAP, return_counts=True)
        return labels, best, tuple(counts)

    def check(o):
        got, gb = o[0].cpu().numpy(), o[1].cpu().numpy()
        assert np.array_equal(got, want_labels), np.flatnonzero(got != want_labels)[:8]
        assert (got[~mask] == -1).all()
        assert np.array_equal(np.isnan(gb), want_labels < 0)
        ok = want_labels >= 0
        assert np.array_equal(gb[ok].view(np.int64), want_best[ok].view(np.int64)), "best64 bits differ"
        done, amb = o[2]
        assert done == amb <= AMB_CAP
        if twins:
            assert done >= 100, done                               # more than two passes of 48 rows at cap = 3

    three_runs("mmr_cosine_assign", run, check)


# ------------------------------------------------------------------ cluster sums, rank, trim
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("K", [7, 300])
def test_cluster_sums(C, device, K, dtype):
    import test_cluster_gpu as TC
    N, E = N_ROWS, TC.E_SUMS
    assert blocks(K * E, 256) > 3 and blocks(N, 256) == 17
    x = 0.004 * torch.randn(N, E, generator=torch.Generator().manual_seed(N + K))
    x = (torch.round(x * 2.0 ** 30) / 2.0 ** 30).to(dtype)
    x = torch.where(x.float().abs() < 2.0 ** -40, torch.zeros_like(x), x)
    lab = TC._labels(N, K, seed=K)                                 # -1 and K are out of range, K // 2 is empty
    assert (lab == -1).any() and (lab == K).any()
    want_sums, want_sizes = TC._sequential_sums(x.to(torch.float64).numpy(), lab, K)
    xd, ld = x.to(device), torch.from_numpy(lab).to(device)

    def check(o):
        assert np.array_equal(o[1].cpu().numpy(), want_sizes)
        assert np.array_equal(o[0].cpu().numpy().view(np.int64), want_sums.view(np.int64)), "sums differ from the sequential fp64 sum"

    three_runs("mmr_cluster_sums", lambda: C.cluster_sums(xd, ld, K), check)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("E,K", [(128, 3), (512, 17)])
def test_cluster_rank_and_trim(C, device, E, K, metric):
    import trim_helpers as T
    N, dtype = N_ROWS, torch.bfloat16
    f = T.fixture(E, K, N, dtype)
    want = T.restated(E, K, N, dtype, metric)
    g, lab = f.gallery.to(device), torch.from_numpy(f.labels).to(device)
    c32 = torch.from_numpy(f.centers64.astype(np.float32)).to(device)

    def check_rank(o):
        dist, order, start = (t.cpu().numpy() for t in o)
        assert np.array_equal(T.bits(dist), T.bits(want.dist))
        assert np.array_equal(start, want.start) and np.array_equal(order, want.order)

    def rank():
        rk = C.rank_in_clusters(g, lab, K, centers=c32, metric=metric)
        return rk.dist, rk.order, rk.start

    three_runs("mmr_cluster_rank", rank, check_rank)
    rk = C.rank_in_clusters(g, lab, K, centers=c32, metric=metric)
    for q in (50.0, 95.0):
        def check_trim(o, q=q):
            thr, trimmed, kept = (t.cpu().numpy() for t in o)
            assert np.array_equal(T.bits(thr), T.bits(want.thresholds[q]))
            assert np.array_equal(trimmed, want.trimmed[q]) and np.array_equal(kept, want.kept[q])

        three_runs("mmr_cluster_percentile_trim", lambda q=q: C.percentile_trim(rk, lab, q), check_trim)


# ------------------------------------------------------------------ silhouette
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_silhouette(C, device, dtype, metric):
    import silhouette_helpers as H
    x, lab, K, S64, B, sizes = H.case("1200x128x6", dtype, metric)
    assert blocks(x.shape[0], 256) == 5
    g, l = x.to(device), torch.from_numpy(lab).to(device)

    def check_sums(o):
        sums, got_sizes = o[0].cpu().numpy(), o[1].cpu().numpy()
        assert np.array_equal(got_sizes, sizes)
        err = np.abs(sums - S64)
        assert (err <= B).all(), (np.argwhere(err > B)[:5], err[err > B][:5])

    sums, got_sizes = three_runs("mmr_silhouette_sums", lambda: C.silhouette_sums(g, l, K, metric), check_sums)
    want = H.samples_rule(sums.cpu().numpy(), lab, got_sizes.cpu().numpy())
    live = (lab >= 0) & (lab < K)

    def check_samples(o):
        samples = o[0].cpu().numpy()
        assert np.isnan(samples[~live]).all() and not np.isnan(samples[live]).any()
        assert np.array_equal(samples[live].view(np.int64), want[live].view(np.int64))

    # the Python call computes the sums again and then the samples: both kernels clamp
    three_runs("mmr_silhouette_samples", lambda: (C.silhouette_samples(g, l, K, metric),), check_samples, 1)


# ------------------------------------------------------------------ hash joins
HASH_CAP = 1100


def _plant_every_tile(HJ, rng, rows_a, rows_b, n_a, n_b, self_join, taken):
    """One pair at distance <= 5 through kind 0 for every tile (pair of 1024-row blocks), the partial last ones included.
    rows_b is rows_a in the self-join.  -> the planted (a, b) pairs"""
    pairs = []
    ta, tb = blocks(n_a, HJ.TILE), blocks(n_b, HJ.TILE)
    for i in range(ta):
        for j in range(i if self_join else 0, tb):
            lo_a, hi_a = i * HJ.TILE, min(n_a, (i + 1) * HJ.TILE)
            lo_b, hi_b = j * HJ.TILE, min(n_b, (j + 1) * HJ.TILE)
            if self_join and i == j and hi_a - lo_a < 2:
                continue                                            # a one-row diagonal tile holds no pair
            a = next(r for r in range(hi_a - 1, lo_a - 1, -1) if ("a", r) not in taken)
            taken.add(("a", a))
            if self_join:
                taken.add(("b", a))
            free = [r for r in range(hi_b - 1, lo_b - 1, -1) if ("b", r) not in taken]
            if free:
                b = free[0]
                rows_b[b, 0] = rows_a[a, 0]
                HJ._flip(rng, rows_b[b], 0, (i + j) % 6)
            else:                                                   # a one-row tile whose row is in a pair already: copy it
                b = hi_b - 1
                rows_a[a, 0] = rows_b[b, 0]
                HJ._flip(rng, rows_a[a], 0, (i + j) % 6)
            taken.add(("b", b))
            if self_join:
                taken.add(("a", b))
            pairs.append((a, b))
    return pairs


def _hash_overflow_run(device, queries, refs, cap, guard=64):
    """The C call with `cap` below the match count (the Python layer would retry): every buffer prefilled with -7"""
    import ctypes
    from mmr_amd import _lib
    L = _lib.lib()
    N, H, W = refs.shape
    M = 0 if queries is None else queries.shape[0]
    need = L.mmr_hash_join_workspace_bytes(M, N, H, W, cap)
    thr = (ctypes.c_int32 * H)(*([5] * H))

    def run():
        ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=device)
        oi = torch.full((cap + guard,), -7, dtype=torch.int32, device=device)
        oj = torch.full((cap + guard,), -7, dtype=torch.int32, device=device)
        od = torch.full((cap + guard,), -7, dtype=torch.int64, device=device)
        counts = torch.full((1 + guard,), -7, dtype=torch.int64, device=device)
        tail = (H, W, thr, None, cap, oi.data_ptr(), oj.data_ptr(), od.data_ptr(), counts.data_ptr(), ws.data_ptr(), need,
                _lib.stream_ptr(device))
        if queries is None:
            _lib.check(L.mmr_hash_self_join(refs.data_ptr(), N, *tail))
        else:
            _lib.check(L.mmr_hash_cross_join(queries.data_ptr(), M, refs.data_ptr(), N, *tail))
        return oi, oj, od, counts
    return run


def _check_hash_overflow(o, cap, bi, bj, bd):
    """counts[0] keeps counting and nothing behind cap is touched.  Which cap of the matching pairs are stored is not
    specified (the join appends them in arrival order and stops at cap), so the stored ones are held to what the call
    does promise: cap distinct matching pairs in (i, j) order with their distances -- every slot below cap written."""
    from mmr_amd import dedup
    oi, oj, od, counts = o
    assert counts[0].item() == bi.size > cap and (counts[1:] == -7).all()
    assert (oi[cap:] == -7).all() and (oj[cap:] == -7).all() and (od[cap:] == -7).all()
    i, j = oi[:cap].cpu().numpy().astype(np.int64), oj[:cap].cpu().numpy().astype(np.int64)
    big = int(max(bi.max(), bj.max())) + 1
    assert (i >= 0).all() and (j >= 0).all() and (np.diff(i * big + j) > 0).all()
    at = np.searchsorted(bi * big + bj, i * big + j)                 # the brute-force list is in (i, j) order too
    assert (at < bi.size).all() and np.array_equal(bi[at], i) and np.array_equal(bj[at], j)
    assert np.array_equal(dedup._unpack_dist(od[:cap], bd.shape[1]).cpu().numpy(), bd[at])


def _same_hash_overflow(base, got, what):
    """Across caps: the count and the untouched slots bit for bit; the stored subset is unspecified (checked by rule)"""
    assert_same_bits(base[3:], got[3:], what)


HASH_OVER_CAP = 800          # below the match counts of the two tests, above 3 * 256: the emit wraps with a ragged last pass
assert 3 * 256 < HASH_OVER_CAP and blocks(HASH_OVER_CAP, 256) == 4


def test_hash_self_join(device):
    import test_hash_join_gpu as HJ
    from mmr_amd import dedup
    n, thr = 2 * HJ.TILE + 1, 5
    assert blocks(n, HJ.TILE) * (blocks(n, HJ.TILE) + 1) // 2 == 6            # tiles on or above the diagonal
    h = HJ._planted_set(n, thr, seed=1000 * thr + n)
    rng = np.random.default_rng(7)
    taken = {(s, r) for s in "ab" for r in (3, 5, 6, n - 1, 64)}              # the traps of _planted_set
    taken.discard(("b", n - 1))                                               # the one row of the last tile may be a copy
    taken.discard(("a", n - 1))
    pairs = _plant_every_tile(HJ, rng, h, h, n, n, True, taken)
    # 43 identical rows over the first two tiles: 903 pairs, so that hash_emit_kernel (which strides over the matches, not
    # over cap) takes a second trip at three workgroups
    same = [100 + 45 * k for k in range(43)]
    assert not {(s, r) for s in "ab" for r in same} & taken
    h[same] = h[same[0]]
    bi, bj, bd = HJ._brute_self(h, [thr] * h.shape[1])
    assert 903 <= bi.size <= HASH_CAP and bi.size > 3 * 256 and bi.size > HASH_OVER_CAP
    found = set(zip(bi.tolist(), bj.tolist()))
    assert all((min(p), max(p)) in found for p in pairs)
    assert {(int(i) // HJ.TILE, int(j) // HJ.TILE) for i, j in found} >= {(0, 0), (0, 1), (0, 2), (1, 1), (1, 2)}
    hd = torch.from_numpy(h).to(device)

    def check(o):
        i, j, d = (t.cpu().numpy() for t in o)
        assert i.size == bi.size
        assert np.array_equal(i, bi) and np.array_equal(j, bj) and np.array_equal(d, bd)

    three_runs("mmr_hash_self_join", lambda: dedup.hash_duplicate_pairs(hd, thr, cap=HASH_CAP), check)
    three_runs("mmr_hash_self_join", _hash_overflow_run(device, None, hd, HASH_OVER_CAP),
               lambda o: _check_hash_overflow(o, HASH_OVER_CAP, bi, bj, bd), same=_same_hash_overflow, check_all=True)


def test_hash_cross_join(device):
    import test_hash_join_gpu as HJ
    from mmr_amd import dedup
    m, n, thr = HJ.TILE + 76, HJ.TILE + 6, 5
    assert blocks(m, HJ.TILE) * blocks(n, HJ.TILE) == 4
    rng = np.random.default_rng(11)
    q, r = HJ._random_hashes(rng, m, 3, 1), HJ._random_hashes(rng, n, 3, 1)
    pairs = _plant_every_tile(HJ, rng, q, r, m, n, False, set())
    # 30 query rows equal to 30 ref rows, in all four tiles: 900 pairs, more than three workgroups of the emit
    qs, rs = [20 + 36 * k for k in range(30)], [10 + 35 * k for k in range(30)]
    assert not set(qs) & {a for a, _ in pairs} and not set(rs) & {b for _, b in pairs} and max(qs) >= HJ.TILE and max(rs) >= HJ.TILE
    q[qs] = q[qs[0]]
    r[rs] = q[qs[0]]
    bi, bj, bd = HJ._brute_cross(q, r, [thr] * 3)
    assert 904 <= bi.size <= HASH_CAP and bi.size > HASH_OVER_CAP and set(pairs) <= set(zip(bi.tolist(), bj.tolist()))
    qd, rd = torch.from_numpy(q).to(device), torch.from_numpy(r).to(device)

    def check(o):
        offsets, idx, d = (t.cpu().numpy() for t in o)
        assert idx.size == bi.size
        assert np.array_equal(np.repeat(np.arange(m), np.diff(offsets)), bi) and np.array_equal(idx, bj) and np.array_equal(d, bd)

    three_runs("mmr_hash_cross_join", lambda: dedup.hash_cross_matches(qd, rd, thr, cap=HASH_CAP), check)
    three_runs("mmr_hash_cross_join", _hash_overflow_run(device, qd, rd, HASH_OVER_CAP),
               lambda o: _check_hash_overflow(o, HASH_OVER_CAP, bi, bj, bd), same=_same_hash_overflow, check_all=True)


# ------------------------------------------------------------------ deep top-k
DEEP_N, DEEP_K = 50000, 300


@pytest.mark.parametrize("Q", [16, 250], ids=["qpad32", "qpad256"])
@pytest.mark.parametrize("masked", [False, True], ids=["mmr_cosine_topk_deep", "mmr_cosine_topk_deep_qmasked"])
def test_cosine_topk_deep(S, oracle, device, masked, Q):
    from mmr_amd import synth
    import search_helpers as SH
    N, E, k = DEEP_N, E_DIM, DEEP_K
    qpad = blocks(Q, 32) * 32
    assert qpad == (32 if Q == 16 else 256) and blocks(blocks(N, 32), 256 * 8 // qpad) > 3       # deep_list_kernel's workgroups
    g = synth.synth_unit_rows(N, E, seed=3 + N).bfloat16()
    q = synth.synth_unit_rows(Q, E, seed=4 + Q).bfloat16()
    if masked:
        import test_query_masks_gpu as QM
        keep = np.random.default_rng(Q).random((Q, N)) < 0.5
        want = QM._oracle_per_query(oracle, q, g, keep, k)
    else:
        want = SH.expect_topk(oracle, q, g, np.ones(N, bool), k)
    gd, qd = g.to(device), q.to(device)
    qmasks = S._row_masks_words(torch.from_numpy(keep).to(device), N) if masked else None

    def run():
        idx, score, d64, _, counts = S._deep_call(qd, gd, k, 1.0, None, None, None, None, S._RANGE_MAX_PAIRS, None, None, True,
                                                  qmasks=qmasks)
        return score, idx, d64, tuple(counts)

    def check(o):
        SH.assert_topk(o[:3], want)
        listed, surv = o[3]
        assert listed > 12 and surv >= Q * k, (listed, surv)       # the rescore wraps at 3 workgroups of 4 pairs

    three_runs("mmr_cosine_topk_deep_qmasked" if masked else "mmr_cosine_topk_deep", run, check)


# ------------------------------------------------------------------ JPEG decode
def test_jpeg_decode(device):
    import jpeg_helpers as jh
    from mmr_amd import jpeg
    gold = {name: (data, want) for name, data, want in jh.golden()}
    names = ("37x51_420_smooth", "48x64_444", "17x33_422_noise")              # three sizes, three subsamplings
    files, wants = [gold[n][0] for n in names], [gold[n][1] for n in names]
    assert blocks(72 + 144 + 36, 32) > 3 and blocks(sum(w.shape[0] * w.shape[1] for w in wants) // 4, 256) > 3

    def check(o):
        for name, got, want in zip(names, o, wants):
            assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), name     # Pillow's bytes

    three_runs("mmr_jpeg_decode_device", lambda: tuple(jpeg.decode_jpeg(files, device=device, on_unsupported="raise")), check)


# ------------------------------------------------------------------ the im2col route of the vision embedding
def test_vision_embedding_im2col(device):
    import test_encoder_stages_gpu as ES
    from mmr_amd import weights
    name, B = "ViT-B/16", 5
    cfg = ES._vision_cfg(name)
    assert cfg.patch != 32 and blocks(B * cfg.grid * cfg.grid * (3 * cfg.patch * cfg.patch // 8), 256) > 3
    w = weights.make_vision_weights(cfg, seed=1)
    tower = ES._tower(cfg, w, device)
    px = ES.position_coded_images(B, cfg.image_size).bfloat16()
    pd = px.to(device)

    def check(o):
        ES._check_vision_embed(o[0], w, cfg, px.float(), list(range(B)), f"{name} B={B}")

    three_runs("mmr_tower_forward", lambda: ES._tap(tower, pd, -1), check)


# ------------------------------------------------------------------ Tip-Adapter grid
def test_tip_adapter_grid(device):
    import test_tip_grid_gpu as TG
    import tip_grid_helpers as G
    import tip_train_helpers as T
    N, S_, C_, E, dtype = TG.CASES[-2]                              # the smallest non-trivial shape of test_tip_grid_gpu
    assert (N, S_, C_, E) == (16, 16, 2, 128)
    betas = [0.01 + 0.4 * i for i in range(17)]                     # five groups of TG_BB = 4 betas, the last with one
    alphas = [0.01, 1.51]
    assert blocks(len(betas), 4) == 5 >= 2 and len(betas) >= 2 * 4
    inp = G.make_inputs(N, S_, C_, E, dtype=dtype)

    def run():
        g = TG.run(inp, betas, alphas)
        return g.L0, g.cache, g.conf, g.f1, g.threshold, g.tp, g.fp, g.fn, g.num_vals, g.status

    def check(o):
        grid = types.SimpleNamespace(L0=o[0], cache=o[1], conf=o[2], f1=o[3], threshold=o[4], tp=o[5], fp=o[6], fn=o[7], num_vals=o[8],
                                     alphas=G.f32(alphas))
        TG.assert_stage2_equal(grid, TG.restated(grid, inp["labels"]))
        assert o[9] == 0
        b32 = G.f32(betas)
        L0_64, cache_64 = G.stage1(inp, b32, torch.float64)
        L0_32, cache_32 = G.stage1(inp, b32, torch.float32)
        for dev, r32, r64 in ((o[0], L0_32, L0_64), (o[1], cache_32, cache_64)):
            assert T.max_err(dev, r64) <= T.allowance(r32, r64)

    three_runs("mmr_tip_adapter_grid", run, check)
