"""GPU: mmr_cluster_rank / mmr_cluster_percentile_trim and the Python layer on top EQUAL the numpy restatement
(tests/trim_helpers.py): distances as bit patterns, order, start, np.percentile's thresholds bit for bit, the trimmed
labels, the kept counts and the trimmed centres, for every parity shape x {bf16, fp16, fp32} x {cosine, euclidean}."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import assign_helpers as A
import trim_helpers as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CASES = [(E, K, N, dtype, metric) for E, K, N in T.PARITY_SHAPES for dtype in T.DTYPES for metric in T.METRICS]


@pytest.fixture(scope="module")
def C(device):
    from mmr_amd import cluster
    return cluster


def on_device(f: T.Fixture, device):
    return (f.gallery.to(device), torch.from_numpy(f.labels).to(device),
            torch.from_numpy(f.centers64.astype(np.float32)).to(device))


def np64(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy()


def assert_ranking(rk, want: T.Restated, what):
    assert rk.dist.dtype == torch.float64 and rk.order.dtype == torch.int64 and rk.start.dtype == torch.int64
    got, exp = T.bits(np64(rk.dist)), T.bits(want.dist)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (what, "dist", bad[:5], np64(rk.dist)[bad[:5]], want.dist[bad[:5]])
    assert np.array_equal(np64(rk.start), want.start), (what, "start")
    assert np.array_equal(np64(rk.order), want.order), (what, "order")


@pytest.mark.parametrize("E,K,N,dtype,metric", CASES, ids=[T.case_id(*c) for c in CASES])
def test_rank_trim_and_centres_equal_the_restatement(C, device, E, K, N, dtype, metric):
    f = T.fixture(E, K, N, dtype)
    want = T.restated(E, K, N, dtype, metric)
    g, lab, c32 = on_device(f, device)
    rk = C.rank_in_clusters(g, lab, K, centers=c32, metric=metric)
    assert_ranking(rk, want, "rank")
    assert torch.equal(rk.centers, c32)
    for k in (0, K - 1):
        assert np64(rk.members(k)).tolist() == want.order[want.start[k]:want.start[k + 1]].tolist()
    for q in T.QS:
        thr, trimmed, kept = C.percentile_trim(rk, lab, q)
        assert thr.dtype == torch.float64 and trimmed.dtype == torch.int32 and kept.dtype == torch.int64
        got, exp = T.bits(np64(thr)), T.bits(want.thresholds[q])
        print(f"q={q}: thresholds differing from np.percentile: {int((got != exp).sum())} of {K}")
        assert np.array_equal(got, exp), (q, np64(thr)[got != exp], want.thresholds[q][got != exp])
        assert np.array_equal(np64(trimmed), want.trimmed[q]), q
        assert np.array_equal(np64(kept), want.kept[q]), q
    # the trimmed centres: cluster_sums over the RESTATED trimmed labels, divided in numpy
    res = C.trimmed_centers(g, lab, K, percentile=95.0, metric=metric, centers=c32)
    sums, sizes = C.cluster_sums(g, torch.from_numpy(want.trimmed[95.0]).to(device), K)
    assert np.array_equal(np64(sizes), want.kept[95.0])
    with np.errstate(invalid="ignore", divide="ignore"):
        centres = np64(sums) / want.kept[95.0].astype(np.float64)[:, None]
    assert res.centers.dtype == torch.float64 and np.array_equal(T.bits(np64(res.centers)), T.bits(centres))
    assert np.array_equal(np64(res.keep), want.trimmed[95.0] >= 0)
    assert np.array_equal(T.bits(np64(res.thresholds)), T.bits(want.thresholds[95.0]))
    assert np.array_equal(np64(res.kept), want.kept[95.0])
    assert np.array_equal(np64(res.sizes), np.diff(want.start))
    if K > 1:
        assert np.isnan(np64(res.centers)[K - 1]).all()                 # the empty cluster


@pytest.mark.parametrize("E,K,N", [(128, 1, 10), (256, 8, 70), (512, 17, 4099)])
@pytest.mark.parametrize("dtype", T.DTYPES, ids=["bf16", "fp16", "fp32"])
def test_the_default_centres_are_the_means_rounded_to_fp32_once(C, device, E, K, N, dtype):
    f = T.fixture(E, K, N, dtype)
    g, lab, _ = on_device(f, device)
    sums, sizes = C.cluster_sums(g, lab, K)
    with np.errstate(invalid="ignore", divide="ignore"):
        c64 = np64(sums) / np64(sizes).astype(np.float64)[:, None]
        c32 = c64.astype(np.float32)
    for metric in T.METRICS:
        rk = C.rank_in_clusters(g, lab, K, metric=metric)
        assert rk.centers.dtype == torch.float32
        assert np.array_equal(np.where(np.isnan(c32), np.float32(0), c32).view(np.int32),
                              np.where(np.isnan(c32), np.float32(0), np64(rk.centers)).view(np.int32))
        assert np.array_equal(np.isnan(c32), np.isnan(np64(rk.centers)))
        assert_ranking(rk, T.restate(f.g32, f.labels, K, c64, metric, qs=()), ("default centres", metric))


@pytest.mark.parametrize("E,K,N", [(128, 1, 2), (128, 3, 31), (256, 8, 70), (768, 33, 2051)])
def test_nearest_is_the_head_of_every_segment(C, device, E, K, N):
    f = T.fixture(E, K, N, torch.float16)
    want = T.restated(E, K, N, torch.float16, "euclidean")
    g, lab, c32 = on_device(f, device)
    rk = C.rank_in_clusters(g, lab, K, centers=c32, metric="euclidean")
    for shots in (1, 5, 64):
        exp = np.full((K, shots), -1, dtype=np.int64)
        for k in range(K):
            seg = want.order[want.start[k]:want.start[k + 1]][:shots]
            exp[k, :seg.size] = seg
        got = rk.nearest(shots)
        assert got.dtype == torch.int64 and np.array_equal(np64(got), exp), shots
    if K > 1:
        assert (np64(rk.nearest(5))[K - 1] == -1).all() and (np.diff(want.start) < 64).any()


@pytest.mark.parametrize("metric", T.METRICS)
def test_row_mask_and_deleted_rows_equal_labels_set_to_minus_one(C, device, metric):
    from mmr_amd import GalleryIndex
    E, K, N = 256, 8, 70
    f = T.fixture(E, K, N, torch.bfloat16)
    g, lab, _ = on_device(f, device)
    gone = np.array([0, 3, 17, 36, 69])
    mask = torch.ones(N, dtype=torch.bool, device=device)
    mask[torch.from_numpy(gone).to(device)] = False
    lab2 = lab.clone()
    lab2[~mask] = -1
    want = C.trimmed_centers(g, lab2, K, metric=metric)
    index = GalleryIndex(g)
    index.delete_rows(gone)
    for got in (C.trimmed_centers(g, lab, K, metric=metric, row_mask=mask), index.trimmed_centers(lab, K, metric=metric)):
        assert np.array_equal(T.bits(np64(got.centers)), T.bits(np64(want.centers)))
        assert torch.equal(got.keep, want.keep) and torch.equal(got.kept, want.kept) and torch.equal(got.sizes, want.sizes)
        assert np.array_equal(T.bits(np64(got.thresholds)), T.bits(np64(want.thresholds)))
        assert not bool(got.keep[~mask].any())
    # and against the restatement, from the default centres of the masked labels
    labels = np.where(np64(mask), f.labels, -1).astype(np.int32)
    live = T.live_of(labels, K)
    with np.errstate(invalid="ignore", divide="ignore"):
        sums, sizes = C.cluster_sums(g, lab2, K)
        c64 = np64(sums) / np64(sizes).astype(np.float64)[:, None]
    r = T.restate(f.g32, labels, K, c64, metric, qs=(95.0,))
    assert np.array_equal(np64(want.keep), r.trimmed[95.0] >= 0) and np.array_equal(np64(want.sizes), np.bincount(labels[live], minlength=K))


def test_the_result_does_not_depend_on_what_the_workspace_or_the_outputs_held(C, device):
    from mmr_amd import _lib
    E, K, N = 512, 17, 4099
    f = T.fixture(E, K, N, torch.bfloat16)
    g, lab, c32 = on_device(f, device)
    ws = torch.empty(_lib.lib().mmr_cluster_rank_workspace_bytes(N, E, K), dtype=torch.uint8, device=device)
    runs = []
    for fill in (0xFF, 0x00):
        ws.fill_(fill)
        rk = C.rank_in_clusters(g, lab, K, centers=c32, metric="euclidean", workspace=ws)
        thr, trimmed, kept = C.percentile_trim(rk, lab, 95.0)
        runs.append((rk, thr, trimmed, kept))
    (a, ta, la, ka), (b, tb, lb, kb) = runs
    assert np.array_equal(np64(a.dist).view(np.int64), np64(b.dist).view(np.int64))
    assert torch.equal(a.order, b.order) and torch.equal(a.start, b.start)
    assert np.array_equal(np64(ta).view(np.int64), np64(tb).view(np.int64)) and torch.equal(la, lb) and torch.equal(ka, kb)
    assert_ranking(a, T.restated(E, K, N, torch.bfloat16, "euclidean"), "poisoned workspace")


def test_an_empty_gallery_writes_only_start(C, device):
    g = torch.empty(0, 128, dtype=torch.float16, device=device)
    lab = torch.empty(0, dtype=torch.int32, device=device)
    rk = C.rank_in_clusters(g, lab, 4, centers=torch.zeros(4, 128, device=device))
    assert rk.dist.numel() == 0 and rk.order.numel() == 0 and np64(rk.start).tolist() == [0] * 5
    thr, trimmed, kept = C.percentile_trim(rk, lab, 50.0)
    assert np.isnan(np64(thr)).all() and trimmed.numel() == 0 and np64(kept).tolist() == [0] * 4
    assert (np64(rk.nearest(3)) == -1).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_outlier_filter_follows_the_reference_flow(C, device, seed):
    """Ten unit fp16 rows around a prototype, row 6 planted from another direction, through the reference's expression in
    float32 numpy (mean, 1 - f @ c, <= np.percentile(.., 95), mean): outlier_filter drops exactly the planted row and
    agrees within 10 * 2^-24 * max|x| per element, which covers the fp32 summation of ten values.  The two farthest
    distances are more than 0.5 apart, so the two arithmetics cannot disagree on the mask."""
    rows = T.reference_rows(seed)
    f = rows.float().numpy()
    want, keep, d = T.reference_outlier_filter(f)
    assert keep.tolist() == [i != 6 for i in range(10)]
    top = np.sort(d)
    assert top[-1] - top[-2] > 0.5
    got, got_keep = C.outlier_filter(rows.to(device), return_keep=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (128,)
    assert np64(got_keep).tolist() == keep.tolist()
    err = np.abs(np64(got).astype(np.float64) - want.astype(np.float64)).max()
    bound = 10 * 2.0 ** -24 * np.abs(f).max()
    print(f"seed {seed}: max difference {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(C.outlier_filter(rows.to(device)), got)


def test_the_robust_centres_example_flags_its_planted_rows():
    spec = importlib.util.spec_from_file_location("robust_centers_synthetic", os.path.join(ROOT, "examples", "robust_centers_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    report = mod.main(["--classes", "4", "--per-class", "60", "--planted", "3", "--dim", "128"])
    assert len(report) == 4
    for cls in report:
        assert sorted(cls["planted"]) == sorted(set(cls["planted"]) & set(cls["outliers"])), cls       # every planted row is flagged
        assert len(cls["outliers"]) <= 3                                                         # 5 % of 60
        assert cls["trimmed_cos"] > cls["plain_cos"]                      # the trimmed centre is nearer the prototype
        assert cls["hits"] >= 50
