"""CPU: the host side of mmr_cluster_rank / mmr_cluster_percentile_trim.  Every refusal returns its code with a message
naming the argument before anything could launch (NULL / fake pointers, meta tensors); the restatement's fixed-order dot
is the C oracle's on the fixtures' own rows; the header's percentile formula is np.percentile bit for bit; and each
planted mistake changes the result on the GPU tests' own fixtures.  Nothing here launches a kernel."""
import os

import numpy as np
import pytest
import torch

import kmeanspp_helpers as H
import trim_helpers as T
from search_helpers import dot64

F32, BF16, F16 = 0, 1, 2


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


# ------------------------------------------------------------------ declarations and exports
def test_the_header_declares_the_calls_and_the_package_exports_them(lib):
    from ctypes import c_double, c_int, c_int64, c_size_t, c_void_p as VP
    L = lib.lib()
    fns = lib.HEADER.functions
    for name in ("mmr_cluster_rank_workspace_bytes", "mmr_cluster_rank", "mmr_cluster_percentile_trim"):
        assert hasattr(L, name) and name in fns and getattr(L, name).argtypes is not None, name
    assert fns["mmr_cluster_rank_workspace_bytes"][:2] == (c_size_t, [c_int64, c_int, c_int])
    restype, argtypes, names = fns["mmr_cluster_rank"]
    assert restype is c_int and argtypes == [VP, c_int, c_int64, c_int, VP, c_int, VP, c_int, VP, VP, VP, VP, c_size_t, VP]
    assert names == ["gallery", "dtype", "N", "E", "labels", "K", "centers", "metric", "dist", "order", "start", "workspace",
                     "workspace_bytes", "stream"]
    restype, argtypes, names = fns["mmr_cluster_percentile_trim"]
    assert restype is c_int and argtypes == [VP, VP, VP, VP, c_int64, c_int, c_double, VP, VP, VP, VP]
    assert names == ["dist", "order", "start", "labels", "N", "K", "q", "thresholds", "trimmed_labels", "kept", "stream"]
    import mmr_amd
    for name in ("rank_in_clusters", "ClusterRanking", "percentile_trim", "trimmed_centers", "TrimmedCenters", "outlier_filter"):
        assert name in mmr_amd.__all__ and getattr(mmr_amd, name) is getattr(mmr_amd.cluster, name)
    assert callable(mmr_amd.GalleryIndex.trimmed_centers)


# ------------------------------------------------------------------ refusals of the C ABI
def test_rank_argument_validation_happens_before_any_launch(lib):
    L = lib.lib()

    def call(gallery=256, dtype=BF16, N=100, E=512, labels=256, K=3, centers=256, metric=1, dist=256, order=256, start=256,
             ws=256, ws_bytes=1 << 40):
        # pointers are never dereferenced: the checks return first
        return L.mmr_cluster_rank(gallery, dtype, N, E, labels, K, centers, metric, dist, order, start, ws, ws_bytes, 0)

    assert call(dtype=9) == -22 and b"dtype" in L.mmr_last_error()
    assert call(N=-1) == -22 and b"N=-1" in L.mmr_last_error()
    assert call(N=(1 << 31) - 1) == -22 and b"N=" in L.mmr_last_error()
    for E in (100, 64, 1024):
        assert call(E=E) == -95 and f"E={E}".encode() in L.mmr_last_error()
    assert call(K=0) == -22 and b"K=0" in L.mmr_last_error()
    assert call(K=65536) == -22 and b"K=65536" in L.mmr_last_error()
    for metric in (-1, 2):
        assert call(metric=metric) == -22 and b"metric" in L.mmr_last_error()
    for name in ("gallery", "labels", "centers", "dist", "order", "start"):
        assert call(**{name: 0}) == -22 and name.encode() in L.mmr_last_error(), name
    assert call(ws=0) == -22 and b"workspace" in L.mmr_last_error()
    assert call(gallery=264) == -22 and b"16-byte" in L.mmr_last_error() and b"gallery" in L.mmr_last_error()
    assert call(centers=260) == -22 and b"centers" in L.mmr_last_error()
    assert call(dist=260) == -22 and b"8-byte" in L.mmr_last_error() and b"dist" in L.mmr_last_error()
    assert call(start=260) == -22 and b"start" in L.mmr_last_error()
    assert call(labels=258) == -22 and b"labels" in L.mmr_last_error()
    assert call(order=258) == -22 and b"order" in L.mmr_last_error()
    assert call(ws=384) == -22 and b"256-byte" in L.mmr_last_error()
    assert call(ws_bytes=8) == -28 and b"workspace" in L.mmr_last_error()
    need = L.mmr_cluster_rank_workspace_bytes(100, 512, 3)
    assert call(ws_bytes=need - 1) == -28


def test_trim_argument_validation_happens_before_any_launch(lib):
    L = lib.lib()

    def call(dist=256, order=256, start=256, labels=256, N=100, K=3, q=95.0, thresholds=256, trimmed=256, kept=256):
        return L.mmr_cluster_percentile_trim(dist, order, start, labels, N, K, q, thresholds, trimmed, kept, 0)

    assert call(N=-1) == -22 and b"N=-1" in L.mmr_last_error()
    assert call(N=(1 << 31) - 1) == -22
    assert call(K=0) == -22 and b"K=0" in L.mmr_last_error()
    assert call(K=65536) == -22
    for q in (-0.001, 100.001, float("nan"), float("inf")):
        assert call(q=q) == -22 and b"q=" in L.mmr_last_error(), q
    for name in ("dist", "order", "start", "labels", "thresholds", "kept"):
        assert call(**{name: 0}) == -22 and name.encode() in L.mmr_last_error(), name
    assert call(trimmed=0) == -22 and b"trimmed_labels" in L.mmr_last_error()
    for name in ("dist", "start", "thresholds", "kept"):
        assert call(**{name: 260}) == -22 and b"8-byte" in L.mmr_last_error() and name.encode() in L.mmr_last_error(), name
    for name in ("order", "labels"):
        assert call(**{name: 258}) == -22 and b"4-byte" in L.mmr_last_error() and name.encode() in L.mmr_last_error(), name
    assert call(trimmed=258) == -22 and b"trimmed_labels" in L.mmr_last_error()


def test_the_workspace_grows_with_the_rows_and_is_zero_for_refused_arguments(lib):
    L = lib.lib()
    base = L.mmr_cluster_rank_workspace_bytes(10000, 512, 8)
    assert base >= 10000 * 24
    assert L.mmr_cluster_rank_workspace_bytes(20000, 512, 8) >= base + 10000 * 24 - 4096
    assert L.mmr_cluster_rank_workspace_bytes(10000, 512, 8000) > base
    assert L.mmr_cluster_rank_workspace_bytes(10000, 128, 8) == base            # nothing of the gallery's width is stored
    assert L.mmr_cluster_rank_workspace_bytes(0, 512, 8) > 0
    for bad in ((-1, 512, 8), ((1 << 31) - 1, 512, 8), (100, 100, 8), (100, 1024, 8), (100, 512, 0), (100, 512, 65536)):
        assert L.mmr_cluster_rank_workspace_bytes(*bad) == 0, bad


def test_python_argument_errors_raise_before_any_launch():
    """Tensors on the meta device: nothing could be launched even if a check were missing."""
    from mmr_amd import cluster as C

    g = torch.empty(100, 512, dtype=torch.bfloat16, device="meta")
    lab = torch.zeros(100, dtype=torch.int32, device="meta")
    with pytest.raises(RuntimeError, match="GPU"):             # every host check passes: only then the device is asked for
        C.rank_in_clusters(g, lab, 3)
    with pytest.raises(ValueError, match="metric"):
        C.rank_in_clusters(g, lab, 3, metric="manhattan")
    with pytest.raises(ValueError, match="fp32, bf16 or fp16"):
        C.rank_in_clusters(g.to(torch.float64), lab, 3)
    with pytest.raises(ValueError, match="unsupported sizes"):
        C.rank_in_clusters(torch.empty(100, 192, dtype=torch.bfloat16, device="meta"), lab, 3)
    for K in (0, 65536):
        with pytest.raises(ValueError, match="K must be"):
            C.rank_in_clusters(g, lab, K)
    for bad in (lab[:99], lab.float(), lab.bool(), [0] * 100):
        with pytest.raises(ValueError, match="labels"):
            C.rank_in_clusters(g, bad, 3)
    for q in (-1.0, 100.5, float("nan")):
        with pytest.raises(ValueError, match="percentile"):
            C.trimmed_centers(g, lab, 3, percentile=q)
    with pytest.raises(ValueError, match="metric"):
        C.trimmed_centers(g, lab, 3, metric="l1")
    with pytest.raises(RuntimeError, match="GPU"):
        C.trimmed_centers(g, lab, 3)
    rk = C.ClusterRanking(torch.empty(100, dtype=torch.float64, device="meta"), torch.empty(100, dtype=torch.int64, device="meta"),
                          torch.empty(4, dtype=torch.int64, device="meta"), torch.empty(3, 512, device="meta"))
    for q in (-1.0, 101.0, float("nan")):
        with pytest.raises(ValueError, match="q must be"):
            C.percentile_trim(rk, lab, q)
    with pytest.raises(ValueError, match="labels"):
        C.percentile_trim(rk, lab[:5], 95.0)
    with pytest.raises(RuntimeError, match="GPU"):
        C.percentile_trim(rk, lab, 95.0)
    with pytest.raises(ValueError, match="features"):
        C.outlier_filter(torch.empty(0, 128, dtype=torch.float16, device="meta"))
    with pytest.raises(ValueError, match="features"):
        C.outlier_filter(torch.empty(128, dtype=torch.float16, device="meta"))
    with pytest.raises(RuntimeError, match="GPU"):
        C.outlier_filter(torch.empty(10, 128, dtype=torch.float16, device="meta"))
    with pytest.raises(ValueError, match="shots"):
        rk.nearest(0)
    with pytest.raises(IndexError):
        rk.members(3)


# ------------------------------------------------------------------ the restatement rests on the C oracle's dot
@pytest.mark.parametrize("E,K,N", T.PARITY_SHAPES[2:])
def test_fixed_dot_is_the_c_oracles_on_the_fixtures_own_rows(ref, E, K, N):
    """At most 48 finite rows of each fixture, spread over it, against their own fp32 centres, and their norms"""
    for dtype in T.DTYPES:
        f = T.fixture(E, K, N, dtype)
        c32 = f.centers64.astype(np.float32)
        live = np.flatnonzero(T.live_of(f.labels, K) & np.isfinite(f.g32).all(1))
        rows = live[np.unique(np.linspace(0, live.size - 1, 48).astype(np.int64))]
        for k in np.unique(f.labels[rows]):
            rk = rows[f.labels[rows] == k]
            want = np.array([dot64(ref, f.g32[i], c32[k]) for i in rk])
            assert np.array_equal(H.fixed_dot(np.ascontiguousarray(f.g32[rk]), c32[k]).view(np.int64), want.view(np.int64)), (dtype, k)
        want = np.array([dot64(ref, f.g32[i], f.g32[i]) for i in rows])
        assert np.array_equal(H.fixed_norms(np.ascontiguousarray(f.g32[rows])).view(np.int64), want.view(np.int64)), dtype
        want = np.array([dot64(ref, c32[k], c32[k]) for k in range(K)])
        assert np.array_equal(H.fixed_norms(c32).view(np.int64), want.view(np.int64)), dtype


# ------------------------------------------------------------------ the header's formula is numpy's percentile
def header_percentile(seg: np.ndarray, q: float) -> float:
    """include/mmr.h's formula, every step its own fp64 operation, on a SORTED segment"""
    n = seg.shape[0]
    if n == 0 or np.isnan(seg[-1]):
        return float("nan")
    v = np.float64(q / 100.0) * np.float64(n - 1)
    lo = np.floor(v)
    hi = min(int(lo) + 1, n - 1)
    t = v - lo
    a, b = seg[int(lo)], seg[hi]
    with np.errstate(invalid="ignore"):
        diff = b - a
        return float(a + diff * t if t < 0.5 else b - diff * (np.float64(1.0) - t))


def test_the_headers_percentile_formula_is_numpys_bit_for_bit():
    rng = np.random.default_rng(17)
    cases = 0
    for n in (1, 2, 3, 10, 12, 21, 100, 241, 1000, 4099):
        for kind in ("uniform", "ties", "ulp", "inf", "tiny"):
            x = rng.uniform(0.0, 2.0, n)
            if kind == "ties":
                x = np.round(x * 4) / 4
            elif kind == "ulp":
                x = 1.0 + np.arange(n) * 2.0 ** -52
            elif kind == "inf":
                x[rng.integers(0, n, max(1, n // 10))] = np.inf
            elif kind == "tiny":
                x = x * 1e-300
            seg = np.sort(x)
            for q in (0.0, 5.0, 33.3, 50.0, 95.0, 99.9, 100.0):
                with np.errstate(invalid="ignore"):
                    want = np.percentile(seg, q)
                assert T.bits([header_percentile(seg, q)])[0] == T.bits([want])[0], (n, kind, q)
                cases += 1
    assert cases == 350
    assert np.isnan(header_percentile(np.array([0.5, np.nan]), 50.0)) and np.isnan(np.percentile(np.array([0.5, np.nan]), 50.0))
    # sizes 10, 12 and 21 at q = 95: t >= 0.5, t < 0.5 and t == 0
    ts = [0.95 * (n - 1) - np.floor(0.95 * (n - 1)) for n in (10, 12, 21)]
    assert ts[0] >= 0.5 and 0.0 < ts[1] < 0.5 and ts[2] == 0.0


# ------------------------------------------------------------------ the fixtures hold what they claim
def test_the_fixtures_hold_what_they_claim():
    for E, K, N in T.PARITY_SHAPES:
        for dtype in T.DTYPES:
            f = T.fixture(E, K, N, dtype)
            assert f.gallery.dtype == dtype and f.g32.shape == (N, E) and f.labels.shape == (N,)
            if K == 1:
                assert (f.labels == 0).all() and np.isfinite(f.g32).all()
                continue
            sizes = np.bincount(f.labels[T.live_of(f.labels, K)], minlength=K)
            assert sizes[K - 1] == 0 and (sizes[:K - 1] >= 3).all()
            assert sorted(f.labels[list(f.notes["dead"])].tolist()) == [-1, K, K + 5]
            a, b = f.notes["dup"]
            assert np.array_equal(f.g32[a], f.g32[b]) and f.labels[a] == f.labels[b] == 0
            far = list(f.notes["far"])
            assert (f.labels[far] == 0).all() and np.array_equal(f.g32[far[0]], f.g32[far[1]]) and np.array_equal(f.g32[far[0]], f.g32[far[2]])
            assert np.isnan(f.g32[f.notes["nan"]]).any() and np.isinf(f.g32[f.notes["inf"]]).any()
            for metric in T.METRICS:
                r = T.restated(E, K, N, dtype, metric)
                seg = r.order[r.start[0]:r.start[1]]
                assert sorted(seg[-3:].tolist()) == sorted(far), "the three identical rows are cluster 0's farthest"
                assert np.isnan(r.dist[f.notes["nan"]]) and np.isnan(r.thresholds[95.0][f.labels[f.notes["nan"]]])
                assert np.isnan(r.dist[list(f.notes["dead"])]).all() and np.isnan(r.thresholds[95.0][K - 1])
                assert r.order[r.start[K]:].tolist() == sorted(np.flatnonzero(~T.live_of(f.labels, K)).tolist())
                d = r.dist[[a, b]]
                assert d[0] == d[1] and list(r.order).index(a) + 1 == list(r.order).index(b), "ties fall to the lower row id"


# ------------------------------------------------------------------ failing controls
@pytest.mark.parametrize("mut", T.MUTATIONS)
def test_each_planted_mistake_changes_the_result(mut):
    """A mutation that left every shared fixture's result alone would be a mistake the GPU tests cannot see."""
    caught = []
    for E, K, N in T.PARITY_SHAPES[:7]:
        for dtype in T.DTYPES:               # "noclamp" shows on the fp32 fixtures alone (trim_helpers.plant_negative)
            for metric in T.METRICS:
                f = T.fixture(E, K, N, dtype)
                got = T.restate(f.g32, f.labels, K, f.centers64, metric, mut=mut)
                if not T.same(got, T.restated(E, K, N, dtype, metric)):
                    caught.append(T.case_id(E, K, N, dtype, metric))
    print(mut, "caught on", caught)
    assert caught, mut
