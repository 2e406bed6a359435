"""CPU: the host side of nearest-centroid assignment and k-means.  The C ABI's argument validation returns before any
launch (an fp32 gallery among the refusals); the workspace grows with N, K and amb_cap; the Python checks raise before
touching the library; include/mmr.h declares the new symbols and _lib.py binds them; the share of rows the scan's margin
leaves to the exact recheck on the GPU tests' own fixtures is small; and the tests' Lloyd agrees with sklearn's."""
import os

import numpy as np
import pytest
import torch

import assign_helpers as A

NEW_SYMBOLS = ("mmr_assign_workspace_bytes", "mmr_cosine_assign", "mmr_cluster_sums_workspace_bytes", "mmr_cluster_sums")
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


def test_new_symbols_are_exported_declared_and_bound(lib):
    L = lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in lib.HEADER.functions, name
        assert getattr(L, name).argtypes is not None, name
    import mmr_amd
    for name in ("cosine_assign", "kmeans", "cluster_sums", "reference_vector_by_clustering", "KMeansResult"):
        assert name in mmr_amd.__all__ and callable(getattr(mmr_amd, name))


def _assign(L, *, gallery=256, centroids=256, dtype=BF16, N=100, K=4, E=512, bias=0, bound=1.0, mask=0, amb_cap=8, labels=256,
            best=0, counts=256, ws=256, ws_bytes=1 << 40):
    # pointers are never dereferenced: the checks return first
    return L.mmr_cosine_assign(gallery, centroids, dtype, N, K, E, bias, bound, None, mask, amb_cap, labels, best, counts, ws,
                               ws_bytes, 0)


def test_assign_argument_validation_happens_before_any_launch(lib):
    L = lib.lib()
    assert _assign(L, dtype=F32) == -95 and b"fp32 galleries are not supported" in L.mmr_last_error()
    assert _assign(L, dtype=7) == -22 and b"dtype" in L.mmr_last_error()
    assert _assign(L, E=100) == -95 and b"E=100" in L.mmr_last_error()
    assert _assign(L, N=-1) == -22 and b"N=-1" in L.mmr_last_error()
    assert _assign(L, N=1 << 31) == -22
    assert _assign(L, K=0) == -22 and b"K=0" in L.mmr_last_error()
    assert _assign(L, bound=float("inf")) == -22 and b"gallery_norm_bound" in L.mmr_last_error()
    assert _assign(L, amb_cap=0) == -22 and b"amb_cap" in L.mmr_last_error()
    assert _assign(L, centroids=0) == -22 and b"centroids" in L.mmr_last_error()
    assert _assign(L, counts=0) == -22
    assert _assign(L, gallery=0) == -22 and b"gallery" in L.mmr_last_error()
    assert _assign(L, labels=0) == -22
    assert _assign(L, gallery=264) == -22 and b"16-byte" in L.mmr_last_error()
    assert _assign(L, bias=4) == -22 and b"8-byte" in L.mmr_last_error()
    assert _assign(L, labels=258) == -22 and b"labels" in L.mmr_last_error()
    assert _assign(L, mask=2) == -22 and b"row_mask" in L.mmr_last_error()
    assert _assign(L, ws_bytes=8) == -28 and b"workspace" in L.mmr_last_error()


def test_cluster_sums_argument_validation_happens_before_any_launch(lib):
    L = lib.lib()

    def call(gallery=256, dtype=F32, N=100, E=64, labels=256, K=3, sums=256, sizes=256, ws=256, ws_bytes=1 << 40):
        return L.mmr_cluster_sums(gallery, dtype, N, E, labels, K, sums, sizes, ws, ws_bytes, 0)

    assert call(dtype=9) == -22 and b"dtype" in L.mmr_last_error()
    assert call(N=-1) == -22
    assert call(E=0) == -22 and b"E=0" in L.mmr_last_error()
    assert call(K=0) == -22 and b"K=0" in L.mmr_last_error()
    assert call(K=70000) == -22
    assert call(sums=0) == -22 and call(sizes=0) == -22 and call(ws=0) == -22
    assert call(gallery=0) == -22 and call(labels=0) == -22
    assert call(sums=260) == -22 and b"8-byte" in L.mmr_last_error()
    assert call(labels=258) == -22
    assert call(ws_bytes=8) == -28 and b"workspace" in L.mmr_last_error()


def test_workspaces_grow_with_their_arguments(lib):
    L = lib.lib()
    base = L.mmr_assign_workspace_bytes(10000, 512, 64, 1000, BF16)
    assert base > 0
    assert L.mmr_assign_workspace_bytes(20000, 512, 64, 1000, BF16) >= base + 10000 * 112 - 4096       # 112 B per row, less the regions' 256-byte padding
    assert L.mmr_assign_workspace_bytes(10000, 512, 64 + 4096, 1000, BF16) > base
    assert L.mmr_assign_workspace_bytes(10000, 512, 64, 1000 + 4096, BF16) >= base + 4096 * 4
    assert L.mmr_assign_workspace_bytes(10000, 512, 64, 1000, F16) == base
    # K does not multiply the per-row storage: a pass's triples are folded before the next pass
    assert L.mmr_assign_workspace_bytes(10000, 512, 4096, 1000, BF16) < base + (1 << 20)
    for bad in ((10000, 512, 64, 1000, F32), (10000, 100, 64, 1000, BF16), (10000, 512, 0, 1000, BF16),
                (10000, 512, 64, 0, BF16), (-1, 512, 64, 1000, BF16)):
        assert L.mmr_assign_workspace_bytes(*bad) == 0, bad
    s = L.mmr_cluster_sums_workspace_bytes(10000, 512, 8)
    assert s > 0
    assert L.mmr_cluster_sums_workspace_bytes(20000, 512, 8) > s
    assert L.mmr_cluster_sums_workspace_bytes(10000, 512, 800) > s
    assert L.mmr_cluster_sums_workspace_bytes(10000, 512, 0) == 0 and L.mmr_cluster_sums_workspace_bytes(10000, 0, 8) == 0


def test_python_argument_errors_raise_before_any_launch():
    """Tensors on the meta device: nothing could be launched even if a check were missing."""
    from mmr_amd import search, cluster

    g = torch.empty(100, 512, dtype=torch.bfloat16, device="meta")
    with pytest.raises(ValueError, match="fp32 galleries are not supported"):
        search._check_assign_args(torch.empty(100, 512, dtype=torch.float32, device="meta"), torch.empty(4, 512), None)
    with pytest.raises(ValueError):
        search._check_assign_args(g, torch.empty(4, 256), None)
    with pytest.raises(ValueError):
        search._check_assign_args(g, torch.empty(0, 512), None)
    with pytest.raises(ValueError):
        search._check_assign_args(g, torch.empty(4, 512), torch.empty(3))
    with pytest.raises(RuntimeError):
        search.cosine_assign(torch.empty(10, 128, dtype=torch.float16), torch.empty(2, 128))
    with pytest.raises(RuntimeError):
        cluster.kmeans(torch.empty(10, 128, dtype=torch.float16), 2, init="sample")
    with pytest.raises(ValueError):
        cluster.kmeans(g, 2, init="sample", metric="manhattan")
    with pytest.raises(RuntimeError):
        cluster.cluster_sums(torch.empty(10, 128), torch.zeros(10, dtype=torch.int32), 2)


def test_new_centroids_follow_their_definition():
    from mmr_amd import cluster

    sums = torch.tensor([[2.0, 4.0], [0.0, 0.0], [3.0, 4.0]], dtype=torch.float64)
    sizes = torch.tensor([2, 0, 5])
    prev = torch.tensor([[9.0, 9.0], [7.0, 8.0], [1.0, 1.0]], dtype=torch.bfloat16)
    e = cluster.new_centroids(sums, sizes, prev, "euclidean")
    assert e.dtype == torch.bfloat16
    assert e.float().tolist() == [[1.0, 2.0], [7.0, 8.0], torch.tensor([0.6, 0.8]).to(torch.bfloat16).float().tolist()]
    c = cluster.new_centroids(sums, sizes, prev, "cosine")
    want0 = (sums[0] / sums[0].square().sum().sqrt()).to(torch.float32).to(torch.bfloat16)
    assert torch.equal(c[0], want0) and c[1].float().tolist() == [7.0, 8.0]           # an empty cluster keeps its centroid
    assert torch.equal(c[2], torch.tensor([0.6, 0.8]).to(torch.bfloat16))
    b = cluster.centroid_bias(prev, "euclidean")
    assert b.dtype == torch.float64 and b.tolist() == [-81.0, -56.5, -1.0]
    assert cluster.centroid_bias(prev, "cosine") is None


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_the_margin_leaves_few_rows_of_the_gpu_fixtures_ambiguous(dtype):
    """What the GPU test bounds by 3 %, from fp64 scores and the kernel's margin: at most 1.5 % here."""
    for E, K, N in A.PARITY_SHAPES:
        g, c = A.parity_fixture(E, K, N, dtype)
        gf, cf = A.f32(g), A.f32(c)
        for bias in (None, A.euclid_bias(cf)):
            share = A.ambiguous_share(gf, cf, bias)
            print(f"E={E} K={K} N={N} {dtype} bias={'none' if bias is None else 'euclid'}: ambiguous share {share:.4%}")
            assert share <= 0.015, (E, K, N, share)


def test_the_oracle_applies_the_rule(ref):
    """Ties to the lowest centroid, NaN never wins, all-NaN and masked rows get -1."""
    g = A.f32(A.unit_rows(6, 128, 1))
    c = np.ascontiguousarray(np.stack([g[0], g[0], g[1], g[1] * np.float32(2.0)]))
    lab, best, _ = A.oracle_assign(ref, g[:2].copy(), c)
    assert lab.tolist() == [0, 3]
    g2 = g[:3].copy()
    g2[2, 5] = np.nan
    lab, best, _ = A.oracle_assign(ref, g2, c, mask=np.array([True, False, True]))
    assert lab.tolist() == [0, -1, -1] and np.isnan(best[1]) and np.isnan(best[2])
    c2 = c.copy()
    c2[0, 0] = np.nan
    assert A.oracle_assign(ref, g[:1].copy(), c2)[0].tolist() == [1]


def test_the_tests_lloyd_agrees_with_sklearn(ref):
    sk = pytest.importorskip("sklearn.cluster")
    g, _, init = A.planted_clusters(3000, 128, 5, seed=11, dtype=torch.float16)
    _, labels, sizes, n_iter, converged = A.lloyd_reference(ref, g, init, "euclidean", 50)
    assert converged
    km = sk.KMeans(n_clusters=5, init=A.f32(init).astype(np.float64), n_init=1, algorithm="lloyd", tol=0, max_iter=50)
    km.fit(A.f32(g).astype(np.float64))
    assert np.array_equal(km.labels_, labels)
