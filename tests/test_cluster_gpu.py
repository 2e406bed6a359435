"""GPU: per-cluster sums (mmr_cluster_sums), k-means and the reference-vector rule of mmr_amd.cluster against sequential
fp64 sums, a torch-fp64 Lloyd on the CPU written from the documented definition, and a numpy restatement of the
reference's get_cluster_features."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import assign_helpers as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALL_DTYPES = [torch.bfloat16, torch.float16, torch.float32]
ALL_IDS = ["bf16", "fp16", "fp32"]
E_SUMS = 300            # two 256-column slabs, the second one short


@pytest.fixture(scope="module")
def C(device):
    from mmr_amd import cluster
    return cluster


@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


def _labels(N, K, seed):
    """int32 [N] in [-1, K] (both ends are skipped by the call) with label K // 2 removed when K > 1 (an empty cluster)"""
    lab = np.random.default_rng(seed).integers(-1, K + 1, N).astype(np.int32)
    if K > 1:
        lab[lab == K // 2] = -1
    return lab


def _sequential_sums(x64, lab, K):
    sums = np.zeros((K, x64.shape[1]), dtype=np.float64)
    sizes = np.zeros(K, dtype=np.int64)
    for k in range(K):
        rows = x64[lab == k]
        sizes[k] = rows.shape[0]
        if rows.shape[0]:
            sums[k] = np.cumsum(rows, axis=0)[-1]             # row after row, from the first
    return sums, sizes


def _raw_sums(device, g, lab, K, fill):
    from mmr_amd import _lib
    L = _lib.lib()
    N, E = g.shape
    need = L.mmr_cluster_sums_workspace_bytes(N, E, K)
    assert need > 0
    ws = torch.full((need,), fill, dtype=torch.uint8, device=device)
    sums = torch.full((K * E * 8,), fill, dtype=torch.uint8, device=device).view(torch.float64)
    sizes = torch.full((K * 8,), fill, dtype=torch.uint8, device=device).view(torch.int64)
    _lib.check(L.mmr_cluster_sums(g.data_ptr(), _lib.dtype_code(g.dtype), N, E, lab.data_ptr(), K, sums.data_ptr(),
                                  sizes.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr(device)))
    torch.cuda.synchronize(device)
    return sums.view(K, E).cpu().numpy(), sizes.cpu().numpy()


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=ALL_IDS)
@pytest.mark.parametrize("N,K", [(5000, 1), (4099, 7), (4099, 300)])
def test_sums_are_bit_equal_to_a_sequential_sum(C, device, N, K, dtype):
    x = 0.004 * torch.randn(N, E_SUMS, generator=torch.Generator().manual_seed(N + K))
    x = (torch.round(x * 2.0 ** 30) / 2.0 ** 30).to(dtype)   # fp32: multiples of 2^-30
    x = torch.where(x.float().abs() < 2.0 ** -40, torch.zeros_like(x), x)
    lab = _labels(N, K, seed=K)
    x64 = x.to(torch.float64).numpy()
    # the fixture's precondition: under it fp64 addition of these values is exact in any order
    nz = np.abs(x64[x64 != 0])
    assert nz.min() >= 2.0 ** -40
    if dtype == torch.float32:
        assert np.array_equal(x64 * 2.0 ** 30, np.round(x64 * 2.0 ** 30))
    assert max(np.abs(x64[lab == k]).sum(0).max() for k in range(K) if (lab == k).any()) < 32
    want_sums, want_sizes = _sequential_sums(x64, lab, K)
    assert (want_sizes == 0).any() or K == 1
    sums, sizes = C.cluster_sums(x.to(device), torch.from_numpy(lab).to(device), K)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (K, E_SUMS) and sizes.dtype == torch.int64
    assert np.array_equal(sizes.cpu().numpy(), want_sizes)
    assert np.array_equal(sums.cpu().numpy().view(np.int64), want_sums.view(np.int64)), "sums differ from the sequential fp64 sum"


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=ALL_IDS)
def test_sums_with_every_label_out_of_range(C, device, dtype):
    """K = 1 and no label in [0, K): every grouping key is K itself, so the sort has one key bit, start = [N, N] and the
    one cluster is empty.  N = 257: a second, one-row block of keys."""
    N, E, K = 257, 128, 1
    x = torch.randn(N, E, generator=torch.Generator().manual_seed(N)).to(dtype)
    lab = np.array([-1, 1, 5, np.iinfo(np.int32).min, np.iinfo(np.int32).max], dtype=np.int32)[np.arange(N) % 5]
    want_sums, want_sizes = _sequential_sums(x.to(torch.float64).numpy(), lab, K)
    assert want_sizes.tolist() == [0] and not want_sums.any()
    sums, sizes = C.cluster_sums(x.to(device), torch.from_numpy(lab).to(device), K)
    assert np.array_equal(sizes.cpu().numpy(), want_sizes)
    assert np.array_equal(sums.cpu().numpy().view(np.int64), want_sums.view(np.int64))


def test_general_fp32_sums_are_close_and_reproducible(device):
    N, K = 4099, 7
    x = torch.randn(N, E_SUMS, generator=torch.Generator().manual_seed(9))
    lab = _labels(N, K, seed=3)
    x64 = x.to(torch.float64).numpy()
    want_sums, want_sizes = _sequential_sums(x64, lab, K)
    xd, ld = x.to(device), torch.from_numpy(lab).to(device)
    s1, n1 = _raw_sums(device, xd, ld, K, 0xFF)
    s2, n2 = _raw_sums(device, xd, ld, K, 0x00)
    assert np.array_equal(s1.view(np.int64), s2.view(np.int64)) and np.array_equal(n1, n2)     # whatever the workspace held
    assert np.array_equal(n1, want_sizes)
    for k in range(K):
        bound = max(want_sizes[k], 1) * 2.0 ** -52 * np.abs(x64[lab == k]).sum(0)
        assert (np.abs(s1[k] - want_sums[k]) <= bound).all(), k


# ------------------------------------------------------------------ k-means
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_kmeans_matches_a_lloyd_written_from_the_definition(C, ref, device, dtype, metric):
    N, E, K = 3000, 128, 5
    g, truth, init = A.planted_clusters(N, E, K, seed=11, dtype=dtype)
    assert A.sum_is_exact(A.f32(g), 2.0 ** -40)             # the CPU's index_add_ and the library's ordered sums agree
    want_c, want_labels, want_sizes, want_iter, want_conv = A.lloyd_reference(ref, g, init, metric, 50)
    assert want_conv and want_iter >= 6                      # several centroid updates, not a one-step fixture
    res = C.kmeans(g.to(device), K, init=init, metric=metric, max_iter=50)
    assert res.converged and res.n_iter == want_iter
    assert np.array_equal(res.labels.cpu().numpy(), want_labels)
    assert np.array_equal(res.sizes.cpu().numpy(), want_sizes)
    assert res.centroids.dtype == dtype and torch.equal(res.centroids.cpu(), want_c)
    # the inertia is that of the returned assignment
    g64, c64 = g.to(torch.float64), want_c.to(torch.float64)[want_labels.astype(np.int64)]
    inertia = float((g64 - c64).square().sum()) if metric == "euclidean" else float(N - (g64 * c64).sum())
    assert abs(res.inertia - inertia) <= 1e-9 * max(1.0, abs(inertia))
    # max_iter bounds the run
    short = C.kmeans(g.to(device), K, init=init, metric=metric, max_iter=2)
    assert short.n_iter == 2 and not short.converged


def test_kmeans_sample_init_is_reproducible(C, device):
    N, E, K = 3000, 128, 5
    g, _, _ = A.planted_clusters(N, E, K, seed=11, dtype=torch.float16)
    gd = g.to(device)
    keep = torch.ones(N, dtype=torch.bool)
    keep[::3] = False
    runs = [C.kmeans(gd, K, init="sample", generator=torch.Generator().manual_seed(8), row_mask=keep.to(device), max_iter=30)
            for _ in range(2)]
    assert torch.equal(runs[0].labels, runs[1].labels) and torch.equal(runs[0].centroids, runs[1].centroids)
    assert runs[0].n_iter == runs[1].n_iter and runs[0].inertia == runs[1].inertia
    lab = runs[0].labels.cpu()
    assert (lab[~keep] == -1).all() and (lab[keep] >= 0).all() and int(runs[0].sizes.sum()) == int(keep.sum())
    other = C.kmeans(gd, K, init="sample", generator=torch.Generator().manual_seed(9), row_mask=keep.to(device), max_iter=1)
    first = C.kmeans(gd, K, init="sample", generator=torch.Generator().manual_seed(8), row_mask=keep.to(device), max_iter=1)
    assert not torch.equal(other.centroids, first.centroids)
    # the sampled centroids are K distinct live rows
    live_rows = {tuple(r.tolist()) for r in g[keep].view(torch.int16)}
    picked = [tuple(r.tolist()) for r in first.centroids.cpu().view(torch.int16)]
    assert len(set(picked)) == K and all(p in live_rows for p in picked)


def test_an_empty_cluster_keeps_its_centroid(C, device):
    N, E, K = 3000, 128, 5
    g, _, init = A.planted_clusters(N, E, K, seed=11, dtype=torch.bfloat16)
    far = (-100.0 * g[:100].float().mean(0, keepdim=True)).to(torch.bfloat16)          # farther from every row than any init row
    init6 = torch.cat([init, far])
    for metric in ("euclidean",):
        res = C.kmeans(g.to(device), K + 1, init=init6, metric=metric, max_iter=50)
        assert int(res.sizes[K]) == 0 and torch.equal(res.centroids[K].cpu(), far[0])
        base = C.kmeans(g.to(device), K, init=init, metric=metric, max_iter=50)
        assert torch.equal(res.labels, base.labels) and torch.equal(res.centroids[:K], base.centroids)


# ------------------------------------------------------------------ the reference's rule
def _numpy_rule(f, labels, shots):
    """code/search_image.py:203-231 restated: f fp64 [n, E], labels in {0, 1}"""
    centres = np.stack([f[labels == k].mean(0) for k in (0, 1)])
    n0, n1 = int((labels == 0).sum()), int((labels == 1).sum())
    if abs(n0 - n1) / len(labels) < 0.2:
        d = np.linalg.norm(f - centres.mean(axis=0), axis=1)
        idx = np.argsort(d, kind="stable")[:shots]
    else:
        major = 0 if n0 >= n1 else 1
        rows = np.where(labels == major)[0]
        d = np.linalg.norm(f[rows] - centres[major], axis=1)
        idx = rows[np.argsort(d, kind="stable")[:shots]]
    return f[idx].mean(axis=0), idx


@pytest.mark.parametrize("n_major", [20, 30], ids=["balanced", "majority"])
def test_reference_vector_by_clustering(C, device, n_major):
    n, E, shots = 40, 128, 5
    gen = torch.Generator().manual_seed(n_major)
    centres = A.unit_rows(2, E, 77)
    member = torch.cat([torch.zeros(n_major, dtype=torch.long), torch.ones(n - n_major, dtype=torch.long)])
    member = member[torch.randperm(n, generator=gen)]
    f = centres[member] + 0.4 * torch.randn(n, E, generator=gen) / E ** 0.5
    f = (f / f.norm(dim=-1, keepdim=True)).to(torch.float16)           # the reference keeps fp16 features
    init = torch.stack([f[int(torch.nonzero(member == 0)[0])], f[int(torch.nonzero(member == 1)[0])]])
    fd = f.to(device)
    labels = C.kmeans(fd, 2, init=init).labels.cpu().numpy()
    assert np.array_equal(labels, member.numpy())
    want_vec, want_idx = _numpy_rule(f.to(torch.float64).numpy(), labels, shots)
    vec, idx = C.reference_vector_by_clustering(fd, shots, init=init, return_indices=True)
    assert vec.dtype == torch.float32 and tuple(vec.shape) == (E,)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.allclose(vec.cpu().numpy(), want_vec, rtol=1e-6, atol=1e-9)
    assert abs(float(vec.norm()) - 1.0) > 1e-3               # a mean of unit rows, not re-normalised
    again = C.reference_vector_by_clustering(fd, shots, init=init)
    assert torch.equal(again, vec)


def test_cluster_gallery_example():
    spec = importlib.util.spec_from_file_location("cluster_gallery_synthetic", os.path.join(ROOT, "examples", "cluster_gallery_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--rows", "20000", "--classes", "6", "--dim", "128"])
    assert out["purity"] > 0.5 and int(out["sizes"].sum()) == 20000     # sampled seeds may share a class: no more is promised
    assert out["clean_shots"] == out["shots"] == 10          # the majority cluster holds the class's own samples
    assert out["hits"] >= 45
