"""CPU: the silhouette tests' own reference and bound, and the host side of the C calls.

The fp64 restatement (silhouette_helpers.py) is held to sklearn; the bound B the GPU tests assert is shown to see a single
missing pair on every cluster of every fixture those tests use (the failing control); mmr_silhouette_workspace_bytes
refuses what the call refuses and grows with N.  Nothing here launches a kernel."""
import os

import numpy as np
import pytest
import torch

import silhouette_helpers as H


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


@pytest.mark.parametrize("metric", list(H.METRICS))
@pytest.mark.parametrize("dtype", list(H.DTYPES))
def test_the_restatement_is_sklearns(dtype, metric):
    metrics = pytest.importorskip("sklearn.metrics")
    x, lab, K, S, _, sizes = H.case("1200x128x6", dtype, metric)
    live = (lab >= 0) & (lab < K)
    ours = H.samples_rule(S, lab, sizes)
    assert np.isnan(ours[~live]).all() and not np.isnan(ours[live]).any()
    theirs = metrics.silhouette_samples(x.to(torch.float64).numpy()[live], lab[live], metric=metric)
    assert np.abs(ours[live] - theirs).max() <= 1e-9
    assert abs(ours[live].mean() - metrics.silhouette_score(x.to(torch.float64).numpy()[live], lab[live], metric=metric)) <= 1e-9


def test_the_rule_on_hand_made_sums():
    # cluster 0 = {row 0, row 1}, cluster 1 = {row 2}, cluster 2 empty, row 3 not live
    sums = np.array([[2.0, 3.0, 0.0], [2.0, 8.0, 0.0], [5.0, 0.0, 0.0], [1.0, 1.0, 0.0]])
    lab = np.array([0, 0, 1, -1], dtype=np.int32)
    sizes = np.array([2, 1, 0], dtype=np.int64)
    out = H.samples_rule(sums, lab, sizes)
    assert out[0] == (3.0 - 2.0) / 3.0 and out[1] == (8.0 - 2.0) / 8.0 and out[2] == 0.0 and np.isnan(out[3])
    sums[0, 1] = np.nan
    assert np.isnan(H.samples_rule(sums, lab, sizes)[0])
    assert H.samples_rule(np.zeros((2, 2)), np.array([0, 1], dtype=np.int32), np.array([1, 1]))[0] == 0.0
    zero = H.samples_rule(np.zeros((3, 2)), np.array([0, 0, 1], dtype=np.int32), np.array([2, 1]))
    assert zero[0] == 0.0                                  # max(a, b) == 0


@pytest.mark.parametrize("metric", list(H.METRICS))
@pytest.mark.parametrize("dtype", list(H.DTYPES))
@pytest.mark.parametrize("shape", list(H.SHAPES))
def test_failing_control_one_missing_pair_breaks_the_bound(shape, dtype, metric):
    """A kernel that dropped the pair (i, j) would be off by d(i, j) at sums[i, labels[j]].  For every cluster c, with j its
    first row, that is more than B[i, c] for EVERY row i outside c: the bound sees one pair among the cluster's 2100."""
    x, lab, K, S, B, sizes = H.case(shape, dtype, metric)
    x64 = x.to(torch.float64).numpy()
    for c in range(K):
        j = int(np.nonzero(lab == c)[0][0])
        d = H.pair_distances(x64, slice(j, j + 1), metric)[0]           # d(j, i) = d(i, j)
        others = lab != c
        assert others.sum() >= 10
        assert (d[others] > B[others, c]).all(), (c, float((d[others] - B[others, c]).min()))


def test_the_bound_is_small_next_to_the_sums():
    _, lab, K, S, B, sizes = H.case("1200x128x6", "bf16", "euclidean")
    big = S > 0
    assert (B[big] / S[big]).max() < 1e-3 and np.median(B[big] / S[big]) < 3e-4


def test_workspace_bytes_refuses_what_the_call_refuses(lib):
    L = lib.lib()
    kmax = lib.HEADER.constants["MMR_SILHOUETTE_K_MAX"]
    ws = L.mmr_silhouette_workspace_bytes
    assert ws(1000, 128, 0, lib.MMR_BF16) == 0
    assert ws(1000, 128, kmax + 1, lib.MMR_BF16) == 0
    assert ws(1000, 100, 4, lib.MMR_BF16) == 0
    assert ws(1000, 128, 4, lib.MMR_F32) == 0
    assert ws(-1, 128, 4, lib.MMR_BF16) == 0
    assert ws(2 ** 31 - 1, 128, 4, lib.MMR_BF16) == 0
    assert ws(1000, 128, kmax, lib.MMR_F16) > 0


def test_workspace_bytes_grows_with_n(lib):
    ws = lib.lib().mmr_silhouette_workspace_bytes
    got = [ws(n, e, 4, dt) for n in (0, 1, 1000, 100_000, 1_000_000) for e in (128,) for dt in (lib.MMR_BF16,)]
    assert got[0] > 0 and all(a < b for a, b in zip(got[1:], got[2:])) and got[0] <= got[1]
    assert ws(100_000, 512, 4, lib.MMR_BF16) > ws(100_000, 128, 4, lib.MMR_BF16)
    # the sorted copy dominates at small K: 2 E bytes per row, plus the per-row arrays and one chunk's partials per 2048 rows
    assert 100_000 * 512 * 2 < ws(100_000, 512, 4, lib.MMR_F16) < 2 * 100_000 * 512 * 2


def test_the_calls_refuse_on_the_host(lib):
    L = lib.lib()
    kmax = lib.HEADER.constants["MMR_SILHOUETTE_K_MAX"]
    # every one of these returns before any launch, so they are safe without a GPU (dummy aligned non-null pointers)
    assert L.mmr_silhouette_sums(256, lib.MMR_F32, 100, 128, 256, 4, 0, 256, 256, 256, 1 << 30, 0) == -95
    assert b"fp32" in L.mmr_last_error()
    assert L.mmr_silhouette_sums(256, lib.MMR_BF16, 100, 100, 256, 4, 0, 256, 256, 256, 1 << 30, 0) == -95
    assert L.mmr_silhouette_sums(256, lib.MMR_BF16, 100, 128, 256, kmax + 1, 0, 256, 256, 256, 1 << 30, 0) == -22
    assert b"K=" in L.mmr_last_error()
    assert L.mmr_silhouette_sums(256, lib.MMR_BF16, 100, 128, 256, 4, 2, 256, 256, 256, 1 << 30, 0) == -22
    assert b"metric" in L.mmr_last_error()
    assert L.mmr_silhouette_sums(256, lib.MMR_BF16, 100, 128, 256, 4, 0, 256, 256, 256, 16, 0) == -28
    assert b"workspace" in L.mmr_last_error()
    assert L.mmr_silhouette_samples(0, 0, 0, 10, 4, 0, 0) == -22
    assert L.mmr_silhouette_samples(0, 0, 0, 0, 4, 0, 0) == 0          # N == 0: nothing to do


def test_the_constant_arrives_through_the_header(lib):
    from mmr_amd import cluster

    assert lib.HEADER.constants["MMR_SILHOUETTE_K_MAX"] == 1024 == cluster.SILHOUETTE_K_MAX
    for name in ("mmr_silhouette_workspace_bytes", "mmr_silhouette_sums", "mmr_silhouette_samples"):
        assert name in lib.HEADER.functions and hasattr(lib.lib(), name), name


def test_the_selection_rule():
    from mmr_amd import cluster

    assert cluster.best_k_of({2: 0.1, 3: 0.4, 4: 0.3}) == 3
    assert cluster.best_k_of({4: 0.4, 3: 0.4, 2: 0.1}) == 3            # a tie goes to the smallest K
    assert cluster.best_k_of({2: float("nan"), 3: -0.2}) == 3
    with pytest.raises(ValueError):
        cluster.best_k_of({2: float("nan")})
