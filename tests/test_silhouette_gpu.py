"""GPU: silhouette sums, samples and score (mmr_silhouette_sums / mmr_silhouette_samples, mmr_amd.cluster) against the fp64
restatement of the definition and the error bound of include/mmr.h (silhouette_helpers.py: S64 and B), plus select_k.

The bound B[i, c] is asserted elementwise; test_silhouette_host.py shows that it sees a single missing pair on these very
fixtures.  An exact-arithmetic fixture separates the bookkeeping (which pairs, which cluster, masking, padding) from the
arithmetic."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import silhouette_helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DT = list(H.DTYPES)
MT = list(H.METRICS)


@pytest.fixture(scope="module")
def C(device):
    from mmr_amd import cluster
    return cluster


def _raw(device, g, lab, K, metric, fill_ws, fill_out=0xFF, ws_bytes=None):
    """The C call with the workspace and the outputs prefilled: -> (rc, sums [N, K] numpy, sizes [K] numpy)"""
    from mmr_amd import _lib
    L = _lib.lib()
    N, E = g.shape
    need = L.mmr_silhouette_workspace_bytes(N, E, K, _lib.dtype_code(g.dtype))
    assert need > 0
    have = need if ws_bytes is None else ws_bytes
    ws = torch.full((max(have, 256),), fill_ws, dtype=torch.uint8, device=device)
    sums = torch.full((N * K * 8,), fill_out, dtype=torch.uint8, device=device).view(torch.float64)
    sizes = torch.full((K * 8,), fill_out, dtype=torch.uint8, device=device).view(torch.int64)
    rc = L.mmr_silhouette_sums(g.data_ptr(), _lib.dtype_code(g.dtype), N, E, lab.data_ptr(), K, H.METRICS[metric], sums.data_ptr(),
                               sizes.data_ptr(), ws.data_ptr(), have, _lib.stream_ptr(device))
    torch.cuda.synchronize(device)
    return rc, sums.view(N, K).cpu().numpy(), sizes.cpu().numpy()


def _dev(device, x, lab):
    return x.to(device), torch.from_numpy(lab).to(device)


# ------------------------------------------------------------------ 1. sums within the bound

@pytest.mark.parametrize("metric", MT)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", list(H.SHAPES))
def test_sums_are_within_the_bound(device, shape, dtype, metric):
    x, lab, K, S, B, sizes = H.case(shape, dtype, metric)
    g, l = _dev(device, x, lab)
    rc, sums, got_sizes = _raw(device, g, l, K, metric, fill_ws=0xFF)
    assert rc == 0
    assert np.array_equal(got_sizes, sizes)
    assert not np.isnan(sums).any()                        # every element written over the 0xFF prefill (a NaN pattern)
    err = np.abs(sums - S)
    live = (lab >= 0) & (lab < K)
    assert (~live).sum() == 8
    print(f"{shape} {dtype} {metric}: largest error / bound {np.max(err[B > 0] / B[B > 0]):.4f}, "
          f"median bound / sum {np.median(B[S > 0] / S[S > 0]):.2e}")
    assert (err <= B).all(), (np.argwhere(err > B)[:5], err[err > B][:5], B[err > B][:5])
    assert (err[~live] <= B[~live]).all()                  # rows that are not live get their sums too


# ------------------------------------------------------------------ 2. self pair and singletons

@pytest.mark.parametrize("metric", MT)
@pytest.mark.parametrize("dtype", DT)
def test_self_pair_and_singletons(C, device, dtype, metric):
    x, lab, K, S, B, sizes = H.case("1200x128x6", dtype, metric)
    g, l = _dev(device, x, lab)
    sums, got_sizes = C.silhouette_sums(g, l, K, metric)
    samples = C.silhouette_samples(g, l, K, metric).cpu().numpy()
    sums = sums.cpu().numpy()
    assert sizes[0] == 1 and sizes[1] == 2
    i = int(np.nonzero(lab == 0)[0][0])
    assert sums[i, 0] == 0.0 and samples[i] == 0.0
    a, b = (int(r) for r in np.nonzero(lab == 1)[0])
    x64 = x.to(torch.float64).numpy()
    d = H.pair_distances(x64, slice(a, a + 1), metric)[0]
    delta = H.pair_delta(x64, slice(a, a + 1), d[None, :], metric)[0]
    assert d[b] > 0.1
    assert abs(sums[a, 1] - d[b]) <= delta[b] and abs(sums[b, 1] - d[b]) <= delta[b]


# ------------------------------------------------------------------ 3. exact arithmetic

@pytest.mark.parametrize("dtype", DT)
def test_exact_arithmetic_fixture(C, device, dtype):
    """Rows 44 e_p, 117 e_q, 240 e_r on three disjoint coordinate ranges, one coordinate per cluster: every dot, norm and
    d^2 is exact in fp32, cross distances are exactly 125, 244 and 267, within-cluster ones exactly 0."""
    E, n = 128, (31, 257, 300)
    val, coord = (44.0, 117.0, 240.0), (3, 50, 101)
    dist = {(0, 1): 125.0, (0, 2): 244.0, (1, 2): 267.0}
    lab = np.repeat(np.arange(3, dtype=np.int32), n)
    lab = lab[np.random.default_rng(5).permutation(lab.size)]
    x = torch.zeros(lab.size, E)
    for c in range(3):
        x[torch.from_numpy(lab == c), coord[c]] = val[c]
    x = x.to(H.DTYPES[dtype])
    assert torch.equal(x.float().square().sum(1).sqrt(), torch.tensor(val)[torch.from_numpy(lab.astype(np.int64))])
    g, l = _dev(device, x, lab)
    sums, sizes = C.silhouette_sums(g, l, 3, "euclidean")
    sums, sizes = sums.cpu().numpy(), sizes.cpu().numpy()
    assert sizes.tolist() == list(n)
    rel = 2.0 ** -22 + 1.001 * 2.0 ** -13
    for i in range(lab.size):
        own = int(lab[i])
        assert sums[i, own] == 0.0, i
        for c in range(3):
            if c != own:
                want = dist[(min(own, c), max(own, c))] * n[c]
                assert abs(sums[i, c] - want) <= rel * want, (i, c, sums[i, c], want)
    samples = C.silhouette_samples(g, l, 3).cpu().numpy()
    assert np.abs(samples - 1.0).max() <= 1e-3


# ------------------------------------------------------------------ 4. samples are the rule

@pytest.mark.parametrize("metric", MT)
def test_samples_are_the_rule_on_the_returned_sums(C, device, metric):
    x, lab, K, S, B, sizes = H.case("1200x128x6", "bf16", metric)
    g, l = _dev(device, x, lab)
    sums, got_sizes = C.silhouette_sums(g, l, K, metric)
    samples = C.silhouette_samples(g, l, K, metric).cpu().numpy()
    want = H.samples_rule(sums.cpu().numpy(), lab, got_sizes.cpu().numpy())
    live = (lab >= 0) & (lab < K)
    assert np.isnan(samples[~live]).all() and not np.isnan(samples[live]).any()
    assert np.array_equal(samples[live].view(np.int64), want[live].view(np.int64))
    assert np.isnan(want[~live]).all()
    score = C.silhouette_score(g, l, K, metric)
    assert abs(score - want[live].mean()) <= lab.size * 2.0 ** -52
    # K = None: labels.max() + 1, here one more than K (the row relabelled K), a cluster of its own
    auto = C.silhouette_samples(g, l, None, metric).cpu().numpy()
    assert auto.shape == (lab.size,) and auto[lab == K][0] == 0.0


# ------------------------------------------------------------------ 5. against the fp64 definition end to end

@pytest.mark.parametrize("metric", MT)
@pytest.mark.parametrize("dtype", DT)
def test_samples_and_score_against_the_definition(C, device, dtype, metric):
    """With relative errors of at most eps = max_c B[i, c] / S64[i, c] on a and on b (a minimum of perturbed means is within
    eps of the true minimum), f(a, b) = (b - a) / max(a, b) = +-(1 - min / max) moves by at most
    (1 + eps) / (1 - eps) - 1 <= 2 eps / (1 - eps) < 4 eps, also where the larger of the two changes sides (f is continuous)."""
    N, E, K, forced = H.SHAPES["1200x128x6"]
    x, lab = H.make_fixture(N, E, K, H.DTYPES[dtype], forced, seed=N + E + K)
    x, lab = H.without_duplicates(x, lab)
    assert x.shape[0] == N - 4
    S, B, sizes = H.sums_and_bound(x, lab, K, metric)
    live = (lab >= 0) & (lab < K)
    used = (sizes > 0)[None, :] & (S > 0)
    eps = np.where(used, B / np.where(S > 0, S, 1.0), 0.0).max(1)
    assert eps.max() <= 5e-4
    want = H.samples_rule(S, lab, sizes)
    g, l = _dev(device, x, lab)
    got = C.silhouette_samples(g, l, K, metric).cpu().numpy()
    assert np.isnan(got[~live]).all()
    err = np.abs(got[live] - want[live])
    print(f"{dtype} {metric}: largest sample error {err.max():.2e}, allowance {4 * eps[live].max():.2e}")
    assert (err <= 4 * eps[live]).all()
    assert abs(C.silhouette_score(g, l, K, metric) - want[live].mean()) <= (4 * eps[live]).mean()


# ------------------------------------------------------------------ 6. reproducible

@pytest.mark.parametrize("metric", MT)
def test_two_runs_agree_bit_for_bit_whatever_the_workspace_held(device, metric):
    x, lab, K, _, _, _ = H.case("3000x128x2", "fp16", metric)
    g, l = _dev(device, x, lab)
    rc1, s1, n1 = _raw(device, g, l, K, metric, fill_ws=0xFF, fill_out=0xFF)
    rc2, s2, n2 = _raw(device, g, l, K, metric, fill_ws=0x00, fill_out=0x00)
    assert rc1 == 0 and rc2 == 0
    assert np.array_equal(s1.view(np.int64), s2.view(np.int64)) and np.array_equal(n1, n2)


# ------------------------------------------------------------------ 7. a non-finite row

@pytest.mark.parametrize("metric", MT)
@pytest.mark.parametrize("dtype", DT)
def test_a_non_finite_row_stays_in_its_cluster_and_its_row(C, device, dtype, metric):
    N, E, K, forced = H.SHAPES["700x512x3"]
    x, lab = H.make_fixture(N, E, K, H.DTYPES[dtype], forced, seed=11)
    r = int(np.nonzero(lab == 2)[0][3])
    x[r, 17] = float("inf")
    S, B, sizes = H.sums_and_bound(x, lab, K, metric)
    g, l = _dev(device, x, lab)
    sums, got_sizes = C.silhouette_sums(g, l, K, metric)               # no error is raised
    sums = sums.cpu().numpy()
    assert np.array_equal(got_sizes.cpu().numpy(), sizes)
    rows = np.arange(N) != r
    for c in (0, 1):
        assert (np.abs(sums[rows, c] - S[rows, c]) <= B[rows, c]).all(), c
    assert not np.isfinite(sums[rows, 2]).any()
    assert not np.isfinite(sums[r, :]).any()


# ------------------------------------------------------------------ 8. errors

def test_errors(C, device):
    from mmr_amd import _lib
    x, lab, K, _, _, _ = H.case("1200x128x6", "bf16", "euclidean")
    g, l = _dev(device, x, lab)
    with pytest.raises(ValueError, match="bf16 or fp16"):
        C.silhouette_sums(g.float(), l, K)
    with pytest.raises(ValueError, match="bf16 or fp16"):
        C.silhouette_score(g.float(), l, K)
    with pytest.raises(ValueError, match="K must be"):
        C.silhouette_sums(g, l, C.SILHOUETTE_K_MAX + 1)
    with pytest.raises(ValueError, match="K must be"):
        C.silhouette_samples(g, l, 0)
    with pytest.raises(ValueError, match="labels"):
        C.silhouette_sums(g, l[:-1], K)
    with pytest.raises(ValueError, match="labels"):
        C.silhouette_sums(g, l.float(), K)
    with pytest.raises(ValueError, match="metric"):
        C.silhouette_sums(g, l, K, metric="manhattan")
    with pytest.raises(ValueError, match="silhouette"):
        C.silhouette_sums(g[:, :100], l, K)
    with pytest.raises(RuntimeError):
        C.silhouette_sums(g.cpu(), l, K)
    with pytest.raises(ValueError, match="non-empty clusters"):
        C.silhouette_score(g, torch.zeros_like(l), K)
    with pytest.raises(ValueError, match="non-empty clusters"):
        C.silhouette_score(g[:5], torch.arange(5, device=device), 5)   # every row its own cluster
    # a too-small workspace: MMR_ENOSPC, as mmr_cluster_sums and mmr_cosine_assign answer
    rc, _, _ = _raw(device, g, l, K, "euclidean", fill_ws=0, ws_bytes=4096)
    assert rc == _lib.HEADER.constants["MMR_ENOSPC"] and b"workspace" in _lib.lib().mmr_last_error()


# ------------------------------------------------------------------ 9. select_k

def test_select_k_finds_the_planted_k(C, device):
    N, E = 1500, 128
    rng = np.random.default_rng(3)
    centres = rng.standard_normal((3, E))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = 3.0 * centres[rng.integers(0, 3, N)] + rng.standard_normal((N, E)) / np.sqrt(E)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    g = torch.from_numpy(x).to(torch.float32).to(torch.bfloat16).to(device)
    res = C.select_k(g, (2, 3, 4), generator=torch.Generator().manual_seed(7))
    assert res.best_k == 3 and sorted(res.scores) == [2, 3, 4] and sorted(res.results) == [2, 3, 4]
    assert res.scores[3] > 0.5
    for k in (2, 3, 4):
        assert res.scores[k] == C.silhouette_score(g, res.results[k].labels, k)
    assert C.best_k_of({2: 0.25, 3: 0.5, 4: 0.5}) == 3                 # a tie goes to the smallest K
    assert C.best_k_of({4: 0.5, 2: 0.5}) == 2
    with pytest.raises(ValueError):
        C.select_k(g, (1, 2))


# ------------------------------------------------------------------ 10. the example

def test_select_k_example(device, capsys):
    spec = importlib.util.spec_from_file_location("select_k_synthetic", os.path.join(ROOT, "examples", "select_k_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--rows", "3000", "--clusters", "3"])
    out = capsys.readouterr().out
    assert "chosen K = 3" in out
