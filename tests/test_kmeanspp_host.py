"""CPU: the k-means++ seeding's restatement (tests/kmeanspp_helpers.py) is sklearn's algorithm, obeys the definition's
boundary rules, and tells every planted mistake apart on the GPU tests' own cases; the host helpers, the argument errors
that need no device and the header's declarations.  Nothing here launches a kernel."""
import math

import numpy as np
import pytest
import torch

import assign_helpers as A
import kmeanspp_helpers as H
from search_helpers import dot64


@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


@pytest.fixture(scope="module")
def C():
    from mmr_amd import cluster
    return cluster


# ------------------------------------------------------------------ the vectorised fixed-order dot is the C oracle's
@pytest.mark.parametrize("E", [128, 256, 512, 768])
def test_fixed_dot_is_the_c_oracles_bit_for_bit(ref, E):
    rng = np.random.default_rng(E)
    g = (rng.standard_normal((96, E)) * np.exp(rng.uniform(-6, 6, (96, 1)))).astype(np.float32)
    g = A.f32(torch.from_numpy(g).to(torch.bfloat16 if E % 256 else torch.float16))
    for c in (0, 17, 95):
        want = np.array([dot64(ref, g[i], g[c]) for i in range(96)])
        assert np.array_equal(H.fixed_dot(g, g[c]).view(np.int64), want.view(np.int64))
    want = np.array([dot64(ref, g[i], g[i]) for i in range(96)])
    assert np.array_equal(H.fixed_norms(g).view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("E,K,N", H.PARITY_SHAPES[1:])
def test_fixed_dot_is_the_c_oracles_on_the_gpu_fixtures_own_rows(ref, E, K, N):
    """The rows the GPU parity tests run on, both dtypes: every row against three centres (the first, the last and one
    between), and every norm -- at most 64 rows of each fixture, spread over it"""
    for dtype in (torch.bfloat16, torch.float16):
        g = A.f32(H.planted(N, E, K, dtype))
        rows = np.unique(np.linspace(0, N - 1, 64).astype(np.int64))
        sub = np.ascontiguousarray(g[rows])
        for c in (0, N // 2, N - 1):
            want = np.array([dot64(ref, g[i], g[c]) for i in rows])
            assert np.array_equal(H.fixed_dot(sub, g[c]).view(np.int64), want.view(np.int64)), (dtype, c)
        want = np.array([dot64(ref, g[i], g[i]) for i in rows])
        assert np.array_equal(H.fixed_norms(sub).view(np.int64), want.view(np.int64)), dtype


# ------------------------------------------------------------------ the restatement is sklearn's algorithm
@pytest.mark.parametrize("N,E,K", [(4099, 128, 8), (2051, 256, 33)])
def test_the_restatement_is_sklearns_greedy_kmeans_plusplus(N, E, K):
    """The mean final potential over 200 variate draws against the mean over 200 random_states of
    sklearn.cluster.kmeans_plusplus, on planted fixtures: within 4 standard errors of the difference.  Measured with the
    project's fixture (assign_helpers.planted_clusters, 8 clusters, bf16): (4099, 128, 8) -0.49 standard errors,
    (2051, 256, 33) -0.66; uniform sampling of the seeds sits +1.8 % / +2.1 % higher, 27 and 51 standard errors away, so
    the check tells D^2 sampling from none.  All 200 restated runs had distinct seeds."""
    skc = pytest.importorskip("sklearn.cluster")
    g = A.f32(H.planted(N, E, K, torch.bfloat16))
    X = g.astype(np.float64)
    gram = X @ X.T
    n2 = (X * X).sum(1)
    G = H.host_norm_bound(g)
    L = H.trials(K)
    shift, _ = H.scale_of(G, "euclidean")

    def potential(idx):
        d = n2[:, None] + n2[idx][None, :] - 2.0 * gram[:, idx]
        return float(np.maximum(d, 0.0).min(1).sum())

    ours, theirs, uniform = [], [], []
    rng = np.random.default_rng(5)
    for i in range(200):
        r = H.restate(g, K, L, H.variates_of(K, L, 31000 + i), G, "euclidean", dots="blas", gram=gram)
        assert len(set(r.indices.tolist())) == K
        ours.append(math.ldexp(int(r.potentials[-1]), -shift))
        _, idx = skc.kmeans_plusplus(X, K, random_state=i)
        theirs.append(potential(idx))
        uniform.append(potential(rng.choice(N, K, replace=False)))
    ours, theirs, uniform = np.array(ours), np.array(theirs), np.array(uniform)
    se = math.sqrt(ours.var(ddof=1) / 200 + theirs.var(ddof=1) / 200)
    z = (ours.mean() - theirs.mean()) / se
    zu = (uniform.mean() - theirs.mean()) / math.sqrt(uniform.var(ddof=1) / 200 + theirs.var(ddof=1) / 200)
    print(f"N={N} E={E} K={K}: restated {ours.mean():.4f}, sklearn {theirs.mean():.4f}, z = {z:+.2f}; "
          f"uniform {uniform.mean():.4f} ({uniform.mean() / theirs.mean() - 1:+.2%}), z = {zu:+.1f}")
    # the integer potential is the fp64 one up to truncation: at most N weight units low
    assert abs(ours[-1] - potential(r.indices)) <= N * math.ldexp(1.0, -shift) + 1e-9 * ours[-1]
    assert abs(z) <= 4.0, (ours.mean(), theirs.mean(), se)


# ------------------------------------------------------------------ the boundary rules, on hand-made weight vectors
W = np.array([0, 0, 5, 0, 3, 0, 0, 8, 0], dtype=np.int64)          # T = 16, prefix sums 0 0 5 5 8 8 8 16 16


def test_sampling_boundaries():
    T = 16
    assert H.sample(W, 0, 1) == 2                                    # b = 0 skips the leading zero weights
    assert H.sample(W, 2 ** 53 - 1, 1) == 7                          # r = T - 1: the last positive row, not the zeros behind it
    assert ((2 ** 53 - 1) * T) >> 53 == T - 1
    assert H.sample(W, H.variate_for(5, T), 1) == 4                  # r equal to a prefix sum: the next positive row
    assert H.sample(W, H.variate_for(4, T), 1) == 2                  # one below it: still that row
    assert H.sample(W, H.variate_for(8, T), 1) == 7 and H.sample(W, H.variate_for(7, T), 1) == 4
    assert H.sample(np.zeros(9, dtype=np.int64), 12345, 3) == 3      # T == 0: the lowest live row
    assert H.sample(W, 0, 1, mut="ge") == 0 and H.sample(W, H.variate_for(5, T), 1, mut="ge") == 2
    # r from a 128-bit product: b T is past 2^64 here
    big = np.array([2 ** 38 - 1] * 4, dtype=np.int64)
    b = 2 ** 53 - 12345
    assert H.sample(big, b, 0) == ((b * int(big.sum())) >> 53) // (2 ** 38 - 1)


def test_ties_between_trials_and_the_weight_rule():
    assert H.pick([7, 3, 9, 3]) == 1 and H.pick([7, 3, 9, 3], "tie_high") == 3 and H.pick([7, 3, 9, 3], "argmax") == 2
    assert H.pick([4, 4, 4]) == 0 and H.pick([4, 4, 4], "argmax") == 0
    d = np.array([-1.0, 0.0, np.nan, 0.75, 1.0, 3.999, 1e30, np.inf])
    assert H.weights_from(d, 2).tolist() == [0, 0, 0, 3, 4, 15, H.WMAX, H.WMAX]
    assert H.weights_from(d, 2, "round").tolist()[3:6] == [3, 4, 16]
    assert H.scale_of(1.0, "euclidean") == (35, 4.0) and H.scale_of(1.0, "cosine") == (36, 2.0)
    assert H.scale_of(0.0, "euclidean") == (0, 0.0) and H.scale_of(0.0, "cosine") == (37, 1.0)
    assert H.scale_of(30.0, "euclidean")[0] == 37 - 11                # 3600 = 2^11.8


# ------------------------------------------------------------------ failing controls
@pytest.fixture(scope="module")
def controls():
    out = []
    for case in H.control_cases():
        G = H.host_norm_bound(case.g32)
        if case.variates is None:
            var, base = case.craft(case, G)
        else:
            var, base = case.variates, H.restate(case.g32, case.K, case.L, case.variates, G, case.metric, case.mask)
        out.append((case, G, var, base))
    return out


def test_the_control_cases_are_what_they_claim(controls):
    by = {c.name.split("-")[0]: (c, base) for c, _, _, base in controls}
    by.update({"-".join(c.name.split("-")[:3]): (c, base) for c, _, _, base in controls})
    dup, base = by["duplicates"]
    assert len(set(base.indices[:3].tolist())) == 3 and sorted(i % 3 for i in base.indices[:3]) == [0, 1, 2]
    assert base.indices[3:].tolist() == [0, 0] and base.potentials[2:].tolist() == [0, 0, 0]
    crafted, base = by["crafted"]
    B = H.BLOCK_ROWS
    # the first live row past block 0: rows B - 6 .. B + 13 are masked
    assert len(set(base.indices.tolist())) == crafted.K and base.indices[0] == B + 14
    assert all(set(c[2:4]) <= set(range(B - 6)) | set(range(B + 14, 700)) for c in base.cands[1:])
    # the block edges: every trial draws exactly the last row of a block or the first row of the next
    one, base = by["edges-E128-K5"]
    assert base.cands == [[2 * B + 187], [B - 1], [B], [2 * B - 1], [2 * B]] and base.indices.tolist() == [2 * B + 187, B - 1, B, 2 * B - 1, 2 * B]
    two, base = by["edges-E128-K3"]
    assert base.cands == [[2 * B + 187], [B - 1, B], [2 * B - 1, 2 * B]]
    assert base.indices[1] in (B - 1, B) and base.indices[2] in (2 * B - 1, 2 * B)


@pytest.mark.parametrize("mut", H.MUTATIONS)
def test_each_planted_mistake_changes_the_result(controls, mut):
    """A mutation that left indices and potentials alone on every shared case would be a mistake the GPU tests cannot see."""
    caught = []
    for case, G, var, base in controls:
        got = H.restate(case.g32, case.K, case.L, var, G, case.metric, case.mask, mut=mut)
        if not (np.array_equal(got.indices, base.indices) and np.array_equal(got.potentials, base.potentials)):
            caught.append(case.name)
    print(mut, "caught on", caught)
    assert caught, mut


# ------------------------------------------------------------------ host helpers and argument errors
def test_trials_and_variates(C):
    assert [C.kmeanspp_trials(k) for k in (1, 2, 3, 8, 20, 21, 64, 65535)] == [2, 2, 3, 4, 4, 5, 6, 13]
    assert all(C.kmeanspp_trials(k) == H.trials(k) for k in range(1, 2000))
    assert C.KMEANSPP_TRIALS_MAX == 16 and C.KMEANSPP_BLOCK_ROWS == 256
    with pytest.raises(ValueError):
        C.kmeanspp_trials(0)
    g = torch.Generator().manual_seed(11)
    v = C.kmeanspp_variates(7, 3, g)
    assert v.dtype == torch.int64 and tuple(v.shape) == (7, 3) and v.device.type == "cpu"
    assert int(v.min()) >= 0 and int(v.max()) < 2 ** 53 and int(v.max()) > 2 ** 48
    assert torch.equal(v, torch.randint(0, 2 ** 53, (7, 3), generator=torch.Generator().manual_seed(11)))
    assert torch.equal(v, torch.from_numpy(H.variates_of(7, 3, 11)))
    for bad in ((0, 3), (4, 0), (4, 17)):
        with pytest.raises(ValueError):
            C.kmeanspp_variates(*bad)


def test_argument_errors_that_need_no_device(C):
    g = torch.zeros(40, 128, dtype=torch.bfloat16)
    ok = C.kmeanspp_variates(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):            # every host check passes: only then the device is asked for
        C.kmeans_plusplus(g, 4, variates=ok)
    with pytest.raises(ValueError, match="metric"):
        C.kmeans_plusplus(g, 4, metric="manhattan")
    with pytest.raises(ValueError, match="bf16 or fp16"):
        C.kmeans_plusplus(g.float(), 4)
    with pytest.raises(ValueError, match="unsupported sizes"):
        C.kmeans_plusplus(torch.zeros(40, 192, dtype=torch.bfloat16), 4)
    for K in (0, 65536):
        with pytest.raises(ValueError, match="K must be"):
            C.kmeans_plusplus(g, K)
    with pytest.raises(ValueError, match="live rows"):
        C.kmeans_plusplus(g, 41)
    for L in (0, 17):
        with pytest.raises(ValueError, match="n_local_trials"):
            C.kmeans_plusplus(g, 4, n_local_trials=L)
    for bad in (ok[:3], ok[:, :2], ok.to(torch.int32), ok.double(), ok.tolist()):
        with pytest.raises(ValueError, match="variates must be"):
            C.kmeans_plusplus(g, 4, variates=bad)
    for val in (-1, 2 ** 53):
        v = ok.clone()
        v[2, 1] = val
        with pytest.raises(ValueError, match="variates must lie"):
            C.kmeans_plusplus(g, 4, variates=v)
    # kmeans keeps the order of its checks: a CPU gallery is a RuntimeError whatever init says
    for init in ("sample", "k-means++", "bogus"):
        with pytest.raises(RuntimeError):
            C.kmeans(g, 4, init=init)


def test_the_header_declares_the_seeding():
    from ctypes import c_float, c_int, c_int64, c_size_t, c_void_p as VP
    from mmr_amd import _header
    Hd = _header.load()
    assert Hd.constants["MMR_KMEANSPP_TRIALS_MAX"] == 16 and Hd.constants["MMR_KMEANSPP_BLOCK_ROWS"] == 256
    assert Hd.functions["mmr_kmeanspp_workspace_bytes"][:2] == (c_size_t, [c_int64, c_int, c_int, c_int])
    restype, argtypes, names = Hd.functions["mmr_kmeanspp_seed"]
    assert restype is c_int
    assert argtypes == [VP, c_int, c_int64, c_int, c_int, c_int, c_int, VP, VP, c_float, VP, VP, VP, VP, VP, VP, c_size_t, VP]
    assert names == ["gallery", "dtype", "N", "E", "K", "L", "metric", "row_mask", "variates_dev", "gallery_norm_bound",
                     "gallery_norm_bound_dev", "indices", "potentials", "shift", "centers", "workspace", "workspace_bytes", "stream"]
    import mmr_amd
    assert {"kmeans_plusplus", "kmeanspp_trials", "kmeanspp_variates"} <= set(mmr_amd.__all__)
    assert mmr_amd.kmeans_plusplus is mmr_amd.cluster.kmeans_plusplus
