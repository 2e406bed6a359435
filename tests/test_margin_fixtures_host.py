"""The preconditions of the margin tests, checked on the CPU (no GPU needed).

tests/test_margin_floor_gpu.py runs fixtures through the search calls whose scan error |acc - dot64| sits at 94 % of the
smallest sound margin (margin_helpers.doc_margin), and counts candidates on pairs crowded just inside it.  This module
proves, with the oracle's own dot64 (oracle/search_ref.c), that the fixtures are what they claim -- so that a failure on the
GPU is the kernel's -- and that each term of the margin has teeth: with G, R, qr or eps_rel halved or dropped, a planted
pair is farther from its threshold than the margin reaches, the first tier's certificate passes without the planted row,
or a candidate count falls under its floor.  ``acc`` below is the scan's product in exact arithmetic (bf16 queries times
the hi half); the MFMA's own accumulation error (at most 2.6 % of 8e-5 |q| G: profiles/mfma_acc_probe.txt) is allowed for
where it matters."""
import functools

import numpy as np
import pytest
import torch

import margin_helpers as M
from search_helpers import dot64

ES = [128, 256, 512, 768]
ACC_ERR = 0.026          # worst MFMA accumulation error, as a share of 8e-5 |q| G (profiles/mfma_acc_probe.txt: 2.1e-6 / 8e-5)


@pytest.fixture(scope="module")
def ref():
    from oracle import search_ref
    return search_ref._load()


@functools.lru_cache(maxsize=None)
def gal_fx(E, self_join=False):
    return M.aligned_gallery_fixture(E, self_join=self_join)


@functools.lru_cache(maxsize=None)
def qry_fx(E):
    return M.aligned_query_fixture(E)


def _bf16_exact(x):
    return np.array_equal(M.bf16_round(x), x)


def _terms(fx, form):
    """(G, R, qr[Q], qh) of a fixture, from the definitions"""
    if not hasattr(fx, "terms"):
        qh = M.bf16_round(fx.q)
        fx.terms = (M.max_norm(fx.g), M.max_norm(fx.g - M.bf16_round(fx.g)), M.resid_norm(fx.q), qh)
    return fx.terms


def test_exact_norm2_is_exact_where_numpy_is_not():
    x = np.array([[2.0 ** 12, 2.0 ** -14, -2.0 ** -14, 1.0], [3.0, 4.0, 0.0, 0.0]], dtype=np.float32)
    n2 = M.exact_norm2(x)
    assert n2[0] == 2.0 ** 24 + 1 + 2.0 ** -27 and n2[1] == 25.0           # 52 bits apart: representable, and fsum finds it
    assert M.exact_norm2(torch.tensor([[0.5, 0.25]], dtype=torch.float16))[0] == 0.3125
    assert M.doc_margin("plain", x[1:], 2.0)[0] == 8e-5 * 5.0 * 2.0
    assert M.doc_margin("split", x[1:], 2.0, R=0.5, qr=[0.25])[0] == 8e-5 * 5.0 * 2.0 * (1 + 2.0 ** -8) + 0.5 + 2.5


@pytest.mark.parametrize("E", ES)
def test_gallery_fixture_is_exact(ref, E):
    fx = gal_fx(E)
    q, g = fx.q, fx.g
    assert fx.N % 32 != 0 and _bf16_exact(q) and np.all(np.abs(q) == M.QMAG)
    assert _bf16_exact(fx.gh) and np.all((np.abs(fx.gh) > 2.0 ** -5) & (np.abs(fx.gh) < 2.0 ** -4 - M.ULP / 2))
    for r in np.concatenate([fx.planted, fx.anti]):
        assert np.array_equal(M.bf16_round(g[r]), fx.gh), "hi of a planted row is gh"
    # the differences below are exact in fp32 and fp64: multiples of 2^-19 under 2^-4
    assert np.all(g[fx.planted].astype(np.float64) - fx.gh == M.DELTA * fx.s)
    assert np.all(g[fx.anti].astype(np.float64) - fx.gh == -M.DELTA * fx.s)
    assert _bf16_exact(g[fx.decoys])
    assert fx.base == dot64(ref, q[0], fx.gh)
    for r in fx.planted:
        assert dot64(ref, q[0], g[r]) == fx.base + fx.D
    for r in fx.anti:
        assert dot64(ref, q[0], g[r]) == fx.base - fx.D
    for r, j in zip(fx.decoys, fx.decoy_j):
        assert dot64(ref, q[0], g[r]) == fx.base + j * M.STEP
    # placement: a 32-row tile of its own each; row 0, a tile's last row, the second stride pass of the 4096-workgroup
    # measuring kernels (rows from 16384), the last row of a short last tile
    special = np.concatenate([fx.planted, fx.anti, fx.decoys])
    assert len(set((special // 32).tolist())) == len(special)
    assert fx.planted[0] == 0 and fx.planted[1] % 32 == 31 and fx.planted[2] > 16384 and fx.planted[3] == fx.N - 1
    # the measured quantities: R is a planted row's, every filler is shorter, rounds closer and scores lower
    G, R, qr, qh = _terms(fx, "split")
    res = M.row_norms(g - M.bf16_round(g))
    assert qr[0] == 0.0 and np.array_equal(qh, q)
    assert set(np.flatnonzero(res == res.max()).tolist()) == set(np.concatenate([fx.planted, fx.anti]).tolist())
    assert abs(R - M.DELTA * np.sqrt(E)) <= 1e-15 * R
    qn = float(np.sqrt(M.exact_norm2(q))[0])
    assert abs(fx.D - qn * R) <= 1e-15 * fx.D                 # dot64 - qh . gh = |q| R: Cauchy-Schwarz with equality
    filler = np.ones(fx.N, dtype=bool)
    filler[special] = False
    d = (q.astype(np.float64) @ g.astype(np.float64).T)[0]
    assert d[filler].max() < fx.base - fx.D and res[filler].max() < 0.6 * R
    assert M.row_norms(g[filler]).max() < 0.6 * G


@pytest.mark.parametrize("E", ES)
def test_gallery_fixture_reaches_the_margin_and_each_term_has_teeth(E):
    fx = gal_fx(E)
    G, R, qr, qh = _terms(fx, "split")
    dm = M.doc_margin("split", qh, G, R=R, qr=qr)[0]
    share = fx.D / dm
    print(f"gallery-aligned E={E}: |acc - dot64| = {share:.4f} of doc_margin; MFMA term {M.R_EPS_REL * np.sqrt(M.exact_norm2(qh))[0] * G * (1 + 2.0 ** -8) / dm:.4f}")
    assert 0.9 <= share < 1.0
    assert fx.D > 2 * M.doc_margin("split", qh, G, R=0.0, qr=qr)[0]          # R dropped: the error is > 2x what is left
    mfma = ACC_ERR * M.R_EPS_REL * np.sqrt(M.exact_norm2(qh))[0] * G
    # R halved: under the threshold that ties dot64 the scan's product is farther away than the margin reaches
    assert fx.D - mfma > M.doc_margin("split", qh, G, R=R / 2, qr=qr)[0]
    # R / 4 (the control of the GPU test): also under the threshold half of |q| R below dot64
    assert fx.D / 2 - mfma > M.doc_margin("split", qh, G, R=R / 4, qr=qr)[0]
    # ... while the honest margin keeps both, and the 2^-8 G fallback is wider still
    assert fx.D + mfma < dm < M.doc_margin("split", qh, G, R=2.0 ** -8 * G, qr=qr)[0]


def _tile_view(fx, acc):
    """(best tile maxima descending, tiles) of the scan's products, 32-row tiles"""
    nt = (fx.N + 31) // 32
    pad = np.full(nt * 32, -np.inf)
    pad[:fx.N] = acc
    tmax = pad.reshape(nt, 32).max(1)
    order = np.lexsort((np.arange(nt), -tmax))
    return tmax, order


@pytest.mark.parametrize("form", ["gallery", "query"])
@pytest.mark.parametrize("E", ES)
def test_topk_ordering_planted_first_and_outside_the_first_tier(ref, form, E):
    from oracle import search_ref
    fx = gal_fx(E) if form == "gallery" else qry_fx(E)
    k = 10
    G, R, qr, qh = _terms(fx, "split")
    oi, _, od = search_ref.cosine_topk(fx.q[:1], fx.g, k)
    assert oi[0, :4].tolist() == sorted(fx.planted.tolist()) and np.all(od[0, :4] == fx.base + fx.D)
    top_decoys = fx.decoys[np.lexsort((fx.decoys, -fx.decoy_j))][:k - 4]
    assert oi[0, 4:].tolist() == top_decoys.tolist()
    assert fx.decoy_j.max() * fx.step < fx.D                                  # every decoy is under the planted rows
    if E == 128:
        assert len(set(fx.decoy_j.tolist())) == M.NDECOY // 2                 # each step value twice
    acc = (qh[:1].astype(np.float64) @ M.bf16_round(fx.g).astype(np.float64).T)[0]
    tmax, order = _tile_view(fx, acc)
    kept, best_out = order[:M.KS_MAX], tmax[order[M.KS_MAX]]
    assert M.NDECOY > M.KS_MAX and not set((fx.planted // 32).tolist()) & set(kept.tolist())
    assert set(kept.tolist()) <= set((fx.decoys // 32).tolist())
    d = (fx.q[:1].astype(np.float64) @ fx.g.astype(np.float64).T)[0]
    rows = (kept[:, None] * 32 + np.arange(32)[None, :]).ravel()
    kth = np.sort(d[rows[rows < fx.N]])[-k]
    dm = M.doc_margin("split", qh[:1], G, R=R, qr=qr[:1])[0]
    mfma = ACC_ERR * M.R_EPS_REL * np.sqrt(M.exact_norm2(qh[:1]))[0] * G
    # the first tier certifies iff kth > best excluded maximum + eps: the honest margin refuses (and the next tier finds
    # the planted rows) ...
    assert kth - best_out + mfma < dm
    # ... and with the targeted term dropped, or a quarter of it (the control), the certificate passes without them
    if form == "gallery":
        weak = M.doc_margin("split", qh[:1], G, R=R / 4, qr=qr[:1])[0]
    else:
        weak = M.doc_margin("split", qh[:1], G, R=R, qr=[0.0])[0]
    assert kth - best_out - mfma > 1.5 * weak
    # deep top-k lists a tile iff its maximum reaches b_k - 2 eps, b_k = the k-th largest tile maximum
    bk = tmax[order[k - 1]]
    assert bk - fx.base + mfma < 2 * dm and bk - fx.base - mfma > 2 * 1.2 * weak


@pytest.mark.parametrize("E", ES)
def test_query_fixture_is_exact_and_reaches_the_margin(ref, E):
    fx = qry_fx(E)
    q, g = fx.q, fx.g
    assert _bf16_exact(g) and np.all(np.abs(g[fx.planted]) == M.QMAG)
    assert np.array_equal(M.bf16_round(q), np.stack([fx.qh, fx.qh])) and _bf16_exact(fx.qh)
    assert np.all(q[0].astype(np.float64) - fx.qh == M.DELTA * np.sign(g[0]))
    assert np.all(q[1].astype(np.float64) - fx.qh == -M.DELTA * np.sign(g[0]))
    assert dot64(ref, fx.qh, g[0]) == 0.0 == fx.base
    for r in fx.planted:
        assert dot64(ref, q[0], g[r]) == fx.D and dot64(ref, q[1], g[r]) == -fx.D
    for r, j in zip(fx.decoys, fx.decoy_j):
        assert dot64(ref, q[0], g[r]) == j * M.QSTEP == dot64(ref, q[1], g[r]) == dot64(ref, fx.qh, g[r])
    special = np.concatenate([fx.planted, fx.decoys])
    assert len(set((special // 32).tolist())) == len(special)
    filler = np.ones(fx.N, dtype=bool)
    filler[special] = False
    d = q.astype(np.float64) @ g.astype(np.float64).T
    assert d[:, filler].max() < -2 * fx.D
    G, R, qr, qh = _terms(fx, "split")
    assert R == 0.0 and G == float(np.sqrt(M.exact_norm2(g[:1]))[0]) and abs(fx.D - qr[0] * G) <= 1e-15 * fx.D
    dm = M.doc_margin("split", qh, G, R=R, qr=qr)
    print(f"query-aligned E={E}: |acc - dot64| = {fx.D / dm[0]:.4f} of doc_margin")
    assert np.all(fx.D >= 0.9 * dm) and np.all(fx.D < dm)
    mfma = ACC_ERR * M.R_EPS_REL * np.sqrt(M.exact_norm2(qh))[0] * G
    assert fx.D > 2 * M.doc_margin("split", qh, G, R=R, qr=[0.0, 0.0])[0]    # qr dropped
    assert fx.D - mfma > M.doc_margin("split", qh, G, R=R, qr=qr / 2)[0]     # qr halved, under the tying threshold


@pytest.mark.parametrize("E", ES)
def test_self_join_fixture_reaches_the_margin(ref, E):
    fx = gal_fx(E, True)
    g, a = fx.g, fx.partner
    G, R, _, _ = _terms(fx, "split")
    ah = M.bf16_round(g[a:a + 1])
    assert np.all(np.abs(ah) == M.QMAG) and G == float(np.sqrt(M.exact_norm2(g[a:a + 1]))[0])
    # in the self-join the query is a row: qr <= R stands in for it
    dm = M.doc_margin("split", ah, G, R=R, qr=[R])[0]
    for r in fx.planted:
        err = dot64(ref, g[a], g[r]) - dot64(ref, ah[0], fx.gh)
        assert err >= 0.9 * dm and err < dm
        assert err > 2 * M.doc_margin("split", ah, G, R=0.0, qr=[0.0])[0]
    print(f"self-join E={E}: |acc - dot64| = {err / dm:.4f} of doc_margin")
    # no pair with a filler comes near the partner's dots: the GPU test's oracle may look at the special rows alone
    special = np.concatenate([fx.planted, fx.anti, fx.decoys, [a]])
    filler = np.ones(fx.N, dtype=bool)
    filler[special] = False
    assert M.row_norms(g[filler]).max() * G < 0.5 * dot64(ref, ah[0], fx.gh)


CROWD = [(dt, E) for dt in (torch.bfloat16, torch.float16) for E in ES]


@functools.lru_cache(maxsize=None)
def crowd(dtype, E):
    return M.crowd_fixture(dtype, E, 20011, 40, 0.5)


@pytest.mark.parametrize("dtype,E", CROWD)
def test_crowd_fixture_fills_the_band_and_half_a_margin_misses_it(ref, dtype, E):
    q, g, dots = crowd(dtype, E)
    tau = 0.5
    qf, gf = M.f32(q), M.f32(g)
    rng = np.random.default_rng(E)
    for a, r in zip(rng.integers(0, q.shape[0], 50), rng.integers(0, g.shape[0], 50)):
        assert abs(dots[a, r] - dot64(ref, qf[a], gf[r])) <= 1e-15
    G = M.max_norm(gf)
    eps = M.doc_margin("plain", qf, G)[:, None]
    band = (dots >= tau - 0.9 * eps) & (dots < tau - 0.5 * eps)
    assert band.sum() >= 200
    floor = int((dots >= tau - 0.9 * eps).sum())
    # G or eps_rel halved: the scan keeps acc >= tau - eps / 2 (1.0001: scan_margin rounds |q| up); with the worst
    # accumulation error on top that is far below the floor
    reach = int((dots >= tau - (0.5 * 1.0001 + ACC_ERR) * eps).sum())
    assert floor - reach >= 150
    # two-sided rule (decide, sweep): the candidates are the pairs within eps of the threshold
    floor2 = int((np.abs(dots - tau) <= 0.9 * eps).sum())
    reach2 = int((np.abs(dots - tau) <= (0.5 * 1.0001 + ACC_ERR) * eps).sum())
    assert floor2 - reach2 >= 300


@pytest.mark.parametrize("dtype,E", CROWD)
def test_assign_crowd_fixture(dtype, E):
    from assign_helpers import ambiguous_rows
    g, c, _ = M.assign_crowd_fixture(dtype, E, 8003, 40)
    gf, cf = M.f32(g), M.f32(c)
    floor = ambiguous_rows(gf, cf, factor=0.9, doc=True)
    half = ambiguous_rows(gf, cf, factor=0.5 * 1.0001 + ACC_ERR, doc=True)
    assert floor.sum() - half.sum() >= 300
