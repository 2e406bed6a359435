"""CPU: the oracle against the committed golden vectors (no GPU, no transformers import).

The goldens are outputs of transformers.CLIPModel / the reference's torch expression,
written by oracle/make_golden.py in the dev container.
"""
import os

import numpy as np
import pytest
import torch

import mmr_amd
from mmr_amd import synth, weights
from oracle import clip_ref, search_ref


def _gold(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


@pytest.mark.parametrize("name,fn", [("tiny-test", "encoder_tiny-test.npz"), ("ViT-B/32", "encoder_ViT-B-32.npz"),
                                     ("ViT-B/16", "encoder_ViT-B-16.npz")])
def test_encoder_oracle_matches_hf_golden(golden_dir, name, fn):
    g = _gold(golden_dir, fn)
    ccfg = mmr_amd.get_config(name)
    w = weights.make_clip_weights(ccfg, seed=int(g["weight_seed"]))
    px = synth.synth_images(int(g["n_img"]), ccfg.vision.image_size, seed=int(g["image_seed"]))
    ids = synth.synth_token_ids(int(g["n_txt"]), ccfg.text.tokens, ccfg.text.vocab, seed=int(g["text_seed"]))
    st = {}
    with torch.no_grad():
        img = clip_ref.encode_image(w, ccfg.vision, px, stages=st)
        txt = clip_ref.encode_text(w, ccfg.text, ids)
        lpi, lpt = clip_ref.clip_forward(w, ccfg, px, ids)
    assert np.abs(img.numpy() - g["image_features"]).max() <= 3e-5
    assert np.abs(txt.numpy() - g["text_features"]).max() <= 3e-5
    assert np.abs(lpi.numpy() - g["logits_per_image"]).max() <= 1e-4
    assert np.abs(lpt.numpy() - g["logits_per_text"]).max() <= 1e-4
    if "v_ln_pre" in g:
        assert np.abs(st["ln_pre"].numpy() - g["v_ln_pre"]).max() <= 3e-5
        assert np.abs(st["layer0"].numpy() - g["v_layer0"]).max() <= 3e-5
        assert np.abs(st["pooled"].numpy() - g["v_pooled"]).max() <= 5e-5


def test_encoder_oracle_rejects_wrong_image_size():
    ccfg = mmr_amd.get_config("tiny-test")
    w = weights.make_vision_weights(ccfg.vision)
    with pytest.raises(ValueError):
        clip_ref.encode_image(w, ccfg.vision, torch.zeros(1, 3, 32, 32))


def test_text_pooling_is_first_eot():
    ids = synth.synth_token_ids(16, 77, 1024, seed=9)
    assert (ids[:, 0] == 1022).all()
    eot = ids.long().argmax(-1)
    for i in range(16):
        assert ids[i, eot[i]] == 1023 and (ids[i, eot[i] + 1:] == 0).all() and (ids[i, 1:eot[i]] < 1022).all()


@pytest.mark.parametrize("N", [1000, 10000])
@pytest.mark.parametrize("Q", [1, 7, 128])
@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_search_oracle_matches_golden(golden_dir, N, Q, tag):
    g = _gold(golden_dir, "search.npz")
    key = f"N{N}_Q{Q}_{tag}"
    gal = synth.synth_unit_rows(N, 512, seed=int(g["meta"][0]))
    q = synth.synth_unit_rows(Q, 512, seed=int(g[key + "_qseed"]))
    if tag == "bf16":
        gal, q = gal.bfloat16(), q.bfloat16()
    idx, score, s64 = search_ref.cosine_topk(q, gal, 10, scale=100.0)
    assert np.array_equal(idx.astype(np.int32), g[key + "_idx"])
    assert np.array_equal(score, g[key + "_score"])
    assert np.array_equal(s64, g[key + "_dot64"])
    # the reference's own expression agrees on these tie-free fixtures
    ridx, rval = search_ref.reference_expression_topk(gal.float(), q.float(), 10, 100.0)
    assert np.array_equal(ridx.numpy(), idx)
    assert np.abs(rval.numpy() - score).max() < 1e-3


def test_search_oracle_tie_rule(golden_dir):
    g = _gold(golden_dir, "search.npz")
    gal = synth.synth_unit_rows(2048, 512, seed=int(g["meta"][1])).bfloat16()
    q = synth.synth_unit_rows(5, 512, seed=int(g["meta"][2])).bfloat16()
    gal[1500:1520] = gal[7]
    gal[40] = gal[900]
    q[0] = gal[7]
    q[1] = gal[900]
    idx, score, s64 = search_ref.cosine_topk(q, gal, 10, scale=100.0)
    assert np.array_equal(idx.astype(np.int32), g["ties_idx"])
    assert list(idx[0]) == [7] + list(range(1500, 1509))      # ties -> lowest index first
    assert np.array_equal(s64, g["ties_dot64"])


def test_search_oracle_edge_cases():
    gal = synth.synth_unit_rows(5, 128, seed=3)
    q = synth.synth_unit_rows(2, 128, seed=4)
    idx, score, _ = search_ref.cosine_topk(q, gal, 8)          # k > N
    assert (idx[:, 5:] == -1).all() and np.isinf(score[:, 5:]).all()
    assert sorted(idx[0, :5].tolist()) == [0, 1, 2, 3, 4]
    sim = search_ref.similarity(q, gal, scale=100.0)
    assert np.allclose(sim, 100.0 * (q @ gal.t()).numpy(), atol=1e-4)
    # merge of two shards == search over the concatenation
    a, b = gal[:3], gal[3:]
    ia, _, sa = search_ref.cosine_topk(q, a, 4)
    ib, _, sb = search_ref.cosine_topk(q, b, 4)
    ib = np.where(ib >= 0, ib + 3, ib)
    mi, ms, _ = search_ref.topk_merge(np.stack([ia, ib]), np.stack([sa, sb]))
    fi, fs, _ = search_ref.cosine_topk(q, gal, 4)
    assert np.array_equal(mi, fi) and np.array_equal(ms, fs)
    n = search_ref.l2norm_rows(torch.randn(4, 128) * 3)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)


# ------------------------------------------------------------------ numeric edges of the search oracle (include/mmr.h,
# "Non-finite values, ties and scale"): the oracle must be right here before it can judge the kernels
def _compacted(q, g, keep, k, scale=1.0):
    """oracle over g[keep] with ids mapped back: NaN-free galleries are the part of the oracle the goldens pin"""
    rows = np.flatnonzero(keep)
    oi, os_, od = search_ref.cosine_topk(q, g[rows], k, scale=scale)
    return np.where(oi >= 0, rows[np.clip(oi, 0, None)], -1), os_, od


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


@pytest.mark.parametrize("bf16", [False, True])
def test_search_oracle_nan_rows_are_absent(bf16):
    g = synth.synth_unit_rows(200, 128, seed=11)
    q = synth.synth_unit_rows(6, 128, seed=12)
    if bf16:
        g, q = g.bfloat16().float(), q.bfloat16().float()
    g, q = g.numpy().copy(), q.numpy()
    clean = search_ref.cosine_topk(q, g, 10)
    bad = [3] if not bf16 else [0, 3, 4, 150, 199]
    g[bad] = np.nan
    g[77, 5] = np.nan                                   # one element poisons the whole row
    keep = np.ones(200, bool)
    keep[bad + [77]] = False
    got = search_ref.cosine_topk(q, g, 10, scale=100.0)
    assert _same_bits(got, _compacted(q, g, keep, 10, scale=100.0))
    assert not np.isin(got[0], bad + [77]).any() and not np.isnan(got[2]).any() and not np.isnan(got[1]).any()
    assert (got[0] >= 0).all()
    # a NaN among the first k rows used to stick in the list and block every later row
    assert got[0][0][:4].tolist() != [1, 0, 2, 3]
    for qi in range(6):                                 # rows untouched by the poison keep their place and their bits
        m = ~np.isin(clean[0][qi], bad + [77])
        n = int(m.sum())
        assert np.array_equal(got[0][qi][:n], clean[0][qi][m]) and np.array_equal(got[2][qi][:n], clean[2][qi][m])
    # all rows but 7 are NaN: 7 results, then empty slots
    keep7 = np.zeros(200, bool)
    keep7[[1, 20, 21, 60, 100, 101, 198]] = True
    g7 = np.where(keep7[:, None], g, np.float32(np.nan))
    got = search_ref.cosine_topk(q, g7, 10)
    assert _same_bits(got, _compacted(q, g7, keep7, 10))
    assert (got[0][:, 7:] == -1).all() and np.isneginf(got[2][:, 7:]).all() and (got[0][:, :7] >= 0).all()
    # a NaN query: every slot empty
    qn = q.copy()
    qn[2, 9] = np.nan
    got = search_ref.cosine_topk(qn, g, 10)
    assert (got[0][2] == -1).all() and np.isneginf(got[1][2]).all() and np.isneginf(got[2][2]).all()
    assert np.array_equal(got[0][[0, 1, 3, 4, 5]], _compacted(q, g, keep, 10)[0][[0, 1, 3, 4, 5]])


def test_search_oracle_infinite_dots_are_ordinary_numbers():
    N, E, k = 8, 128, 8
    g = synth.synth_unit_rows(N, E, seed=13).numpy().copy()
    q = synth.synth_unit_rows(3, E, seed=14).numpy().copy()
    g[5, 17] = np.inf
    q[0, 17], q[1, 17], q[2, 17] = 0.0, 0.25, -0.25     # dot with row 5: NaN, +inf, -inf
    idx, score, d64 = search_ref.cosine_topk(q, g, k, scale=100.0)
    keep = np.arange(N) != 5
    assert _same_bits((idx[:1], score[:1], d64[:1]), _compacted(q[:1], g, keep, k, scale=100.0))   # NaN for this query only
    assert idx[0, 7] == -1 and 5 not in idx[0]
    assert idx[1, 0] == 5 and d64[1, 0] == np.inf and score[1, 0] == np.inf                           # +inf ranks first
    assert idx[2, 7] == 5 and d64[2, 7] == -np.inf and score[2, 7] == -np.inf                         # -inf last, but present
    rest = _compacted(q[1:], g, keep, k - 1)
    assert np.array_equal(idx[1, 1:], rest[0][0]) and np.array_equal(idx[2, :7], rest[0][1])
    # with k better rows the -inf row is simply not in the list
    assert 5 not in search_ref.cosine_topk(q[2:], g, 7)[0]
    sim = search_ref.similarity(q, g, 100.0)
    assert np.isnan(sim[0, 5]) and sim[1, 5] == np.inf and sim[2, 5] == -np.inf and np.isfinite(np.delete(sim, 5, 1)).all()


def test_search_oracle_zero_query_ties_with_every_row():
    g = synth.synth_unit_rows(300, 128, seed=15).numpy()       # random signs: partial sums cancel to +0.0 or stay +0.0
    assert (g < 0).any() and (g > 0).any()
    q = np.zeros((2, 128), np.float32)
    q[1] = -0.0                                                # products are -0.0 / +0.0; the sum from +0.0 is +0.0
    idx, score, d64 = search_ref.cosine_topk(q, g, 10)
    assert np.array_equal(idx, np.tile(np.arange(10), (2, 1)))
    assert (d64 == 0).all() and not np.signbit(d64).any() and not np.signbit(score).any()


@pytest.mark.parametrize("e", [-60, 60])
@pytest.mark.parametrize("bf16", [False, True])
def test_search_oracle_power_of_two_scaling_is_exact(e, bf16):
    g = synth.synth_unit_rows(500, 128, seed=16)
    q = synth.synth_unit_rows(7, 128, seed=17)
    if bf16:
        g, q = g.bfloat16().float(), q.bfloat16().float()
    g, q = g.numpy(), q.numpy()
    gs = np.ldexp(g, e).astype(np.float32)
    assert np.isfinite(gs).all() and np.array_equal(np.ldexp(gs.astype(np.float64), -e), g.astype(np.float64))
    i0, s0, d0 = search_ref.cosine_topk(q, g, 10)
    for qq, gg, ee in ((q, gs, e), (np.ldexp(q, e).astype(np.float32), g, e), (np.ldexp(q, e // 2).astype(np.float32), gs, e + e // 2)):
        i1, s1, d1 = search_ref.cosine_topk(qq, gg, 10)
        assert np.array_equal(i1, i0)
        assert np.array_equal(d1.view(np.int64), np.ldexp(d0, ee).view(np.int64))
        with np.errstate(over="ignore"):
            assert np.array_equal(s1, np.ldexp(d0, ee).astype(np.float32))


def test_search_oracle_merge_edges():
    nan, inf = np.nan, np.inf
    # [parts=3, Q=2, k=4]; part 2 is all-empty.  Query 0: NaN candidate, id 9 in two parts with the same dot, ties
    # across parts; query 1: only -inf candidates, a NaN one and an empty slot that carries a large dot
    ids = np.array([[[5, 9, 2, -1], [4, -1, 6, -1]],
                    [[7, 9, 3, 11], [1, -1, -1, -1]],
                    [[-1, -1, -1, -1], [-1, -1, -1, -1]]], np.int64)
    dots = np.array([[[1.0, 0.5, nan, 0.0], [-inf, 9.0, nan, 0.0]],
                     [[1.0, 0.5, 0.5, -inf], [-inf, 0.0, 0.0, 0.0]],
                     [[3.0, 3.0, 3.0, 3.0], [-inf, -inf, -inf, -inf]]], np.float64)
    idx, score, d64 = search_ref.topk_merge(ids, dots, scale=2.0)
    assert idx.tolist() == [[5, 7, 3, 9], [1, 4, -1, -1]]
    assert np.array_equal(d64, np.array([[1.0, 1.0, 0.5, 0.5], [-inf, -inf, -inf, -inf]]))
    assert np.array_equal(score, np.array([[2.0, 2.0, 1.0, 1.0], [-inf, -inf, -inf, -inf]], np.float32))
    # k = 6 reaches past the finite candidates: the -inf one is returned with its id, then empty slots
    ids6 = np.concatenate([ids[:, :1], np.full((3, 1, 2), -1, np.int64)], axis=2)
    dots6 = np.concatenate([dots[:, :1], np.zeros((3, 1, 2))], axis=2)
    idx, score, d64 = search_ref.topk_merge(ids6, dots6)
    assert idx.tolist() == [[5, 7, 3, 9, 11, -1]] and d64[0, 4] == -inf and d64[0, 5] == -inf
