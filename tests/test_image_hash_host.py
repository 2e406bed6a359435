"""Host: the image-hash oracle against itself and against Pillow, the LANCZOS coefficient tables, the hex round trip and
the argument checks of mmr_amd.dedup's image-hash calls.  No GPU: everything here is PIL, numpy and host Python.

The controls at the end replace one step of the literal path by a plausible wrong one and must change a hash on the
fixtures: fixtures on which BICUBIC, a swapped pass order, L after the resize or LSB-first packing give the same hashes
would not tell a wrong kernel from a right one.
"""
import numpy as np
import pytest
import torch
from PIL import Image

import image_hash_helpers as ih
from mmr_amd import dedup
from mmr_amd.preprocess import PRECISION_BITS, resample_tables

# sizes at which no hash is degenerate for a natural image: both sides give whash blocks of at least 2 x 2 at hs = 16
NATURAL_SIZES = [(33, 70), (64, 257), (97, 131), (255, 256), (256, 255), (300, 300), (480, 640)]


def _resize_int(L, ow, oh):
    """Pillow's two-pass 8-bit resize in numpy integers, driven by resample_tables(filter="lanczos")"""
    def one_pass(a, out):                                   # along axis 1
        if a.shape[1] == out:
            return a
        b, c, _ = resample_tables(a.shape[1], out, 0, out, filter="lanczos")
        res = np.empty((a.shape[0], out), np.uint8)
        for x in range(out):
            x0, n = int(b[x, 0]), int(b[x, 1])
            acc = a[:, x0:x0 + n].astype(np.int64) @ c[x, :n].astype(np.int64) + (1 << (PRECISION_BITS - 1))
            res[:, x] = np.clip(acc >> PRECISION_BITS, 0, 255)
        return res
    return one_pass(one_pass(L, ow).T, oh).T


@pytest.mark.parametrize("hw", ih.SIZES)
def test_lanczos_tables_reproduce_pillow(hw):
    h, w = hw
    arr = dict(ih.fixtures(h, w))
    for name in ("natural", "stripes", "noise"):
        L = np.asarray(ih.to_L(arr[name]))
        for hs in ih.HASH_SIZES:
            S = ih.whash_side(h, w, hs)
            for ow, oh in ((hs + 1, hs), (4 * hs, 4 * hs), (S, S)):
                assert np.array_equal(_resize_int(L, ow, oh), ih.resized(arr[name], ow, oh)), (name, hs, ow, oh)


def test_identity_tables_are_the_identity():
    # a pass whose input and output size are equal is skipped by Pillow; the tables make it a copy
    for n in (1, 9, 17, 32, 64, 256):
        b, c, _ = resample_tables(n, n, 0, n, filter="lanczos")
        for x in range(n):
            row = np.zeros(n, np.int64)
            row[b[x, 0]: b[x, 0] + b[x, 1]] = c[x, :b[x, 1]]
            assert row[x] == 1 << PRECISION_BITS and np.count_nonzero(row) == 1


def test_luma_formula_is_pillows():
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (7, 5), (33, 70), (64, 257), (97, 131), (300, 300)):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        mine = (a[..., 0].astype(np.int64) * 19595 + a[..., 1].astype(np.int64) * 38470 + a[..., 2].astype(np.int64) * 7471 + 0x8000) >> 16
        assert np.array_equal(mine.astype(np.uint8), np.asarray(ih.to_L(a)))


# the shapes tests/test_preprocess.py resizes, to 224 and 64 pixels
_PREPROCESS_SIZES = [(37, 53), (224, 224), (300, 200), (200, 300), (1000, 751), (97, 640), (224, 225), (64, 64), (231, 500)]


def _bicubic_parent(in_size, out_size, first, count):
    """the table builder as it stood before the filter argument, restated: bicubic, support 2"""
    import math

    def bicubic(x, a=-0.5):
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0

    scale = float(np.float32(in_size) - np.float32(0.0)) / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = (int(math.ceil(support)) * 2 + 1 + 3) // 4 * 4
    bounds, coeffs = np.zeros((count, 2), np.int32), np.zeros((count, ksize), np.int32)
    for j in range(count):
        center = 0.0 + (first + j + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [bicubic((x + xmin - center + 0.5) * (1.0 / fs)) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        for x, v in enumerate(k):
            coeffs[j, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[j] = (xmin, xmax)
    return bounds, coeffs, ksize


@pytest.mark.parametrize("hw", _PREPROCESS_SIZES)
def test_bicubic_tables_are_unchanged(hw):
    from mmr_amd.preprocess import resize_geometry

    h, w = hw
    for n_px in (224, 64):
        nh, nw, top, left = resize_geometry(h, w, n_px)
        for args in ((w, nw, left, n_px), (h, nh, top, n_px)):
            want = _bicubic_parent(*args)
            for got in (resample_tables(*args), resample_tables(*args, filter="bicubic")):
                assert got[2] == want[2] and got[0].dtype == np.int32 and got[1].dtype == np.int32
                assert got[0].tobytes() == want[0].tobytes() and got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes()


def test_unknown_filter_is_refused():
    with pytest.raises(ValueError, match="filter"):
        resample_tables(10, 5, 0, 5, filter="box")


@pytest.mark.parametrize("hs", ih.HASH_SIZES)
@pytest.mark.parametrize("hw", NATURAL_SIZES)
def test_rule_path_equals_literal_path_on_natural_images(hw, hs):
    arr = dict(ih.fixtures(*hw))
    for name in ("natural", "noise"):
        bits, status = ih.rule_bits(arr[name], hs)
        # pure noise may tie whash's two middle block sums (16 pixels per block at 97 x 131, hs = 16): a flagged kind is
        # not compared, an unflagged one always is
        assert status == 0 or name == "noise", (name, status)
        lit = ih.literal_bits(arr[name], hs)
        for k, flag in zip(ih.KINDS, (ih.PHASH_NEAR_MEDIAN, 0, ih.WHASH_TIED_MEDIAN)):
            if not status & flag:
                assert np.array_equal(bits[k], lit[k]), (name, k)


@pytest.mark.parametrize("hs", ih.HASH_SIZES)
@pytest.mark.parametrize("hw", [(16, 16), (97, 131), (300, 300)])
def test_degenerate_status_bits(hw, hs):
    arr = dict(ih.fixtures(*hw))
    for name in ("zeros", "ones", "flat128"):
        # one non-zero coefficient, hs*hs - 1 rounding residues around a zero median; all block sums equal
        bits, status = ih.rule_bits(arr[name], hs)
        assert status == ih.PHASH_NEAR_MEDIAN | ih.WHASH_TIED_MEDIAN, name
        assert not bits["dhash"].any() and not bits["whash"].any() and not bits["phash"][1:].any()
    for name in ("halves", "stripes"):
        # constant along y: only row u = 0 of the DCT is non-zero, so the median sits among residues
        _, status = ih.rule_bits(arr[name], hs)
        assert status & ih.PHASH_NEAR_MEDIAN, name
    # left half 0, right half 255: the two middle block sums come from different halves
    _, status = ih.rule_bits(arr["halves"], hs)
    assert not status & ih.WHASH_TIED_MEDIAN


def test_one_pixel_image_is_flagged():
    for hs in ih.HASH_SIZES:
        _, status = ih.rule_bits(np.full((1, 1, 3), 77, np.uint8), hs)
        assert status == ih.PHASH_NEAR_MEDIAN | ih.WHASH_TIED_MEDIAN


def test_stripes_reach_both_clips():
    # the horizontal pass of the striped fixture over- and undershoots before the clip: 0 and 255 are both produced by it
    h, w = 97, 131
    L = np.asarray(ih.to_L(dict(ih.fixtures(h, w))["stripes"])).astype(np.int64)
    b, c, _ = resample_tables(w, 9, 0, 9, filter="lanczos")
    raw = np.array([(L[0, b[x, 0]: b[x, 0] + b[x, 1]] * c[x, :b[x, 1]]).sum() + (1 << (PRECISION_BITS - 1)) for x in range(9)]) >> PRECISION_BITS
    wide = dict(ih.fixtures(64, 257))["stripes"]
    S = ih.whash_side(64, 257, 8)
    Lw = np.asarray(ih.to_L(wide)).astype(np.int64)
    b, c, _ = resample_tables(257, S, 0, S, filter="lanczos")
    raw_w = np.array([(Lw[0, b[x, 0]: b[x, 0] + b[x, 1]] * c[x, :b[x, 1]]).sum() + (1 << (PRECISION_BITS - 1)) for x in range(S)]) >> PRECISION_BITS
    both = np.concatenate([raw, raw_w])
    assert both.min() < 0 and both.max() > 255


def test_matrix_dct_is_scipys():
    fft = pytest.importorskip("scipy.fftpack")
    for hs in ih.HASH_SIZES:
        p = ih.planes(dict(ih.fixtures(97, 131))["natural"], hs)["phash"].astype(np.float64)
        want = fft.dct(fft.dct(p, axis=0), axis=1)[:hs, :hs]
        for got in (ih.dct_matrix(p, hs), ih.phash_coefficients(p, hs)):
            assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
            assert np.array_equal(got > np.median(got), want > np.median(want))
    assert np.array_equal(dedup.dct_cosine_table(8), ih.cos_table(8)) and np.array_equal(dedup.dct_cosine_table(16), ih.cos_table(16))


def test_whash_side():
    for h, w in ih.SIZES + [ih.BIG]:
        for hs in ih.HASH_SIZES:
            assert dedup.whash_side(h, w, hs) == ih.whash_side(h, w, hs)


# ---------------------------------------------------------------------------------------------------------------- hex
@pytest.mark.parametrize("hs", ih.HASH_SIZES)
def test_hex_round_trip(hs):
    rng = np.random.default_rng(hs)
    W = hs * hs // 64
    h = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, (50, 3, W), dtype=np.int64, endpoint=True)
    h[0] = np.iinfo(np.int64).min                    # bit 63 alone
    h[1] = -1
    h[2] = 0
    h[3, :, 0] = 1                                   # leading zeros survive
    rows = dedup.hashes_to_hex(torch.from_numpy(h), hs)
    assert all(len(s) == hs * hs // 4 and s == s.lower() for row in rows for s in row)
    assert torch.equal(dedup.hashes_from_hex(rows), torch.from_numpy(h))
    assert rows[0][0].startswith("8") and set(rows[1][1]) == {"f"} and set(rows[2][2]) == {"0"}
    assert dedup.hashes_to_hex(h, hs) == rows                       # numpy in, same strings


def test_hex_is_imagehash_format():
    arr = dict(ih.fixtures(97, 131))["natural"]
    for hs in ih.HASH_SIZES:
        bits, _ = ih.rule_bits(arr, hs)
        words = np.stack([ih.pack(bits[k]) for k in ih.KINDS])[None]
        assert dedup.hashes_to_hex(words, hs) == [tuple(ih.to_hex(bits[k]) for k in ih.KINDS)]
        assert torch.equal(dedup.hashes_from_hex([ih.literal_hex(arr, hs)]), torch.from_numpy(words))


def test_hashes_to_hex_argument_errors():
    with pytest.raises(ValueError, match="hash_size"):
        dedup.hashes_to_hex(np.zeros((1, 3, 1), np.int64), 12)
    with pytest.raises(ValueError, match="int64"):
        dedup.hashes_to_hex(np.zeros((1, 3, 1), np.int32), 8)
    with pytest.raises(ValueError, match="hash_size=16"):
        dedup.hashes_to_hex(np.zeros((1, 3, 1), np.int64), 16)
    with pytest.raises(ValueError, match="hash_size=8"):
        dedup.hashes_to_hex(np.zeros((1, 3, 4), np.int64), 8)


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_image_hashes_argument_errors():
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        dedup.image_hashes([img])
    with pytest.raises(ValueError, match="hash_size"):
        dedup.image_hashes([img], hash_size=12)
    with pytest.raises(ValueError, match="kinds"):
        dedup.image_hashes([img], kinds=())
    with pytest.raises(ValueError, match="kinds"):
        dedup.image_hashes([img], kinds=("ahash",))
    with pytest.raises(ValueError, match="order"):
        dedup.image_hashes([img], kinds=("dhash", "phash"))
    with pytest.raises(ValueError, match="uint8"):
        dedup.image_hashes([img.float()])
    with pytest.raises(ValueError, match="uint8"):
        dedup.image_hashes([torch.zeros(8, 8, 4, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="empty"):
        dedup.image_hashes([])
    with pytest.raises(ValueError, match=r"\[B,H,W,3\]"):
        dedup.image_hashes(torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="keys"):
        dedup.find_image_duplicates(["a", "b"], [img])


# ---------------------------------------------------------------------------------------------------------------- controls
def _hex_set(**controls):
    return [ih.literal_hex(dict(ih.fixtures(h, w))["natural"], hs, **controls) for h, w in NATURAL_SIZES for hs in ih.HASH_SIZES]


def test_control_bicubic_differs():
    assert _hex_set(resample=Image.BICUBIC) != _hex_set()


def test_control_vertical_pass_first_differs():
    # hash bits are a lossy view of the bytes, so the control is judged on the bytes the GPU tests compare
    diff = 0
    for h, w in NATURAL_SIZES:
        arr = dict(ih.fixtures(h, w))["natural"]
        swapped = np.asarray(ih.to_L(arr).resize((w, 32), Image.LANCZOS).resize((32, 32), Image.LANCZOS))
        diff += int((swapped != ih.resized(arr, 32, 32)).sum())
    assert diff > 0


def test_control_luma_after_resize_differs():
    diff = 0
    for h, w in NATURAL_SIZES:
        arr = dict(ih.fixtures(h, w))["natural"]
        late = np.asarray(Image.fromarray(arr, "RGB").resize((32, 32), Image.LANCZOS).convert("L"))
        diff += int((late != ih.resized(arr, 32, 32)).sum())
    assert diff > 0


def test_control_lsb_first_packing_differs():
    arr = dict(ih.fixtures(97, 131))["natural"]
    bits, _ = ih.rule_bits(arr, 8)
    for k in ih.KINDS:
        assert not np.array_equal(ih.pack(bits[k]), ih.pack(bits[k], lsb_first=True))
