"""The oracle of the image-hash tests: imagehash 4.x's phash / dhash / whash restated with PIL and numpy only.

Two paths per image.
  literal_*: what imagehash does, step for step -- ``convert("L").resize(..., LANCZOS)`` by Pillow itself, then the DCT as a
             matrix product (scipy.fftpack.dct type 2 is that sum), or the float Haar path of whash (orthonormal wavedec2 to
             the top level, zero the LL, waverec2, wavedec2 to level log2(S / hs)), then ``> median``, then imagehash's hex.
  rule_*:    the contract of include/mmr.h -- the same Pillow bytes, phash as the fp64 sums in the device's order with the
             eps margin, whash as integer block sums against the two middle values -- with the status bits.
The two agree wherever status is 0; where it is not, imagehash's own bits are floating-point noise.
imagehash and pywt themselves are not used (they are not installed where this runs); whash rests on the derivation in
DESIGN.md section 3 plus the literal Haar restatement below.
"""
import functools
import math

import numpy as np
from PIL import Image

KINDS = ("phash", "dhash", "whash")
PHASH_NEAR_MEDIAN, WHASH_TIED_MEDIAN = 1, 2

# (H, W): the identity pass of every target (9 and 17 wide, 8 and 16 high, 32, 64, powers of two), upscaling, a row stride
# that is no multiple of 4, either side straddling a power of two, widths beyond any 256- or 1024-column block
SIZES = [(1, 1), (7, 5), (8, 9), (3, 200), (16, 16), (32, 32), (33, 70), (64, 257), (97, 131), (255, 256), (256, 255),
         (300, 300), (480, 640), (513, 1025)]
BIG = (1200, 1600)
HASH_SIZES = (8, 16)


# ---------------------------------------------------------------------------------------------------------------- images
def natural(h, w, seed):
    """low-resolution random RGB, upsampled bicubically, plus +-6 uniform noise: smooth structure with texture"""
    rng = np.random.default_rng(seed)
    lh, lw = max(2, h // 24 + 2), max(2, w // 24 + 2)
    low = Image.fromarray(rng.integers(0, 256, (lh, lw, 3), dtype=np.uint8), "RGB")
    up = np.asarray(low.resize((w, h), Image.BICUBIC)).astype(np.int16)
    return np.clip(up + rng.integers(-6, 7, up.shape), 0, 255).astype(np.uint8)


def degenerate(h, w):
    """name -> RGB image: the cases where a hash is ill-defined or the resize clips"""
    out = {"zeros": np.zeros((h, w, 3), np.uint8), "ones": np.full((h, w, 3), 255, np.uint8),
           "flat128": np.full((h, w, 3), 128, np.uint8)}
    halves = np.zeros((h, w, 3), np.uint8)
    halves[:, w // 2:] = 255
    out["halves"] = halves
    period = max(2, 2 * (w // 9))                      # near the dhash downscale factor: over- and undershoot, both clips
    stripes = np.zeros((h, w, 3), np.uint8)
    stripes[:, (np.arange(w) % period) < period // 2] = 255
    out["stripes"] = stripes
    out["noise"] = np.random.default_rng(h * 100003 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def fixtures(h, w):
    """[(name, RGB uint8 [h,w,3])]: one natural image and the degenerate ones of that size (read-only)"""
    items = [("natural", natural(h, w, seed=h * 7919 + w))] + list(degenerate(h, w).items())
    for _, a in items:
        a.setflags(write=False)
    return items


# ---------------------------------------------------------------------------------------------------------------- pieces
def to_L(arr):
    arr = np.ascontiguousarray(arr)
    return Image.fromarray(arr, "RGB").convert("L") if arr.ndim == 3 else Image.fromarray(arr, "L")


def resized(arr, w, h, resample=Image.LANCZOS):
    """uint8 [h, w]: Pillow's convert("L").resize((w, h), LANCZOS)"""
    return np.asarray(to_L(arr).resize((w, h), resample))


def whash_side(h, w, hs):
    return max(2 ** int(math.log2(min(h, w))), hs)


@functools.lru_cache(maxsize=None)
def cos_table(hs):
    n = 4 * hs
    return np.array([[math.cos(math.pi * (2 * x + 1) * v / (2 * n)) for x in range(n)] for v in range(hs)], dtype=np.float64)


def dct_matrix(p, hs):
    """d[u][v], u, v < hs, of scipy.fftpack.dct(dct(p, axis=0), axis=1) (type 2, unnormalised), as a matrix product"""
    C = cos_table(hs)
    return 4.0 * (C @ p.astype(np.float64) @ C.T)


def planes(arr, hs):
    """the three resized images: dict(dhash [hs, hs+1], phash [4hs, 4hs], whash [S, S])"""
    h, w = arr.shape[:2]
    S = whash_side(h, w, hs)
    return {"dhash": resized(arr, hs + 1, hs), "phash": resized(arr, 4 * hs, 4 * hs), "whash": resized(arr, S, S)}


def block_sums(p, hs):
    B = p.shape[0] // hs
    return p.astype(np.int64).reshape(hs, B, hs, B).sum(axis=(1, 3))


# ---------------------------------------------------------------------------------------------------------------- literal
_S2 = 1.0 / math.sqrt(2.0)


def _haar_dwt2(x):
    lo, hi = _S2 * x[:, 0::2] + _S2 * x[:, 1::2], _S2 * x[:, 0::2] - _S2 * x[:, 1::2]
    return (_S2 * lo[0::2] + _S2 * lo[1::2], _S2 * lo[0::2] - _S2 * lo[1::2],
            _S2 * hi[0::2] + _S2 * hi[1::2], _S2 * hi[0::2] - _S2 * hi[1::2])


def _haar_idwt2(ll, lh, hl, hh):
    lo = np.empty((ll.shape[0] * 2, ll.shape[1]))
    hi = np.empty_like(lo)
    lo[0::2], lo[1::2] = _S2 * ll + _S2 * lh, _S2 * ll - _S2 * lh
    hi[0::2], hi[1::2] = _S2 * hl + _S2 * hh, _S2 * hl - _S2 * hh
    x = np.empty((lo.shape[0], lo.shape[1] * 2))
    x[:, 0::2], x[:, 1::2] = _S2 * lo + _S2 * hi, _S2 * lo - _S2 * hi
    return x


def _wavedec2(x, level):
    details = []
    for _ in range(level):
        x, *d = _haar_dwt2(x)
        details.append(d)
    return x, details[::-1]


def _waverec2(ll, details):
    for d in details:
        ll = _haar_idwt2(ll, *d)
    return ll


def literal_bits(arr, hs, resample=Image.LANCZOS, vertical_first=False, luma_last=False):
    """kind -> bool [hs, hs], imagehash's own steps.  The keyword arguments build the failing controls."""
    h, w = arr.shape[:2]
    S = whash_side(h, w, hs)

    def R(ow, oh):
        if luma_last:                       # L after the resize
            return np.asarray(Image.fromarray(np.ascontiguousarray(arr), "RGB").resize((ow, oh), resample).convert("L"))
        if vertical_first:                  # vertical pass, then horizontal
            return np.asarray(to_L(arr).resize((w, oh), resample).resize((ow, oh), resample))
        return resized(arr, ow, oh, resample)

    out = {}
    d = dct_matrix(R(4 * hs, 4 * hs), hs)
    out["phash"] = d > np.median(d)
    p = R(hs + 1, hs)
    out["dhash"] = p[:, 1:] > p[:, :-1]
    pixels = R(S, S) / 255.0
    top, level = int(math.log2(S)), int(math.log2(S)) - int(math.log2(hs))
    ll, det = _wavedec2(pixels, top)
    pixels = _waverec2(ll * 0, det)
    low, _ = _wavedec2(pixels, level)
    out["whash"] = low > np.median(low)
    return out


def to_hex(bits):
    """imagehash's str(): bits.flatten() as one big-endian binary number, in hex"""
    flat = bits.flatten()
    return "{:0>{w}x}".format(int("".join(str(int(b)) for b in flat), 2), w=math.ceil(flat.size / 4))


def literal_hex(arr, hs, kinds=KINDS, **controls):
    b = literal_bits(arr, hs, **controls)
    return tuple(to_hex(b[k]) for k in kinds)


# ---------------------------------------------------------------------------------------------------------------- rule
def phash_coefficients(p, hs):
    """d[u][v] in the device's order: t[y][v] = sum_x p[y][x] C[v][x] (x ascending), d = 4 sum_y C[u][y] t[y][v]
    (y ascending), every product and every sum rounded to fp64"""
    C, n = cos_table(hs), 4 * hs
    pf = p.astype(np.float64)
    t = np.zeros((n, hs))
    for x in range(n):
        t = t + pf[:, x][:, None] * C[None, :, x]
    d = np.zeros((hs, hs))
    for y in range(n):
        d = d + C[:, y][:, None] * t[y][None, :]
    return 4.0 * d


def rule_bits(arr, hs):
    """(kind -> bool [hs, hs], status): the contract's rules on Pillow's bytes"""
    pl = planes(arr, hs)
    out, status = {}, 0
    d = phash_coefficients(pl["phash"], hs)
    srt = np.sort(d, axis=None)
    med = (srt[d.size // 2 - 1] + srt[d.size // 2]) * 0.5
    eps = 2.0 ** -32 * d[0, 0]
    diff = d - med
    out["phash"] = diff > eps
    if (np.abs(diff) <= eps).any():
        status |= PHASH_NEAR_MEDIAN
    p = pl["dhash"]
    out["dhash"] = p[:, 1:] > p[:, :-1]
    s = block_sums(pl["whash"], hs)
    srt = np.sort(s, axis=None)
    a, b = int(srt[s.size // 2 - 1]), int(srt[s.size // 2])
    out["whash"] = 2 * s > a + b
    if a == b:
        status |= WHASH_TIED_MEDIAN
    return out, status


def pack(bits, lsb_first=False):
    """bool [hs, hs] -> int64 [hs*hs/64]: flatten, most significant bit first, element [0][0] is bit 63 of word 0"""
    flat = bits.flatten().astype(np.uint8)
    words = []
    for w in range(flat.size // 64):
        chunk = flat[64 * w: 64 * w + 64]
        if lsb_first:
            chunk = chunk[::-1]
        words.append(int("".join(str(int(b)) for b in chunk), 2))
    return np.array(words, dtype=np.uint64).view(np.int64)


@functools.lru_cache(maxsize=None)
def expected(h, w, hs, name):
    """(int64 [3, W] rule hashes, status, literal hex strings) of fixture ``name`` of that size, computed once"""
    arr = dict(fixtures(h, w))[name]
    bits, status = rule_bits(arr, hs)
    words = np.stack([pack(bits[k]) for k in KINDS])
    words.setflags(write=False)
    return words, status, literal_hex(arr, hs)
