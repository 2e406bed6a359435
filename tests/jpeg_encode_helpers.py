"""Shared by the JPEG encode tests: the numpy restatement of libjpeg's integer forward path from pixels to quantised
coefficients ("JPEG encode"), the shape list, the Pillow writer, and the golden set under
tests/golden/jpeg_encode/.

    python tests/jpeg_encode_helpers.py        # rewrites tests/golden/jpeg_encode/ from the seeded builder and this machine's Pillow
"""
import io
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode")
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}

# ITU-T T.81 Annex K.1, natural order
STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
                     103, 99], dtype=np.int64)
STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                      + [99] * 32, dtype=np.int64)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ------------------------------------------------------------------------------------------------ the arithmetic


def quant_tables(quality):
    """(luma, chroma) uint16 [64] in natural order: libjpeg's jpeg_quality_scaling of the Annex K tables"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((std * s + 50) // 100, 1, 255).astype(np.uint16) for std in (STD_LUMA, STD_CHROMA))


def composite(rgba, background=(255, 255, 255)):
    """uint8 [H, W, 4] over a colour, as Image.paste(img, mask=alpha) does it"""
    c, a = rgba[:, :, :3].astype(np.int64), rgba[:, :, 3:4].astype(np.int64)
    t = c * a + np.array(background, dtype=np.int64).reshape(1, 1, 3) * (255 - a) + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def ycc(rgb):
    R, G, B = (rgb[:, :, k].astype(np.int64) for k in range(3))
    return [(19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
            (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16,
            (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16]


def _pad(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def geometry(H, W, hmax, vmax):
    """(mcus_x, mcus_y)"""
    return -(-W // (8 * hmax)), -(-H // (8 * vmax))


def planes(px, subsampling="4:2:0", background=(255, 255, 255)):
    """uint8 [H, W] / [H, W, 3] / [H, W, 4] -> the padded uint8 component planes libjpeg hands to its forward DCT"""
    if px.ndim == 2:
        mx, my = geometry(px.shape[0], px.shape[1], 1, 1)
        return [_pad(px.astype(np.int64), my * 8, mx * 8).astype(np.uint8)]
    if px.shape[2] == 4:
        px = composite(px, background)
    H, W = px.shape[:2]
    hmax, vmax = SAMPLING[subsampling]
    mx, my = geometry(H, W, hmax, vmax)
    full = [_pad(c, -(-H // vmax) * vmax, mx * 8 * hmax) for c in ycc(px)]      # columns to the MCU, rows to a multiple of vmax only
    out = [_pad(full[0], my * 8 * vmax, mx * 8 * hmax)]
    for c in full[1:]:
        if (hmax, vmax) == (2, 1):
            bias = (np.arange(c.shape[1] // 2) & 1).reshape(1, -1)
            c = (c[:, 0::2] + c[:, 1::2] + bias) >> 1
        elif (hmax, vmax) == (2, 2):
            bias = (1 + (np.arange(c.shape[1] // 2) & 1)).reshape(1, -1)
            c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(_pad(c, my * 8, mx * 8))                                       # then the downsampled rows repeat
    return [p.astype(np.uint8) for p in out]


def _descale(v, n):
    return (v + (1 << (n - 1))) >> n


def fdct_pass(x, first):
    """One 8-point pass of jfdctint on int64 arrays x[0..7]: the row pass (first) or the column pass."""
    x0, x1, x2, x3, x4, x5, x6, x7 = x
    t0, t7, t1, t6, t2, t5, t3, t4 = x0 + x7, x0 - x7, x1 + x6, x1 - x6, x2 + x5, x2 - x5, x3 + x4, x3 - x4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o0, o4 = ((t10 + t11) << 2, (t10 - t11) << 2) if first else (_descale(t10 + t11, 2), _descale(t10 - t11, 2))
    z1 = (t12 + t13) * 4433
    o2, o6 = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    return [o0, _descale(t7 + z1 + z4, n), o2, _descale(t6 + z2 + z3, n), o4, _descale(t5 + z2 + z4, n), o6, _descale(t4 + z1 + z3, n)]


def fdct_quant(plane, q):
    """uint8 plane [h8, w8], uint16 [64] table -> int16 [blocks, 64] in raster order over the block grid, natural order"""
    gh, gw = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.astype(np.int64).reshape(gh, 8, gw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8) - 128
    rows = np.stack(fdct_pass([x[:, :, k] for k in range(8)], True), axis=2)
    cols = np.stack(fdct_pass([rows[:, k, :] for k in range(8)], False), axis=1)
    d = 8 * q.astype(np.int64).reshape(1, 8, 8)
    m = (np.abs(cols) + (d >> 1)) // d
    return (np.sign(cols) * m).astype(np.int16).reshape(-1, 64)


def coefficients(pl, qts, H, W, hmax, vmax):
    """padded planes -> one int16 [blocks_c, 64] per component, the luma dummy blocks filled by libjpeg's rule"""
    out = [fdct_quant(p, qts[0 if c == 0 else 1]) for c, p in enumerate(pl)]
    if len(pl) == 3:
        gw = pl[0].shape[1] // 8
        real_w, real_h = -(-W // 8), -(-H // 8)
        Y = out[0]
        for my in range(pl[0].shape[0] // (8 * vmax)):
            for mx in range(gw // hmax):
                prev = None
                for iy in range(vmax):
                    for ix in range(hmax):
                        by, bx = my * vmax + iy, mx * hmax + ix
                        if bx >= real_w or by >= real_h:
                            Y[by * gw + bx] = 0
                            Y[by * gw + bx, 0] = prev
                        prev = Y[by * gw + bx, 0]
    return out


def restate(px, quality=95, subsampling="4:2:0", background=(255, 255, 255)):
    """-> (padded planes, [int16 [blocks_c, 64]], (qt_luma, qt_chroma), (hmax, vmax))"""
    hmax, vmax = (1, 1) if px.ndim == 2 else SAMPLING[subsampling]
    pl = planes(px, subsampling, background)
    qts = quant_tables(quality)
    return pl, coefficients(pl, qts, px.shape[0], px.shape[1], hmax, vmax), qts, (hmax, vmax)


# ------------------------------------------------------------------------------------------------ the cases

def pixels(h, w, content, seed, channels=3):
    """Seeded uint8 [h, w, channels] ([h, w] for channels = 1): noise, or a smooth ramp with a little noise on it."""
    rng = np.random.default_rng(seed)
    shape = (h, w) if channels == 1 else (h, w, channels)
    if content == "noise":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = (yy * 3 + xx * 5)[:, :, None] * np.array([1, 2, 3, 1])[None, None, :channels] + rng.integers(0, 4, size=(h, w, channels))
    return (ramp.reshape(shape) % 256).astype(np.uint8)


def write_jpeg(px, quality=95, subsampling="4:2:0", restart=0, background=None):
    """The yardstick: Pillow's bytes.  RGBA goes over the background first, as tool/Image format conversion.py:49-53 does."""
    from PIL import Image

    im = Image.fromarray(px)
    if px.ndim == 3 and px.shape[2] == 4:
        bg = Image.new("RGB", im.size, tuple(background or (255, 255, 255)))
        bg.paste(im, mask=im.split()[3])
        im = bg
    kw = dict(quality=quality)
    if px.ndim == 3:
        kw["subsampling"] = subsampling
    if restart:
        kw["restart_marker_blocks"] = restart
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def _case(h, w, sub="4:2:0", content="noise", quality=95, channels=3, restart=0, background=None):
    name = f"{h}x{w}_{'grey' if channels == 1 else sub.replace(':', '')}_{content}_q{quality}"
    name += (f"_rst{restart}" if restart else "") + ("_rgba" if channels == 4 else "") + ("_bg" if background else "")
    return dict(name=name, h=h, w=w, sub=sub, content=content, quality=quality, channels=channels, restart=restart, background=background)


_SIZES = ((1, 1), (8, 8), (9, 2), (9, 3), (5, 1), (1, 5), (16, 16), (17, 33), (24, 40), (37, 51), (100, 75))
SHAPE_LIST = (
    [_case(h, w, s, "noise") for (h, w) in _SIZES for s in SAMPLING]
    + [_case(h, w, s, "smooth") for (h, w) in ((8, 8), (17, 33), (24, 40), (37, 51)) for s in SAMPLING]
    + [_case(h, w, channels=1) for (h, w) in ((1, 1), (9, 3), (17, 33), (37, 51))]
    + [_case(h, w, s, quality=q) for (h, w) in ((17, 33), (24, 40)) for s in ("4:2:0", "4:4:4") for q in (100, 5, 75, 30)]
    + [_case(37, 51, "4:2:0", restart=3), _case(37, 51, "4:2:2", restart=1), _case(17, 33, "4:4:4", restart=2), _case(37, 51, channels=1, restart=9)]
    + [_case(24, 40, "4:2:0", channels=4), _case(17, 33, "4:4:4", channels=4, background=(10, 200, 77)), _case(9, 3, "4:2:2", channels=4)]
)
LARGE = _case(480, 640, "4:2:0", "smooth")
GOLDEN_NAMES = (
    "1x1_420_noise_q95", "1x1_444_noise_q95", "8x8_420_noise_q95", "8x8_444_noise_q95", "9x2_420_noise_q95", "9x2_422_noise_q95",
    "9x3_420_noise_q95", "9x3_422_noise_q95", "5x1_420_noise_q95", "1x5_420_noise_q95", "16x16_420_noise_q95", "16x16_422_noise_q95",
    "17x33_420_noise_q95", "17x33_422_noise_q95", "17x33_444_noise_q95", "24x40_420_noise_q95", "24x40_444_noise_q95", "37x51_420_noise_q95",
    "37x51_422_noise_q95", "37x51_420_smooth_q95", "1x1_grey_noise_q95", "17x33_grey_noise_q95", "37x51_grey_noise_q95",
    "17x33_420_noise_q100", "24x40_444_noise_q100", "17x33_420_noise_q5", "24x40_444_noise_q5", "8x8_422_noise_q95", "24x40_422_noise_q95", "9x3_444_noise_q95", "37x51_420_noise_q95_rst3",
    "24x40_420_noise_q95_rgba", "17x33_444_noise_q95_rgba_bg")


def case_pixels(case, seed=None):
    if seed is None:
        seed = 2000 + [c["name"] for c in SHAPE_LIST + [LARGE]].index(case["name"])
    return pixels(case["h"], case["w"], case["content"], seed, case["channels"])


def case_options(case):
    """the keyword arguments of encode_jpeg (and of write_jpeg, which calls restart_interval `restart`) for a case"""
    kw = dict(quality=case["quality"], subsampling=case["sub"])
    if case["background"]:
        kw["background"] = case["background"]
    return kw


def build(case, px=None):
    """The Pillow-written bytes of one case."""
    px = case_pixels(case) if px is None else px
    return write_jpeg(px, case["quality"], case["sub"], case["restart"], case["background"])


def golden():
    """[(case, source pixels, Pillow's bytes)] as committed under tests/golden/jpeg_encode/"""
    by_name = {c["name"]: c for c in SHAPE_LIST}
    out = []
    with np.load(os.path.join(GOLDEN_DIR, "pixels.npz")) as z:
        for name in GOLDEN_NAMES:
            with open(os.path.join(GOLDEN_DIR, name + ".jpg"), "rb") as f:
                out.append((by_name[name], z[name], f.read()))
    return out


def golden_composited():
    """uint8 [H, W, 3] per RGBA golden: what Pillow's paste over the background gave"""
    with np.load(os.path.join(GOLDEN_DIR, "composited.npz")) as z:
        return {k: z[k] for k in z.files}


_live = None


def live_pillow_reproduces_golden():
    """Whether this machine's Pillow writes the golden bytes from the golden pixels (another libjpeg may not)."""
    global _live
    if _live is None:
        _live = all(build(case, px) == data for case, px, data in golden())
    return _live


def scan_of(data):
    """the bytes of a file from its first entropy-coded byte on (a mismatch there is the arithmetic's, before it the framing's)"""
    at = data.index(b"\xff\xda")
    return data[at + 2 + ((data[at + 2] << 8) | data[at + 3]):]


def write_golden():
    import PIL
    from PIL import Image

    os.makedirs(GOLDEN_DIR, exist_ok=True)
    by_name = {c["name"]: c for c in SHAPE_LIST}
    px, comp = {}, {}
    for name in GOLDEN_NAMES:
        case = by_name[name]
        px[name] = case_pixels(case)
        with open(os.path.join(GOLDEN_DIR, name + ".jpg"), "wb") as f:
            f.write(build(case, px[name]))
        if case["channels"] == 4:
            im = Image.fromarray(px[name])
            bg = Image.new("RGB", im.size, tuple(case["background"] or (255, 255, 255)))
            bg.paste(im, mask=im.split()[3])
            comp[name] = np.asarray(bg)
    np.savez_compressed(os.path.join(GOLDEN_DIR, "pixels.npz"), **px)
    np.savez_compressed(os.path.join(GOLDEN_DIR, "composited.npz"), **comp)
    with open(os.path.join(GOLDEN_DIR, "provenance.json"), "w") as f:
        json.dump({"pillow": PIL.__version__, "written_by": "tests/jpeg_encode_helpers.py", "files": list(GOLDEN_NAMES)}, f, indent=1)


if __name__ == "__main__":
    write_golden()
