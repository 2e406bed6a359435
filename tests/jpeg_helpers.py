"""Shared by the JPEG decode tests: the numpy restatement of libjpeg's integer decode from coefficients to RGB
("JPEG decode"), the builder of the Pillow-written test files, the golden set under tests/golden/jpeg/, and
the sanitizer build of the stand-alone programs that every JPEG host test runs.

    python tests/jpeg_helpers.py        # rewrites tests/golden/jpeg/ from the seeded builder and this machine's Pillow
"""
import io
import json
import os
import shutil
import subprocess

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")


def build_sanitized(tmp_path, sources, exe, include=()):
    """A stand-alone program under the address and undefined-behaviour sanitizers: compiles ``sources`` (paths; one of them
    has the main) with the include directories ``include`` into ``tmp_path / exe`` and returns that path, or None on a
    machine without a C++ compiler."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        return None
    out = os.path.join(str(tmp_path), exe)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-static-libubsan", "-pthread"] + [a for d in include for a in ("-I", d)] + list(sources) + ["-o", out], check=True)
    return out


# ------------------------------------------------------------------------------------------------ the arithmetic

F0_298, F0_390, F0_541, F0_765, F0_899, F1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F1_501, F1_847, F1_961, F2_053, F2_562, F3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _fix(v):
    return int(v * 65536 + 0.5)


def idct_pass(x, s):
    """One 8-point pass of jidctint on int64 arrays x[0..7] (any common shape), descale shift s."""
    x0, x1, x2, x3, x4, x5, x6, x7 = x
    z1 = (x2 + x6) * F0_541
    t2 = z1 - x6 * F1_847
    t3 = z1 + x2 * F0_765
    t0 = (x0 + x4) << 13
    t1 = (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x7, x5, x3, x1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * F1_175
    a0, a1, a2, a3 = a0 * F0_298, a1 * F2_053, a2 * F3_072, a3 * F1_501
    z1, z2 = z1 * -F0_899, z2 * -F2_562
    z3 = z3 * -F1_961 + z5
    z4 = z4 * -F0_390 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    r = 1 << (s - 1)
    return [(v + r) >> s for v in (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)]


def idct_blocks(coef, q):
    """int16 [n, 64] natural-order coefficients, uint16 [64] table -> uint8 [n, 8, 8] samples: columns first, then rows."""
    x = coef.astype(np.int64).reshape(-1, 8, 8) * q.astype(np.int64).reshape(1, 8, 8)
    cols = np.stack(idct_pass([x[:, k, :] for k in range(8)], 11), axis=1)          # [n, 8 rows, 8 cols]
    rows = np.stack(idct_pass([cols[:, :, k] for k in range(8)], 18), axis=2)
    return np.clip(rows + 128, 0, 255).astype(np.uint8)


def plane_of(blocks, grid_h, grid_w):
    """uint8 [grid_h * grid_w, 8, 8] in raster order -> the padded plane [grid_h * 8, grid_w * 8]"""
    return blocks.reshape(grid_h, grid_w, 8, 8).transpose(0, 2, 1, 3).reshape(grid_h * 8, grid_w * 8)


def upsample_h2v1(p):
    dh, dw = p.shape
    p = p.astype(np.int64)
    out = np.empty((dh, 2 * dw), dtype=np.int64)
    if dw <= 2:
        out[:, 0::2] = p
        out[:, 1::2] = p
        return out
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0] = p[:, 0]
    out[:, -1] = p[:, -1]
    return out


def upsample_h2v2(p):
    dh, dw = p.shape
    p = p.astype(np.int64)
    if dw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * dh, 2 * dw), dtype=np.int64)
    for parity, other in ((0, up), (1, down)):
        s = 3 * p + other
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[parity::2, 0::2] = (3 * s + left + 8) >> 4
        out[parity::2, 1::2] = (3 * s + right + 7) >> 4
    return out


def color(Y, Cb, Cr):
    Y, cb, cr = Y.astype(np.int64), Cb.astype(np.int64) - 128, Cr.astype(np.int64) - 128
    R = Y + ((_fix(1.40200) * cr + 32768) >> 16)
    G = Y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    B = Y + ((_fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=-1), 0, 255).astype(np.uint8)


def restate(info, blocks, qt):
    """``info``: the probe's record (W, H, ncomp, hmax, vmax, mcus_x, mcus_y); ``blocks``: one int16 [n_c, 64] per component;
    ``qt`` uint16 [3, 64].  -> (padded uint8 planes, RGB uint8 [H, W, 3])."""
    W, H, nc = int(info["W"]), int(info["H"]), int(info["ncomp"])
    hmax, vmax, mx, my = int(info["hmax"]), int(info["vmax"]), int(info["mcus_x"]), int(info["mcus_y"])
    planes = []
    for c in range(nc):
        h, v = (hmax, vmax) if c == 0 else (1, 1)
        planes.append(plane_of(idct_blocks(blocks[c], qt[c]), my * v, mx * h))
    Y = planes[0][:H, :W]
    if nc == 1:
        return planes, np.repeat(Y[:, :, None], 3, axis=2)
    dh, dw = -(-H // vmax), -(-W // hmax)
    ch = []
    for p in planes[1:]:
        p = p[:dh, :dw]
        if (hmax, vmax) == (2, 1):
            p = upsample_h2v1(p)
        elif (hmax, vmax) == (2, 2):
            p = upsample_h2v2(p)
        ch.append(np.asarray(p)[:H, :W])
    return planes, color(Y, ch[0], ch[1])


# ------------------------------------------------------------------------------------------------ the test files

def pixels(h, w, content, seed, grey=False):
    """Seeded uint8 [h, w, 3] (or [h, w]): noise, or smooth = a small noise image resized up bicubically."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    shape = (h, w) if grey else (h, w, 3)
    if content == "noise":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    sh, sw = h // 8 + 2, w // 8 + 2
    small = rng.integers(0, 256, size=(sh, sw) if grey else (sh, sw, 3), dtype=np.uint8)
    return np.asarray(Image.fromarray(small).resize((w, h), Image.BICUBIC))


def write_jpeg(px, **save):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(px).save(buf, "JPEG", **save)
    return buf.getvalue()


def pillow_rgb(data):
    from PIL import Image

    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


def _case(name, h, w, sub=None, content="noise", quality=85, grey=False, **save):
    if sub is not None:
        save["subsampling"] = sub
    return dict(name=name, h=h, w=w, content=content, grey=grey, save=dict(quality=quality, **save))


# the smallest shapes at which each piece can go wrong (H x W)
SHAPE_LIST = (
    [_case(f"1x1_{s.replace(':', '')}", 1, 1, s) for s in ("4:4:4", "4:2:2", "4:2:0")] + [_case("1x1_grey", 1, 1, grey=True)]
    + [_case(f"9x{w}_{s.replace(':', '')}", 9, w, s) for w in (2, 3, 4) for s in ("4:2:0", "4:2:2")]
    + [_case("2x9_420", 2, 9, "4:2:0"), _case("5x1_420", 5, 1, "4:2:0"), _case("1x5_420", 1, 5, "4:2:0")]
    + [_case(f"{h}x{w}_{s.replace(':', '')}_{c}", h, w, s, c) for (h, w) in ((17, 33), (37, 51)) for s in ("4:4:4", "4:2:2", "4:2:0")
       for c in ("noise", "smooth")]
    + [_case("48x64_420", 48, 64, "4:2:0", "smooth"), _case("48x64_444", 48, 64, "4:4:4"), _case("48x64_422", 48, 64, "4:2:2")]
    + [_case("15x16_420", 15, 16, "4:2:0"), _case("16x15_420", 16, 15, "4:2:0"), _case("16x15_422", 16, 15, "4:2:2")]
    + [_case("17x33_grey", 17, 33, grey=True), _case("33x17_grey_smooth", 33, 17, content="smooth", grey=True)]
    + [_case("37x51_420_rst1", 37, 51, "4:2:0", restart_marker_blocks=1), _case("37x51_420_rst3", 37, 51, "4:2:0", "smooth", restart_marker_blocks=3),
       _case("17x33_444_rst2", 17, 33, "4:4:4", restart_marker_blocks=2), _case("17x33_grey_rst1", 17, 33, grey=True, restart_marker_blocks=1)]
    + [_case("37x51_420_opt", 37, 51, "4:2:0", optimize=True), _case("17x33_422_opt_smooth", 17, 33, "4:2:2", "smooth", optimize=True)]
    + [_case("17x33_444_q100", 17, 33, "4:4:4", quality=100), _case("37x51_420_q100", 37, 51, "4:2:0", quality=100)]
    + [_case("37x51_420_q5", 37, 51, "4:2:0", quality=5), _case("17x33_444_q5", 17, 33, "4:4:4", quality=5)]
)
LARGE = _case("480x640_420_smooth", 480, 640, "4:2:0", "smooth")
GOLDEN_NAMES = ("1x1_420", "1x1_grey", "9x2_420", "9x3_422", "9x4_420", "5x1_420", "1x5_420", "17x33_422_noise", "37x51_420_smooth",
                "48x64_444", "16x15_420", "17x33_grey", "37x51_420_rst3", "37x51_420_opt", "17x33_444_q100", "37x51_420_q5")


def build(case, seed=None):
    """The Pillow-written bytes of one case; the seed is the case's position in the list unless given."""
    if seed is None:
        seed = 1000 + [c["name"] for c in SHAPE_LIST + [LARGE]].index(case["name"])
    return write_jpeg(pixels(case["h"], case["w"], case["content"], seed, case["grey"]), **case["save"])


def golden():
    """[(name, file bytes, Pillow's RGB uint8 [H, W, 3])] as committed under tests/golden/jpeg/"""
    with np.load(os.path.join(GOLDEN_DIR, "decoded.npz")) as z:
        out = []
        for name in GOLDEN_NAMES:
            with open(os.path.join(GOLDEN_DIR, name + ".jpg"), "rb") as f:
                out.append((name, f.read(), z[name]))
    return out


_live = None


def live_pillow_reproduces_golden():
    """Whether this machine's Pillow decodes the golden files to the golden pixels (another libjpeg may not)."""
    global _live
    if _live is None:
        _live = all(np.array_equal(pillow_rgb(data), want) for _, data, want in golden())
    return _live


def write_golden():
    import PIL

    os.makedirs(GOLDEN_DIR, exist_ok=True)
    by_name = {c["name"]: c for c in SHAPE_LIST}
    decoded = {}
    for name in GOLDEN_NAMES:
        data = build(by_name[name])
        with open(os.path.join(GOLDEN_DIR, name + ".jpg"), "wb") as f:
            f.write(data)
        decoded[name] = pillow_rgb(data)
    np.savez_compressed(os.path.join(GOLDEN_DIR, "decoded.npz"), **decoded)
    with open(os.path.join(GOLDEN_DIR, "provenance.json"), "w") as f:
        json.dump({"pillow": PIL.__version__, "files": list(GOLDEN_NAMES)}, f, indent=1)


if __name__ == "__main__":
    write_golden()
