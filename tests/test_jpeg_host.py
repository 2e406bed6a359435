"""CPU: the host stage of the JPEG decode.  The probe on every fixture; the entropy stage's coefficients pushed through the
numpy restatement of the device arithmetic (tests/jpeg_helpers.py) equal the committed goldens, and this machine's Pillow over
the whole shape list when it reproduces the goldens; status codes of files outside the scope and of damaged files; a bad
file between good ones; the argument checks; and csrc/jpeg_host.cpp under the address and undefined-behaviour sanitizers,
as a stand-alone program over seeded mutations of the goldens.  Nothing here launches a kernel."""
import glob
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_helpers as jh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def jpeg():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    from mmr_amd import jpeg

    return jpeg


@pytest.fixture(scope="module")
def gold():
    return jh.golden()


def _rgb(host, i):
    return jh.restate(host.infos[i], host.blocks(i), host.qt[i])[1]


def _status(jpeg, data):
    return int(jpeg.entropy_decode([data]).status[0])


# ------------------------------------------------------------------ the probe

def test_the_golden_set_is_small_and_complete(gold):
    assert len(gold) == len(jh.GOLDEN_NAMES) >= 12
    files = glob.glob(os.path.join(jh.GOLDEN_DIR, "*"))
    assert sum(os.path.getsize(f) for f in files) < 128 << 10
    assert all(w.shape[0] <= 64 and w.shape[1] <= 64 and w.shape[2] == 3 and w.dtype == np.uint8 for _, _, w in gold)


def test_jpeg_info_on_every_fixture(jpeg, gold):
    sampling = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "grey": (1, 1)}
    for name, data, want in gold:
        info = jpeg.jpeg_info(data)
        assert info["status"] == 0 and info["status_name"] == "ok", name
        assert (info["H"], info["W"]) == want.shape[:2], name
        assert info["ncomp"] == (1 if "grey" in name else 3), name
        h, v = sampling[name.split("_")[1]]
        assert (info["hmax"], info["vmax"]) == (h, v), name
        mx, my = -(-info["W"] // (8 * h)), -(-info["H"] // (8 * v))
        assert (info["mcus_x"], info["mcus_y"]) == (mx, my), name
        blocks = (mx * my * h * v,) + ((mx * my, mx * my) if info["ncomp"] == 3 else ())
        assert info["blocks"] == blocks and info["coef_bytes"] == 128 * sum(blocks), name
    path = os.path.join(jh.GOLDEN_DIR, jh.GOLDEN_NAMES[0] + ".jpg")
    assert jpeg.jpeg_info(path) == jpeg.jpeg_info(gold[0][1])              # a path reads the same file


# ------------------------------------------------------------------ coefficients -> restatement -> Pillow's bytes

def test_coefficients_through_the_restatement_equal_the_goldens(jpeg, gold):
    host = jpeg.entropy_decode([d for _, d, _ in gold])
    assert host.status.tolist() == [0] * len(gold)
    for i, (name, _, want) in enumerate(gold):
        got = _rgb(host, i)
        assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))


def test_coefficients_through_the_restatement_equal_live_pillow_over_the_shape_list(jpeg):
    if not jh.live_pillow_reproduces_golden():
        pytest.skip("this machine's Pillow does not decode the golden files to the golden pixels: only the live comparison is skipped")
    cases = jh.SHAPE_LIST + [jh.LARGE]
    datas = [jh.build(c) for c in cases]
    host = jpeg.entropy_decode(datas)
    assert not host.status.any()
    for i, c in enumerate(cases):
        want = jh.pillow_rgb(datas[i])
        got = _rgb(host, i)
        assert got.shape == want.shape and np.array_equal(got, want), (c["name"], int((got != want).sum()))


def test_thread_counts_give_the_same_coefficients(jpeg, gold):
    datas = [d for _, d, _ in gold] * 3
    a, b = jpeg.entropy_decode(datas, threads=1), jpeg.entropy_decode(datas, threads=16)
    n = a.coef_bytes // 2
    assert n == b.coef_bytes // 2 and np.array_equal(a.coef[:n], b.coef[:n]) and np.array_equal(a.qt, b.qt)
    assert np.array_equal(a.status, b.status) and np.array_equal(a.coef_off, b.coef_off)


def _segment(data, marker):
    """offset of the first `FF marker` in the headers"""
    at = data.index(bytes([0xFF, marker]))
    return at


def test_comments_fill_bytes_and_trailing_bytes_change_nothing(jpeg, gold):
    name, data, want = gold[8]
    dqt = _segment(data, 0xDB)
    sos = _segment(data, 0xDA)
    edited = (data[:dqt] + b"\xff\xfe\x00\x07hello" + b"\xff\xec\x00\x04ab" + data[dqt:sos] + b"\xff\xff\xff" + data[sos:]
              + b"trailing bytes after EOI\xff\xd9\x00")
    host = jpeg.entropy_decode([data, edited])
    assert host.status.tolist() == [0, 0]
    assert np.array_equal(_rgb(host, 1), want)


# ------------------------------------------------------------------ status codes

def _saved(px, **kw):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(px).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_files_outside_the_scope_are_unsupported(jpeg):
    from PIL import Image

    px = jh.pixels(24, 40, "smooth", 3)
    assert _status(jpeg, _saved(px, quality=85, progressive=True)) == jpeg.JPEG_UNSUPPORTED
    buf = io.BytesIO()
    Image.fromarray(px).convert("CMYK").save(buf, "JPEG", quality=85)
    assert _status(jpeg, buf.getvalue()) == jpeg.JPEG_UNSUPPORTED
    assert jpeg.jpeg_info(buf.getvalue())["status_name"] == "unsupported"
    base = _saved(px, quality=85, subsampling="4:4:4")
    sof = _segment(base, 0xC0)
    twelve = bytearray(base)
    twelve[sof + 4] = 12                                     # sample precision
    assert _status(jpeg, bytes(twelve)) == jpeg.JPEG_UNSUPPORTED
    odd = bytearray(base)
    odd[sof + 11] = 0x12                                     # luma sampling 1 x 2
    assert _status(jpeg, bytes(odd)) == jpeg.JPEG_UNSUPPORTED
    zero = bytearray(base)
    zero[sof + 5: sof + 7] = b"\x00\x00"                     # height 0 (what a DNL file carries)
    assert _status(jpeg, bytes(zero)) == jpeg.JPEG_UNSUPPORTED
    assert _status(jpeg, base) == 0


def test_truncation_at_several_offsets_is_corrupt(jpeg, gold):
    name, data, _ = gold[8]
    sos = _segment(data, 0xDA)
    for cut in (0, 1, 2, 3, 20, sos // 2, sos + 3, sos + 14, (sos + len(data)) // 2, len(data) - 40, len(data) - 2, len(data) - 1):
        assert _status(jpeg, data[:cut]) == jpeg.JPEG_CORRUPT, cut
    assert _status(jpeg, b"") == jpeg.JPEG_CORRUPT
    assert jpeg.jpeg_info(b"")["status"] == jpeg.JPEG_CORRUPT


def test_a_flipped_byte_in_a_huffman_table_or_in_the_scan_is_corrupt(jpeg, gold):
    name, data, _ = gold[8]
    dht = _segment(data, 0xC4)
    bad = bytearray(data)
    bad[dht + 5] ^= 0xFF                                     # the count of 1-bit codes: 0 -> 255, no prefix code has that many
    assert _status(jpeg, bytes(bad)) == jpeg.JPEG_CORRUPT
    bad = bytearray(data)
    bad[dht + 2: dht + 4] = b"\xff\xf0"                      # a segment length past the end of the file
    assert _status(jpeg, bytes(bad)) == jpeg.JPEG_CORRUPT
    sos = _segment(data, 0xDA)
    at = next(i for i in range(sos + 20, len(data) - 8) if data[i] != 0xFF and data[i + 1] not in (0x00, 0xFF) and data[i - 1] != 0xFF)
    bad = bytearray(data)
    bad[at] = 0xFF                                           # the scan now ends early, at a marker that is no restart
    assert _status(jpeg, bytes(bad)) == jpeg.JPEG_CORRUPT
    rst = next(d for n, d, _ in gold if "rst" in n)
    at = rst.index(b"\xff\xd0", _segment(rst, 0xDA))
    bad = bytearray(rst)
    bad[at + 1] = 0xD3                                       # a wrong restart marker
    assert _status(jpeg, bytes(bad)) == jpeg.JPEG_CORRUPT
    assert _status(jpeg, rst) == 0
    assert _status(jpeg, data[:dht] + data[sos:]) == jpeg.JPEG_CORRUPT      # the Huffman tables dropped: a missing table


def test_a_bad_file_between_good_ones_leaves_them_correct(jpeg, gold):
    bad = gold[8][1][: len(gold[8][1]) // 2]
    progressive = _saved(jh.pixels(24, 40, "smooth", 3), progressive=True)
    datas = [gold[7][1], bad, gold[9][1], progressive, b"not a jpeg", gold[12][1]]
    host = jpeg.entropy_decode(datas, threads=3)
    assert host.status.tolist() == [0, 2, 0, 1, 2, 0]
    for i, g in ((0, 7), (2, 9), (5, 12)):
        assert np.array_equal(_rgb(host, i), gold[g][2])


# ------------------------------------------------------------------ argument checks (none reaches a device)

def test_argument_checks_run_before_anything_else(jpeg, gold, monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("an argument check came after device work")

    monkeypatch.setattr(jpeg, "JpegPlan", no_device)
    monkeypatch.setattr(jpeg, "entropy_decode", no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    data = gold[0][1]
    for call in (jpeg.decode_jpeg, jpeg.decode_jpeg_batches):
        arg = [data] if call is jpeg.decode_jpeg else [[data]]
        with pytest.raises(ValueError, match="on_unsupported"):
            call(arg, on_unsupported="skip")
        for threads in (0, 17, True, 2.0):
            with pytest.raises(ValueError, match="threads"):
                call(arg, threads=threads)
        with pytest.raises(RuntimeError, match="GPU"):
            call(arg, device="cpu")
    with pytest.raises(ValueError, match="list"):
        jpeg.decode_jpeg(data)
    with pytest.raises(ValueError, match="list"):
        jpeg.decode_jpeg("some/path.jpg")
    with pytest.raises(ValueError, match="empty"):
        jpeg.decode_jpeg([])
    with pytest.raises(ValueError, match=r"files\[1\]"):
        jpeg.decode_jpeg([data, 7])
    with pytest.raises(ValueError, match="iterable"):
        jpeg.decode_jpeg_batches(data)
    with pytest.raises(ValueError, match="bytes or a path"):
        jpeg.jpeg_info(7)


def test_the_library_checks_its_own_arguments(jpeg, gold):
    import ctypes

    from mmr_amd import _lib

    L = _lib.lib()
    data = gold[0][1]
    info = np.zeros(1, dtype=_lib.struct_dtype("mmr_jpeg_info"))
    assert L.mmr_jpeg_probe(data, len(data), info.ctypes.data) == 0
    coef = np.zeros(int(info[0]["coef_bytes"]) // 2 + 8, dtype=np.int16)
    qt, status = np.zeros(192, dtype=np.uint16), np.zeros(1, dtype=np.int32)
    ptrs, sizes = (ctypes.c_char_p * 1)(data), np.array([len(data)], dtype=np.int64)

    def call(off, threads):
        o = np.array([off], dtype=np.int64)
        return L.mmr_jpeg_entropy_decode(ptrs, sizes.ctypes.data, 1, info.ctypes.data, coef.ctypes.data, o.ctypes.data, qt.ctypes.data,
                                         status.ctypes.data, threads)

    assert call(0, 1) == 0 and status[0] == 0
    for threads in (0, 17, -1):
        assert call(0, threads) == -22 and b"threads" in L.mmr_last_error()
    assert call(2, 1) == -22 and b"multiple of 16" in L.mmr_last_error()
    assert call(-16, 1) == -22
    assert L.mmr_jpeg_entropy_decode(None, None, 1, None, None, None, None, None, 1) == -22
    # the device entry points refuse bad descriptors on the host, before any launch
    assert L.mmr_jpeg_workspace_bytes(None, 1) == 0 and b"null" in L.mmr_last_error()
    desc = np.zeros(2, dtype=_lib.struct_dtype("mmr_jpeg_desc"))
    assert L.mmr_jpeg_workspace_bytes(desc.ctypes.data, 2) == 16          # two rows without blocks
    desc[0]["W"], desc[0]["H"], desc[0]["ncomp"], desc[0]["hmax"], desc[0]["vmax"] = 17, 9, 3, 2, 2
    desc[0]["mcus_x"], desc[0]["mcus_y"], desc[0]["out"] = 2, 1, 4096
    desc[1]["block_first"], desc[1]["run_first"] = 12, 39
    assert L.mmr_jpeg_workspace_bytes(desc.ctypes.data, 2) == 12 * 64
    desc[1]["block_first"] = 11
    assert L.mmr_jpeg_workspace_bytes(desc.ctypes.data, 2) == 0 and b"prefix" in L.mmr_last_error()
    desc[1]["block_first"], desc[0]["vmax"] = 12, 3
    assert L.mmr_jpeg_workspace_bytes(desc.ctypes.data, 2) == 0
    desc[0]["vmax"], desc[0]["out"] = 2, 4097
    assert L.mmr_jpeg_workspace_bytes(desc.ctypes.data, 2) == 0 and b"aligned" in L.mmr_last_error()
    assert L.mmr_jpeg_decode_device(None, 1, None, None, None, 0, None) == -22
    assert L.mmr_jpeg_decode_device(None, 0, None, None, None, 0, None) == 0
    assert L.mmr_version() == 1


# ------------------------------------------------------------------ the host stage under the sanitizers

def test_the_host_stage_is_clean_under_the_sanitizers(tmp_path):
    src = os.path.join(ROOT, "multi-modal-retrieval-system-image-search-and-data-governance_amd", "csrc", "jpeg_host.cpp")
    exe = jh.build_sanitized(tmp_path, [src, os.path.join(ROOT, "tests", "jpeg_fuzz_main.cpp")], "jpeg_fuzz")
    if exe is None:
        pytest.skip("no C++ compiler on this machine")
    files = sorted(glob.glob(os.path.join(jh.GOLDEN_DIR, "*.jpg")))
    run = subprocess.run([exe] + files + ["--seeds", "1", "2", "3"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "decoded" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
