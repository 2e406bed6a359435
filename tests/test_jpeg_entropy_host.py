"""CPU: the device Huffman stage without a device.  The two fixtures still hold the subsequence-boundary cases they were
chosen for; mmr_jpeg_scan_prepare gives the probe's status and geometry and the documented descriptors; its argument checks
and those of the device entry points; and the kernel's logic, through the header it shares with the emulation program,
under the address and undefined-behaviour sanitizers: every golden, fixture and shape of the list equals the host stage, and
seeded mutations are accepted exactly when the host stage accepts them.  Nothing here launches a kernel."""
import ctypes
import glob
import io
import os
import re
import subprocess

import numpy as np
import pytest

import jpeg_entropy_helpers as eh
import jpeg_helpers as jh

MUTATION_SEEDS, MUTATIONS_PER_SEED = eh.MUTATION_SEEDS, eh.MUTATIONS_PER_SEED


@pytest.fixture(scope="module")
def jpeg():
    import __graft_entry__ as ge
    from mmr_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    from mmr_amd import jpeg

    return jpeg


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("jpeg_entropy_emul")
    exe = eh.build_emulation(tmp)
    if exe is None:
        pytest.skip("no C++ compiler on this machine")
    return exe, tmp


def _prepare(L, datas):
    from mmr_amd import _lib

    B = len(datas)
    infos = np.zeros(B, dtype=_lib.struct_dtype("mmr_jpeg_info"))
    desc = np.zeros(B, dtype=_lib.struct_dtype("mmr_jpeg_scan_desc"))
    tables = np.zeros((B, _lib.HEADER.constants["MMR_JPEG_TABLE_BYTES"]), dtype=np.uint8)
    qt, status = np.zeros((B, 3, 64), dtype=np.uint16), np.full(B, -1, dtype=np.int32)
    ptrs, sizes = (ctypes.c_char_p * B)(*datas), np.array([len(d) for d in datas], dtype=np.int64)
    rc = L.mmr_jpeg_scan_prepare(ptrs, sizes.ctypes.data, B, infos.ctypes.data, desc.ctypes.data, tables.ctypes.data, qt.ctypes.data, status.ctypes.data)
    assert rc == 0
    return infos, desc, tables, qt, status


# ------------------------------------------------------------------ the fixtures

def test_the_fixtures_still_hold_their_boundary_cases():
    (n1, f1), (n2, f2) = eh.fixtures()
    assert (n1, n2) == tuple(eh.FIXTURES)
    a, b = eh.boundary_facts(f1), eh.boundary_facts(f2)
    assert a["markers"] == 63 and a["subsequences"] > 256, a
    for key in ("marker_ff_last", "marker_ff_first", "marker_ends", "stuffed_ff_last"):
        assert a[key] >= 1, (key, a)
    assert b["stuffed_ff_last"] >= 1 and b["stuffed_ff_first"] >= 1 and b["subsequences"] > 1024, b
    assert sum(os.path.getsize(f) for f in glob.glob(os.path.join(eh.FIXTURE_DIR, "*"))) < 64 << 10


def test_the_builder_reproduces_the_fixtures_with_the_pillow_that_wrote_them():
    import json

    import PIL

    with open(os.path.join(eh.FIXTURE_DIR, "provenance.json")) as f:
        prov = json.load(f)
    if PIL.__version__ != prov["pillow"]:
        pytest.skip("another Pillow wrote the fixtures: an encoder may place the bytes elsewhere, the committed files are the test")
    for name, data in eh.fixtures():
        assert eh.build_fixture(name) == data, name


# ------------------------------------------------------------------ mmr_jpeg_scan_prepare

def test_scan_prepare_gives_the_probe_and_the_documented_descriptors(jpeg):
    from mmr_amd import _lib

    L = _lib.lib()
    files = [(n, d) for n, d, _ in jh.golden()] + eh.fixtures()
    datas = [d for _, d in files]
    infos, desc, tables, qt, status = _prepare(L, datas)
    host = jpeg.entropy_decode(datas)
    assert status.tolist() == [0] * len(files) and np.array_equal(qt, host.qt)
    bytes_at = coef_at = 0
    for i, (name, data) in enumerate(files):
        want = np.zeros(1, dtype=infos.dtype)
        assert L.mmr_jpeg_probe(data, len(data), want.ctypes.data) == 0
        assert infos[i].tobytes() == want[0].tobytes(), name
        d = desc[i]
        start = eh.scan_start(data)
        assert (int(d["scan_start"]), int(d["scan_bytes"])) == (start, len(data) - start), name
        assert [int(d[k]) for k in ("ncomp", "hmax", "vmax", "mcus_x", "mcus_y", "blocks0", "blocks1", "blocks2")] == \
               [int(want[0][k]) for k in ("ncomp", "hmax", "vmax", "mcus_x", "mcus_y", "blocks0", "blocks1", "blocks2")], name
        assert int(d["restart"]) == (3 if "rst3" in name else 1 if "rst1" in name else 0), name
        assert (int(d["bytes_off"]), int(d["state_off"]), int(d["coef_off"])) == (bytes_at, bytes_at, coef_at), name
        assert int(d["tables_off"]) == i * tables.shape[1] and int(d["status"]) == 0
        slots = [int(d[k]) for k in ("td0", "td1", "td2", "ta0", "ta1", "ta2")]
        assert all(0 <= s < 6 for s in slots) and slots[0] != slots[3], (name, slots)
        if int(d["ncomp"]) == 3:
            assert slots[1] == slots[2] and slots[4] == slots[5] and slots[0] != slots[1], (name, slots)     # Pillow: chroma shares its tables
        assert tables[i].any()
        bytes_at += (len(data) - start + 15) // 16 * 16
        coef_at += int(want[0]["coef_bytes"])
    assert np.array_equal(desc["coef_off"], host.coef_off)


def test_unsupported_and_truncated_files_keep_their_host_status(jpeg):
    from PIL import Image

    from mmr_amd import _lib

    gold = jh.golden()
    buf = io.BytesIO()
    Image.fromarray(jh.pixels(24, 40, "smooth", 3)).save(buf, "JPEG", quality=85, progressive=True)
    sos = gold[8][1].index(b"\xff\xda")
    datas = [gold[7][1], buf.getvalue(), gold[8][1][: sos // 2], b"not a jpeg", b"", gold[8][1][: sos + 40], gold[9][1]]
    infos, desc, tables, qt, status = _prepare(_lib.lib(), datas)
    host = jpeg.entropy_decode(datas)
    assert status.tolist() == [0, jpeg.JPEG_UNSUPPORTED, jpeg.JPEG_CORRUPT, jpeg.JPEG_CORRUPT, jpeg.JPEG_CORRUPT, 0, 0]
    assert host.status.tolist() == [0, 1, 2, 2, 2, 2, 0]              # the file cut inside its scan: the probe passes, the decode does not
    assert np.array_equal(infos["status"], host.infos["status"])
    for i in (1, 2, 3, 4):
        assert int(desc[i]["ncomp"]) == 0 and int(desc[i]["scan_bytes"]) == 0 and int(desc[i]["status"]) == status[i]
        assert not tables[i].any() and not qt[i].any()
    assert int(desc[6]["bytes_off"]) == int(desc[5]["bytes_off"]) + (int(desc[5]["scan_bytes"]) + 15) // 16 * 16


def test_a_scan_over_the_cap_is_declined_on_the_host(jpeg):
    from mmr_amd import _lib

    cap = _lib.HEADER.constants["MMR_JPEG_DEVICE_MAX_SCAN"]
    assert _lib.HEADER.constants["MMR_JPEG_DECLINED"] == 3 == jpeg.JPEG_DECLINED and cap == 4 << 20
    data = jh.golden()[8][1]
    start = eh.scan_start(data)
    fits, over = data + bytes(cap - (len(data) - start)), data + bytes(cap - (len(data) - start) + 1)     # bytes behind EOI count
    infos, desc, tables, qt, status = _prepare(_lib.lib(), [fits, over])
    assert status.tolist() == [0, 3] and infos["status"].tolist() == [0, 0]
    assert int(desc[0]["scan_bytes"]) == cap and int(desc[1]["ncomp"]) == 0 and int(desc[1]["status"]) == 3
    assert qt[1].any()                                                # the host stage's tables are there for the arbiter


def test_argument_checks_answer_einval_with_a_message(jpeg):
    from mmr_amd import _lib

    L = _lib.lib()
    assert L.mmr_jpeg_scan_prepare(None, None, 1, None, None, None, None, None) == -22 and b"mmr_jpeg_scan_prepare" in L.mmr_last_error()
    assert L.mmr_jpeg_scan_prepare(None, None, -1, None, None, None, None, None) == -22
    assert L.mmr_jpeg_scan_prepare(None, None, 0, None, None, None, None, None) == 0
    for S in (0, 8, 24, 2048, -16):
        assert L.mmr_jpeg_entropy_decode_device(None, 1, None, None, None, None, S, 4, None, 0, None) == -22 and b"subseq_bytes" in L.mmr_last_error()
    for R in (0, 1025, -1):
        assert L.mmr_jpeg_entropy_decode_device(None, 1, None, None, None, None, 16, R, None, 0, None) == -22 and b"max_rounds" in L.mmr_last_error()
    assert L.mmr_jpeg_entropy_decode_device(None, 1, None, None, None, None, 16, 4, None, 0, None) == -22 and b"null" in L.mmr_last_error()
    assert L.mmr_jpeg_entropy_decode_device(None, 70000, None, None, None, None, 16, 4, None, 0, None) == -22
    assert L.mmr_jpeg_entropy_decode_device(None, 0, None, None, None, None, 16, 4, None, 0, None) == 0
    # the workspace query checks a host copy of the descriptors
    assert L.mmr_jpeg_entropy_workspace_bytes(None, 1, 16) == 0 and b"null" in L.mmr_last_error()
    infos, desc, tables, qt, status = _prepare(L, [d for _, d in eh.fixtures()])
    assert L.mmr_jpeg_entropy_workspace_bytes(desc.ctypes.data, 2, 24) == 0 and b"power of two" in L.mmr_last_error()
    assert L.mmr_jpeg_entropy_workspace_bytes(desc.ctypes.data, 2, 16) == 16          # fewer than 2048 subsequences each: states in LDS
    for field, value, word in (("coef_off", 8, b"multiples of 16"), ("bytes_off", -16, b"multiples of 16"), ("scan_bytes", (4 << 20) + 1, b"scan_bytes"),
                               ("hmax", 3, b"outside"), ("blocks1", 7, b"outside"), ("td1", 6, b"outside")):
        bad = desc.copy()
        bad[1][field] = value
        assert L.mmr_jpeg_entropy_workspace_bytes(bad.ctypes.data, 2, 16) == 0 and word in L.mmr_last_error(), field
    big = desc.copy()
    big[1]["scan_bytes"], big[1]["state_off"] = 16 * 2049, 4096                        # one subsequence too many for LDS
    assert L.mmr_jpeg_entropy_workspace_bytes(big.ctypes.data, 2, 16) == 4096 + 16 * 2049
    # the Python layer refuses before any device work
    for kw, word in ((dict(subseq_bytes=24), "subseq_bytes"), (dict(subseq_bytes=True), "subseq_bytes"), (dict(max_rounds=0), "max_rounds"),
                     (dict(max_rounds=2.0), "max_rounds")):
        with pytest.raises(ValueError, match=word):
            jpeg.entropy_decode_device([b"x"], device="cuda", **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        jpeg.entropy_decode_device([b"x"], device="cpu")
    for call, arg in ((jpeg.decode_jpeg, [b"x"]), (jpeg.decode_jpeg_batches, [[b"x"]])):
        with pytest.raises(ValueError, match="entropy"):
            call(arg, entropy="gpu")


def test_the_header_declares_the_new_symbols_and_the_library_exports_them(jpeg):
    from mmr_amd import _lib

    L = _lib.lib()
    for name in ("mmr_jpeg_scan_prepare", "mmr_jpeg_entropy_workspace_bytes", "mmr_jpeg_entropy_decode_device"):
        assert name in _lib.HEADER.functions and hasattr(L, name), name
    assert len(_lib.HEADER.functions["mmr_jpeg_entropy_decode_device"][1]) == 11
    dt = _lib.struct_dtype("mmr_jpeg_scan_desc")
    assert dt.itemsize == 112 and dt.names[:6] == ("scan_start", "scan_bytes", "bytes_off", "tables_off", "coef_off", "state_off")
    assert _lib.HEADER.constants["MMR_JPEG_TABLE_BYTES"] == 6 * 336 * 4
    assert jpeg.SUBSEQ_BYTES == 128 and jpeg.MAX_ROUNDS == 64


# ------------------------------------------------------------------ the kernel's logic under the sanitizers

def _run(exe, args, timeout=600):
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    return run.stdout


def test_the_emulation_equals_the_host_stage_on_every_good_file(emulation):
    exe, tmp = emulation
    files = sorted(glob.glob(os.path.join(jh.GOLDEN_DIR, "*.jpg"))) + [os.path.join(eh.FIXTURE_DIR, n + ".jpg") for n in eh.FIXTURES]
    assert len(files) == 18
    for case in jh.SHAPE_LIST:
        path = os.path.join(str(tmp), case["name"] + ".jpg")
        with open(path, "wb") as f:
            f.write(jh.build(case))
        files.append(path)
    out = _run(exe, ["--subseq", "16", "128", "--good"] + files)
    assert f"emulated {2 * len(files)} good files, 0 mutations (0 accepted, 0 declined), 0 failures" in out, out[-2000:]
    rounds = {(m.group(1), int(m.group(2))): (int(m.group(3)), int(m.group(4)))
              for m in re.finditer(r"^rounds (\S+)\.jpg S=(\d+) rounds=(\d+) subseq=(\d+)$", out, flags=re.M)}
    print({k: v for k, v in rounds.items() if k[0] in eh.FIXTURES})
    for name, data in eh.fixtures():
        r, n = rounds[(name, 16)]
        assert n == eh.subsequences(data, 16) and 2 <= r <= n, (name, r, n)
    # the GPU tests of the round cap rely on this: two rounds do not converge the second fixture
    assert rounds[("96x96_420_q100", 16)][0] >= 3 and rounds[("96x96_420_q100", 16)][1] > 1024
    # and on these: every file of the GPU coefficient test converges within the default cap at the default size
    assert all(r <= 64 for (name, S), (r, n) in rounds.items() if S == 128), rounds


def test_the_emulation_accepts_a_mutation_exactly_when_the_host_stage_does(emulation):
    exe, tmp = emulation
    muts = []
    for name, data in eh.mutation_sources():
        for seed in MUTATION_SEEDS:
            muts += eh.mutations(data, seed, MUTATIONS_PER_SEED)
    assert len(muts) == 2500
    pack = os.path.join(str(tmp), "mutations.pack")
    eh.write_pack(pack, muts)
    out = _run(exe, ["--subseq", "16", "--pack", pack])
    m = re.search(r"emulated 0 good files, 2500 mutations \((\d+) accepted, (\d+) declined\), 0 failures", out)
    assert m, out[-2000:]
    assert int(m.group(1)) >= 100 and int(m.group(2)) >= 100, out[-300:]              # both outcomes are exercised
