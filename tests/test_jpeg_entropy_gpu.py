"""GPU: the device Huffman stage against the host stage (exact int16 coefficients) and, through the two decode kernels,
against Pillow's bytes: coefficients at two subsequence sizes, the cap on the rounds, seeded mutations (the ones the CPU
emulation has passed under the sanitizers) with guard regions behind every coefficient span, decode_jpeg(entropy="device")
against entropy="host" including bad files, and graph capture of the entropy call with the decode kernels."""
import io

import numpy as np
import pytest
import torch

import jpeg_entropy_helpers as eh
import jpeg_helpers as jh

pytestmark = pytest.mark.gpu

DECLINED = 3


@pytest.fixture(scope="module")
def jpeg(device):
    from mmr_amd import jpeg

    return jpeg


@pytest.fixture(scope="module")
def good_files():
    """[(name, bytes)]: goldens, fixtures and the shape list, built once"""
    return [(n, d) for n, d, _ in jh.golden()] + eh.fixtures() + [(c["name"], jh.build(c)) for c in jh.SHAPE_LIST]


@pytest.fixture(scope="module")
def host_of_good(jpeg, good_files):
    return jpeg.entropy_decode([d for _, d in good_files])


def _equal_blocks(dev, host, row, name):
    got, want = dev.blocks(row), host.blocks(row)
    assert len(got) == len(want), name
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (name, "component", c, int((g != w).sum()))


# ------------------------------------------------------------------ 1. coefficients

@pytest.mark.parametrize("subseq", [16, None])
def test_coefficients_equal_the_host_stage(jpeg, device, good_files, host_of_good, subseq):
    # at 16 bytes the q100 noise files need hundreds of rounds (tests/test_jpeg_entropy_host.py prints them); the default cap
    # is for the default size, where the same test shows every one of these files within it
    dev = jpeg.entropy_decode_device([d for _, d in good_files], device, subseq_bytes=subseq, max_rounds=1024 if subseq else None)
    assert not host_of_good.status.any()
    S = subseq or jpeg.SUBSEQ_BYTES
    print({n: (int(r), int(k)) for (n, _), r, k in zip(good_files, dev.rounds, dev.subsequences)})
    assert dev.status.dtype == np.int32 and dev.status.tolist() == [0] * len(good_files)
    for i, (name, data) in enumerate(good_files):
        assert int(dev.subsequences[i]) == eh.subsequences(data, S), name
        assert int(dev.rounds[i]) >= (2 if eh.subsequences(data, S) > 1 else 1), name
        _equal_blocks(dev, host_of_good, i, name)


def test_coefficients_of_a_vga_file_with_more_subsequences_than_lanes(jpeg, device):
    data = jh.build(jh.LARGE)
    assert eh.subsequences(data, 128) > 256
    dev = jpeg.entropy_decode_device([data], device, subseq_bytes=128)
    host = jpeg.entropy_decode([data])
    print(int(dev.rounds[0]), int(dev.subsequences[0]))
    assert dev.status.tolist() == [0] and host.status.tolist() == [0] and int(dev.rounds[0]) >= 2
    _equal_blocks(dev, host, 0, "480x640")


# ------------------------------------------------------------------ 2. the cap on the rounds

def test_the_round_cap_declines_and_never_returns_wrong_coefficients(jpeg, device):
    files = eh.fixtures()
    datas = [d for _, d in files]
    host = jpeg.entropy_decode(datas)
    for cap in (1, 2):
        dev = jpeg.entropy_decode_device(datas, device, subseq_bytes=16, max_rounds=cap)
        assert dev.rounds.max() <= cap
        for i, (name, _) in enumerate(files):
            assert int(dev.status[i]) in (0, DECLINED), (name, cap)
            if dev.status[i] == 0:
                _equal_blocks(dev, host, i, name)
        assert int(dev.status[1]) == DECLINED, cap
    n = eh.subsequences(datas[1], 16)
    assert n > 1024
    dev = jpeg.entropy_decode_device(datas, device, subseq_bytes=16, max_rounds=min(n, 1024))
    assert dev.status.tolist() == [0, 0]
    _equal_blocks(dev, host, 1, files[1][0])


# ------------------------------------------------------------------ 3. mutations

def test_mutations_are_accepted_exactly_when_the_host_stage_accepts_them(jpeg, device):
    muts = []
    for name, data in eh.mutation_sources():
        muts += eh.mutations(data, eh.MUTATION_SEEDS[0], eh.MUTATIONS_PER_SEED)[:60]       # a prefix of what the emulation decoded
    assert len(muts) == 300
    good = jh.golden()[9][1]
    datas = [good] + muts + [good]
    host = jpeg.entropy_decode(datas)
    guard, fill = 256, 0x5A5A
    dev = jpeg.entropy_decode_device(datas, device, subseq_bytes=16, max_rounds=1024, guard=guard, fill=fill)
    status = dev.status
    assert set(status.tolist()) <= {0, 1, 2, DECLINED}
    accepted = 0
    for i in range(len(datas)):
        assert (status[i] == 0) == (host.status[i] == 0), (i, int(status[i]), int(host.status[i]))
        if host.infos[i]["status"] != 0:
            assert status[i] == host.status[i], i                     # what the probe refuses keeps the probe's status
        if status[i] == 0:
            _equal_blocks(dev, host, i, i)
            accepted += 1
    assert status[0] == 0 and status[-1] == 0 and 30 <= accepted <= 270, accepted      # untouched neighbours, both outcomes
    flat = dev.coef_dev.cpu().numpy()
    for i in np.flatnonzero(dev.ready):
        end = (int(dev.coef_off[i]) + int(dev.infos[i]["coef_bytes"])) // 2
        assert (flat[end: end + guard // 2] == fill).all(), i
    assert (flat[dev.coef_bytes // 2:] == fill).all()


# ------------------------------------------------------------------ 4. end to end

def _bad_batch():
    from PIL import Image

    gold = jh.golden()
    buf = io.BytesIO()
    Image.fromarray(jh.pixels(40, 56, "smooth", 7)).save(buf, "JPEG", quality=85, progressive=True)
    truncated = gold[8][1][: len(gold[8][1]) * 2 // 3]
    flipped = bytearray(gold[9][1])
    flipped[eh.scan_start(gold[9][1]) + 100] ^= 0x55
    return [gold[7][1], truncated, gold[8][1], bytes(flipped), buf.getvalue(), gold[11][1], gold[12][1]]


def _same_lists(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None and y is None) or (x is not None and y is not None and x.shape == y.shape and torch.equal(x, y)), i


def test_decode_jpeg_on_the_device_equals_the_host_path(jpeg, device):
    gold = jh.golden()
    files = [d for _, d, _ in gold] + [d for _, d in eh.fixtures()]
    a, sa = jpeg.decode_jpeg(files, device=device, on_unsupported="none", return_status=True, entropy="device")
    b, sb = jpeg.decode_jpeg(files, device=device, on_unsupported="none", return_status=True, entropy="host")
    assert np.array_equal(sa, sb) and not sa.any() and sa.dtype == sb.dtype
    _same_lists(a, b)
    for (name, _, want), got in zip(gold, a):
        assert np.array_equal(got.cpu().numpy(), want), name          # the committed Pillow pixels
    bad = _bad_batch()
    a, sa = jpeg.decode_jpeg(bad, device=device, on_unsupported="none", return_status=True, entropy="device")
    b, sb = jpeg.decode_jpeg(bad, device=device, on_unsupported="none", return_status=True, entropy="host")
    assert np.array_equal(sa, sb) and sa.tolist() == [0, 2, 0, sb[3], 1, 0, 0] and sb[3] in (0, 2), (sa, sb)
    _same_lists(a, b)
    assert a[1] is None and a[4] is None
    readable = [f for f, s in zip(bad, sb) if s != 2]                 # "pillow": Pillow raises for a corrupt file on either path
    a, sa = jpeg.decode_jpeg(readable, device=device, on_unsupported="pillow", return_status=True, entropy="device")
    b, sb = jpeg.decode_jpeg(readable, device=device, on_unsupported="pillow", return_status=True, entropy="host")
    assert np.array_equal(sa, sb) and sorted(sa.tolist())[-1] == 1 and all(x is not None for x in a)
    _same_lists(a, b)
    for entropy in ("host", "device"):
        with pytest.raises(ValueError, match=r"files\[1\] is corrupt"):
            jpeg.decode_jpeg(bad, device=device, on_unsupported="raise", entropy=entropy)
    only_bad, s = jpeg.decode_jpeg([bad[1], bad[4]], device=device, on_unsupported="none", return_status=True, entropy="device")
    assert only_bad == [None, None] and s.tolist() == [2, 1]          # nothing for the device stage


def test_overlapped_batches_on_the_device_equal_plain_calls(jpeg, device):
    gold = [d for _, d, _ in jh.golden()]
    batches = [gold[:5], gold[5:9], _bad_batch(), gold[9:] + [d for _, d in eh.fixtures()], gold[3:4]]
    plain = [jpeg.decode_jpeg(b, device=device, on_unsupported="none", return_status=True) for b in batches]
    count = 0
    for (imgs, status), (pimgs, pstatus) in zip(
            jpeg.decode_jpeg_batches(iter(batches), device=device, on_unsupported="none", return_status=True, entropy="device"), plain):
        assert np.array_equal(status, pstatus)
        _same_lists(imgs, pimgs)
        count += 1
    assert count == 5


# ------------------------------------------------------------------ 5. capture

def test_the_entropy_call_and_the_decode_kernels_replay_from_one_graph(jpeg, device):
    gold = jh.golden()
    picks = [7, 8, 9, 11, 12]
    files = [gold[i][1] for i in picks] + [eh.fixtures()[0][1]]
    res = jpeg.DeviceEntropyResult(jpeg.ScanBatch(files), device).upload()
    plan = jpeg.JpegPlan(res, device).upload()
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        res.run()
        plan.run()                                          # warm up outside the capture
    side.synchronize()
    first = [im.clone() for im in plan.images()]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res.run()
        plan.run()
    res.coef_dev.fill_(0x1234)
    plan.workspace.zero_()
    plan.out.zero_()
    res.stat_dev.fill_(-1)
    torch.cuda.synchronize(device)
    graph.replay()
    torch.cuda.synchronize(device)
    res._stat = None
    assert res.status.tolist() == [0] * len(files)
    for i, (got, was) in enumerate(zip(plan.images(), first)):
        assert torch.equal(got, was), i
    for i, g in enumerate(picks):
        assert np.array_equal(plan.images()[i].cpu().numpy(), gold[g][2]), gold[g][0]
