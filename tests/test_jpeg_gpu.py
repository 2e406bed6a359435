"""GPU: decode_jpeg equals Pillow byte for byte -- the committed goldens always, this machine's Pillow over the whole shape
list when it reproduces the goldens -- for single calls and one ragged batch; the component planes are checked on their
own, so that an inverse-DCT error is not blamed on the upsampling; bad files in a batch, guard bands behind every image,
repeatability, graph replay, the overlapped batches, and the hashes and preprocessed bytes of the decoded tensors."""
import numpy as np
import pytest
import torch

import jpeg_helpers as jh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jpeg(device):
    from mmr_amd import jpeg

    return jpeg


@pytest.fixture(scope="module")
def shape_list():
    """[(name, file bytes, live Pillow's RGB)] for the shape list and the one large image, built once"""
    if not jh.live_pillow_reproduces_golden():
        pytest.skip("this machine's Pillow does not decode the golden files to the golden pixels: live comparisons are skipped, "
                    "the golden comparisons still run")
    out = []
    for case in jh.SHAPE_LIST + [jh.LARGE]:
        data = jh.build(case)
        out.append((case["name"], data, jh.pillow_rgb(data)))
    return out


def _same(got, want, name):
    assert got is not None and tuple(got.shape) == want.shape and got.dtype == torch.uint8, (name, None if got is None else got.shape, want.shape)
    g = got.cpu().numpy()
    assert np.array_equal(g, want), (name, int((g != want).sum()), "bytes differ")


def test_goldens_byte_for_byte(jpeg, device):
    gold = jh.golden()
    imgs, status = jpeg.decode_jpeg([d for _, d, _ in gold], device=device, on_unsupported="none", return_status=True)
    assert status.dtype == np.int32 and not status.any()
    for (name, _, want), got in zip(gold, imgs):
        _same(got, want, name)
    for name, data, want in gold[:4]:
        _same(jpeg.decode_jpeg([data], device=device, on_unsupported="raise")[0], want, name)


def test_live_pillow_one_image_per_call(jpeg, device, shape_list):
    for name, data, want in shape_list:
        _same(jpeg.decode_jpeg([data], device=device, on_unsupported="raise")[0], want, name)


def test_live_pillow_one_ragged_call(jpeg, device, shape_list):
    imgs = jpeg.decode_jpeg([d for _, d, _ in shape_list], device=device, on_unsupported="raise")
    for (name, _, want), got in zip(shape_list, imgs):
        _same(got, want, name)


def test_component_planes_equal_the_restatement(jpeg, device):
    cases = jh.SHAPE_LIST + [jh.LARGE]
    host = jpeg.entropy_decode([jh.build(c) for c in cases])
    assert not host.status.any()
    plan = jpeg.JpegPlan(host, device).upload().run()
    for i, c in enumerate(cases):
        want, _ = jh.restate(host.infos[i], host.blocks(i), host.qt[i])
        got = plan.planes(i)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), (c["name"], "plane", k)


def _bad_batch():
    from PIL import Image
    import io

    gold = jh.golden()
    px = jh.pixels(40, 56, "smooth", 7)
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, "JPEG", quality=85, progressive=True)
    progressive = buf.getvalue()
    truncated = gold[8][1][: len(gold[8][1]) * 2 // 3]
    files = [gold[7][1], gold[8][1], progressive, truncated, gold[9][1], gold[12][1]]
    wants = [gold[7][2], gold[8][2], None, None, gold[9][2], gold[12][2]]
    return files, wants, progressive


def test_bad_files_in_the_middle_of_a_batch(jpeg, device):
    files, wants, progressive = _bad_batch()
    imgs, status = jpeg.decode_jpeg(files, device=device, on_unsupported="none", return_status=True)
    assert status.tolist() == [0, 0, jpeg.JPEG_UNSUPPORTED, jpeg.JPEG_CORRUPT, 0, 0]
    for i, want in enumerate(wants):
        if want is None:
            assert imgs[i] is None
        else:
            _same(imgs[i], want, i)
    with pytest.raises(ValueError, match=r"files\[2\]"):
        jpeg.decode_jpeg(files, device=device, on_unsupported="raise")
    imgs, status = jpeg.decode_jpeg(files[2:4], device=device, on_unsupported="none", return_status=True)     # nothing for the device
    assert imgs == [None, None] and status.tolist() == [jpeg.JPEG_UNSUPPORTED, jpeg.JPEG_CORRUPT]
    imgs = jpeg.decode_jpeg(files[:3] + files[4:], device=device)            # "pillow": the progressive file is Pillow's
    _same(imgs[2], jh.pillow_rgb(progressive), "progressive")
    for got, want in zip(imgs[:2] + imgs[3:], wants[:2] + wants[4:]):
        _same(got, want, "neighbour")


def test_guard_bands_behind_every_image_stay_untouched(jpeg, device):
    gold = jh.golden()
    files, wants, _ = _bad_batch()
    files, wants = [d for _, d, _ in gold] + files, [w for _, _, w in gold] + wants
    host = jpeg.entropy_decode(files)
    plan = jpeg.JpegPlan(host, device, guard=64, fill=0xA5).upload().run()
    out = plan.out.cpu().numpy()
    covered = np.zeros(out.size, dtype=bool)
    for i, want in enumerate(wants):
        if want is None:
            assert plan.images()[i] is None
            continue
        at = int(plan.offsets[i])
        assert np.array_equal(out[at: at + want.size].reshape(want.shape), want), i
        assert (out[at + want.size: at + want.size + 64] == 0xA5).all(), i
        covered[at: at + want.size] = True
    assert (out[~covered] == 0xA5).all()


def test_two_calls_give_identical_bytes(jpeg, device):
    files = [d for _, d, _ in jh.golden()]
    a = jpeg.decode_jpeg(files, device=device)
    b = jpeg.decode_jpeg(files, device=device)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_graph_replay_after_the_coefficients_were_overwritten(jpeg, device):
    names = ("17x33_422_noise", "37x51_420_smooth", "48x64_444", "17x33_grey", "9x3_422")
    by_name = {c["name"]: c for c in jh.SHAPE_LIST}
    first = [jh.build(by_name[n], seed=1) for n in names]
    second = [jh.build(by_name[n], seed=2) for n in names]
    ha, hb = jpeg.entropy_decode(first), jpeg.entropy_decode(second)
    assert np.array_equal(ha.coef_off, hb.coef_off) and ha.coef_bytes == hb.coef_bytes
    plan = jpeg.JpegPlan(ha, device).upload()
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        plan.run()                                          # warm up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.run()
    n = hb.coef_bytes // 2
    plan.coef_dev[:n].copy_(torch.from_numpy(hb.coef[:n]))  # the second batch in the same buffers
    plan.qt_dev.copy_(torch.from_numpy(hb.qt.view(np.int16).reshape(-1)))
    plan.out.zero_()
    torch.cuda.synchronize(device)
    graph.replay()
    torch.cuda.synchronize(device)
    for i, (name, data, got) in enumerate(zip(names, second, plan.images())):
        _, want = jh.restate(hb.infos[i], hb.blocks(i), hb.qt[i])
        _same(got, want, name)
        if jh.live_pillow_reproduces_golden():
            _same(got, jh.pillow_rgb(data), name)


def test_overlapped_batches_equal_plain_calls(jpeg, device):
    gold = [d for _, d, _ in jh.golden()]
    files, _, _ = _bad_batch()
    batches = [gold[:5], gold[5:9], files, gold[9:], gold[3:4]]
    plain = [jpeg.decode_jpeg(b, device=device, on_unsupported="none", return_status=True) for b in batches]
    count = 0
    for (imgs, status), (pimgs, pstatus) in zip(jpeg.decode_jpeg_batches(iter(batches), device=device, on_unsupported="none", return_status=True), plain):
        assert np.array_equal(status, pstatus) and len(imgs) == len(pimgs)
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(imgs, pimgs))
        count += 1
    assert count == 5 and plain[2][1].tolist() == [0, 0, 1, 2, 0, 0]


def test_hashes_and_preprocess_of_decoded_tensors_equal_those_of_pillow_pixels(jpeg, device):
    import mmr_amd
    from mmr_amd import preprocess

    gold = [g for g in jh.golden() if g[2].shape[0] >= 16 and g[2].shape[1] >= 15]
    assert len(gold) >= 6
    ours = jpeg.decode_jpeg([d for _, d, _ in gold], device=device, on_unsupported="raise")
    theirs = [torch.from_numpy(w).to(device) for _, _, w in gold]
    ha, sa = mmr_amd.image_hashes(ours, return_status=True)
    hb, sb = mmr_amd.image_hashes(theirs, return_status=True)
    assert torch.equal(ha, hb) and torch.equal(sa, sb)
    assert torch.equal(preprocess.preprocess_batch(ours, 32), preprocess.preprocess_batch(theirs, 32))
