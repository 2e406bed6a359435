"""GPU: encode_jpeg equals Pillow byte for byte -- the committed goldens always, this machine's Pillow over the whole shape
list when it reproduces the goldens -- one image per call and all in one ragged call; the component planes after the first
kernel and the coefficients after the second are compared with the numpy restatement on their own, so that an error is
blamed on the right kernel; guard bands, untouched inputs, refused inputs, graph replay, RGBA compositing, the round trip
through decode_jpeg, the overlapped batches and save_jpeg."""
import numpy as np
import pytest
import torch

import jpeg_encode_helpers as eh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jpeg(device):
    from mmr_amd import jpeg

    return jpeg


@pytest.fixture(scope="module")
def live():
    """[(case, pixels, live Pillow's bytes)] for the shape list and the one 480 x 640 image, built once"""
    if not eh.live_pillow_reproduces_golden():
        pytest.skip("this machine's Pillow does not write the golden files from the golden pixels: live comparisons are skipped, "
                    "the golden comparisons still run")
    out = []
    for case in eh.SHAPE_LIST + [eh.LARGE]:
        px = eh.case_pixels(case)
        out.append((case, px, eh.build(case, px)))
    return out


def _options(case):
    return dict(eh.case_options(case), restart_interval=case["restart"])


def _groups(items):
    """cases that share their options, so that each group is one ragged call: {options: [index]}"""
    groups = {}
    for i, (case, _, _) in enumerate(items):
        groups.setdefault(tuple(sorted((k, str(v)) for k, v in _options(case).items())), []).append(i)
    return groups


def _ragged(jpeg, device, items):
    got = [None] * len(items)
    for rows in _groups(items).values():
        files = jpeg.encode_jpeg([torch.from_numpy(items[i][1]).to(device) for i in rows], **_options(items[rows[0]][0]))
        for i, f in zip(rows, files):
            got[i] = f
    return got


def _same_file(got, want, name):
    assert isinstance(got, bytes), name
    where = "the scan" if got[:len(got) - len(eh.scan_of(got))] == want[:len(want) - len(eh.scan_of(want))] else "the headers"
    assert got == want, (name, len(got), len(want), "first difference in " + where)


def test_goldens_byte_for_byte(jpeg, device):
    gold = eh.golden()
    for (case, _, want), got in zip(gold, _ragged(jpeg, device, gold)):
        _same_file(got, want, case["name"])
    for case, px, want in gold[:6] + gold[-4:]:
        _same_file(jpeg.encode_jpeg(torch.from_numpy(px).to(device), **_options(case))[0], want, case["name"])


def test_live_pillow_one_image_per_call(jpeg, device, live):
    for case, px, want in live:
        _same_file(jpeg.encode_jpeg([torch.from_numpy(px).to(device)], **_options(case))[0], want, case["name"])


def test_live_pillow_ragged_calls(jpeg, device, live):
    assert max(len(rows) for rows in _groups(live).values()) >= 12              # most of the list shares quality 95
    for (case, _, want), got in zip(live, _ragged(jpeg, device, live)):
        _same_file(got, want, case["name"])


def test_pillows_subsampling_codes_and_greyscale_ignore(jpeg, device):
    case, px, want = next(g for g in eh.golden() if g[0]["name"] == "17x33_422_noise_q95")
    x = torch.from_numpy(px).to(device)
    assert jpeg.encode_jpeg(x, subsampling=1)[0] == want
    grey = next(g for g in eh.golden() if g[0]["name"] == "17x33_grey_noise_q95")
    for s in ("4:4:4", 1, "4:2:0"):
        assert jpeg.encode_jpeg(torch.from_numpy(grey[1]).to(device), subsampling=s)[0] == grey[2]


def test_planes_and_coefficients_equal_the_restatement_each_on_its_own(jpeg, device):
    cases = eh.SHAPE_LIST + [eh.LARGE]
    by_options = {}
    for c in cases:
        by_options.setdefault((c["quality"], c["sub"], c["background"]), []).append(c)
    for (quality, sub, background), group in by_options.items():
        pxs = [eh.case_pixels(c) for c in group]
        bg = background or (255, 255, 255)
        plan = jpeg.JpegEncodePlan([torch.from_numpy(p).to(device) for p in pxs], quality, sub, bg).run()
        files, coefs = jpeg.encode_jpeg([torch.from_numpy(p).to(device) for p in pxs], quality, sub, background=bg, return_coefficients=True)
        for i, (c, px) in enumerate(zip(group, pxs)):
            want_planes, want_coef, _, _ = eh.restate(px, quality, sub, bg)
            got = plan.planes(i)
            assert len(got) == len(want_planes)
            for k, (g, w) in enumerate(zip(got, want_planes)):
                g = g.cpu().numpy()
                assert g.shape == w.shape and np.array_equal(g, w), (c["name"], "kernel 1, plane", k, int((g != w).sum()))
            for blocks in (plan.blocks(i), coefs[i]):
                assert len(blocks) == len(want_coef)
                for k, (g, w) in enumerate(zip(blocks, want_coef)):
                    assert g.dtype == np.int16 and g.shape == w.shape and np.array_equal(g, w), (c["name"], "kernel 2, component", k, int((g != w).sum()))


def test_guard_bands_behind_every_plane_span_and_coefficient_span_stay_untouched(jpeg, device):
    gold = [g for g in eh.golden() if g[0]["quality"] == 95 and g[0]["sub"] == "4:2:0" and not g[0]["background"]]
    assert len(gold) >= 12
    plan = jpeg.JpegEncodePlan([torch.from_numpy(px).to(device) for _, px, _ in gold], 95, "4:2:0", guard=64, fill=0xA5).run()
    ws, coef = plan.workspace.cpu().numpy(), plan.coef_dev.view(torch.uint8).cpu().numpy()
    covered_ws, covered_coef = np.zeros(ws.size, dtype=bool), np.zeros(coef.size, dtype=bool)
    for i, (case, px, _) in enumerate(gold):
        want_planes, want_coef, _, _ = eh.restate(px, 95, "4:2:0")
        blocks = sum(len(c) for c in want_coef)
        at = int(plan.desc_host[i]["plane_off"])
        assert np.array_equal(ws[at: at + blocks * 64], np.concatenate([p.reshape(-1) for p in want_planes])), case["name"]
        assert (ws[at + blocks * 64: at + blocks * 64 + 64] == 0xA5).all(), case["name"]
        covered_ws[at: at + blocks * 64] = True
        at = int(plan.coef_off[i])
        assert np.array_equal(coef[at: at + blocks * 128].view(np.int16), np.concatenate([c.reshape(-1) for c in want_coef])), case["name"]
        assert (coef[at + blocks * 128: at + blocks * 128 + 64] == 0xA5).all(), case["name"]
        covered_coef[at: at + blocks * 128] = True
    assert (~covered_ws).sum() == 64 * len(gold) and (ws[~covered_ws] == 0xA5).all()
    assert (~covered_coef).sum() == 64 * len(gold) and (coef[~covered_coef] == 0xA5).all()


def test_inputs_are_unchanged_and_two_calls_give_identical_bytes(jpeg, device):
    gold = [g for g in eh.golden() if g[0]["quality"] == 95 and g[0]["sub"] == "4:2:0" and not g[0]["restart"]]
    xs = [torch.from_numpy(px).to(device) for _, px, _ in gold]
    a = jpeg.encode_jpeg(xs)
    b = jpeg.encode_jpeg(xs)
    assert a == b
    for x, (_, px, _) in zip(xs, gold):
        assert np.array_equal(x.cpu().numpy(), px)


def test_refused_inputs(jpeg, device):
    x = torch.zeros(16, 24, 3, dtype=torch.uint8, device=device)
    with pytest.raises(ValueError, match="contiguous"):
        jpeg.encode_jpeg([x[:, ::2]])
    with pytest.raises(ValueError, match="contiguous"):
        jpeg.encode_jpeg([x.permute(1, 0, 2)])
    with pytest.raises(ValueError, match="contiguous"):
        jpeg.encode_jpeg(torch.zeros(16, 24, 4, dtype=torch.uint8, device=device)[:, :, :3])
    for bad in (x.float(), x.to(torch.int8), x.to(torch.int16)):
        with pytest.raises(ValueError, match="uint8"):
            jpeg.encode_jpeg([x, bad])
    with pytest.raises(ValueError, match=r"\[H, W"):
        jpeg.encode_jpeg([x[None]])
    with pytest.raises(RuntimeError, match="GPU"):
        jpeg.encode_jpeg([x, x.cpu()])
    with pytest.raises(ValueError, match="quality"):
        jpeg.encode_jpeg([x], quality=0)
    assert jpeg.encode_jpeg([x])[0][:2] == b"\xff\xd8"


def test_graph_replay_on_new_pixels_of_the_same_sizes(jpeg, device):
    names = ("17x33_422_noise_q95", "37x51_422_noise_q95", "9x3_422_noise_q95", "17x33_grey_noise_q95", "9x3_422_noise_q95_rgba")
    by_name = {c["name"]: c for c in eh.SHAPE_LIST}
    first = [eh.case_pixels(by_name[n], seed=1) for n in names]
    second = [eh.case_pixels(by_name[n], seed=2) for n in names]
    xs = [torch.from_numpy(p).to(device) for p in first]
    plan = jpeg.JpegEncodePlan(xs, 95, "4:2:2")
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        plan.run()                                          # warm up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.run()
    for x, p in zip(xs, second):
        x.copy_(torch.from_numpy(p))                        # the second batch in the same tensors
    plan.coef_dev.zero_()
    torch.cuda.synchronize(device)
    graph.replay()
    torch.cuda.synchronize(device)
    files, status = jpeg.entropy_encode(plan.coef_dev.cpu().numpy(), plan.coef_off, plan.infos, plan.qt)
    assert not status.any()
    for i, (n, px) in enumerate(zip(names, second)):
        _, want, _, _ = eh.restate(px, 95, "4:2:2")
        assert all(np.array_equal(g, w) for g, w in zip(plan.blocks(i), want)), n
        if eh.live_pillow_reproduces_golden():
            _same_file(files[i], eh.write_jpeg(px, 95, "4:2:2"), n)
    assert files != jpeg.encode_jpeg([torch.from_numpy(p).to(device) for p in first], subsampling="4:2:2")


def test_rgba_over_white_and_over_another_colour(jpeg, device):
    comp = eh.golden_composited()
    rgba = [g for g in eh.golden() if g[0]["channels"] == 4]
    assert {bool(c["background"]) for c, _, _ in rgba} == {True, False}
    for case, px, want in rgba:
        bg = case["background"] or (255, 255, 255)
        x = torch.from_numpy(px).to(device)
        _same_file(jpeg.encode_jpeg(x, subsampling=case["sub"], background=bg)[0], want, case["name"])
        # the composited RGB pixels give the same file, and the alpha band matters
        assert jpeg.encode_jpeg(torch.from_numpy(comp[case["name"]]).to(device), subsampling=case["sub"])[0] == want
        assert jpeg.encode_jpeg(x[:, :, :3].contiguous(), subsampling=case["sub"])[0] != want
    if eh.live_pillow_reproduces_golden():
        px = eh.pixels(37, 51, "noise", 77, channels=4)
        px[:8, :, 3], px[8:16, :, 3] = 0, 255                  # the two ends of the blend
        for bg in ((255, 255, 255), (0, 0, 0), (12, 250, 99)):
            for sub in ("4:2:0", "4:4:4"):
                got = jpeg.encode_jpeg(torch.from_numpy(px).to(device), quality=90, subsampling=sub, background=bg)[0]
                _same_file(got, eh.write_jpeg(px, 90, sub, background=bg), (bg, sub))


def test_decode_of_our_file_equals_pillows_decode_of_pillows_file(jpeg, device):
    from PIL import Image
    import io

    gold = eh.golden()
    ours = _ragged(jpeg, device, gold)
    decoded = jpeg.decode_jpeg(ours, device=device, on_unsupported="raise")
    live = eh.live_pillow_reproduces_golden()
    for (case, _, want), mine, d in zip(gold, ours, decoded):
        assert mine == want, case["name"]
        if live:                                                # Pillow's decode of the golden bytes, where this Pillow is the goldens' Pillow
            with Image.open(io.BytesIO(want)) as im:
                assert np.array_equal(d.cpu().numpy(), np.array(im.convert("RGB"), dtype=np.uint8)), case["name"]


def test_overlapped_batches_and_save_jpeg_equal_plain_calls(jpeg, device, tmp_path):
    gold = [g for g in eh.golden() if g[0]["quality"] == 95 and g[0]["sub"] == "4:2:0" and not g[0]["restart"] and not g[0]["background"]]
    xs = [torch.from_numpy(px).to(device) for _, px, _ in gold]
    batches = [xs[:5], xs[5:6], xs[6:11], xs[11:], xs[2:4]]
    plain = [jpeg.encode_jpeg(b) for b in batches]
    got = list(jpeg.encode_jpeg_batches(iter(batches)))
    assert got == plain and [f for files in plain[:4] for f in files] == [want for _, _, want in gold]
    assert list(jpeg.encode_jpeg_batches([])) == []
    paths = [str(tmp_path / f"{i}.jpg") for i in range(len(xs))]
    sizes = jpeg.save_jpeg(xs, paths)
    for p, n, (_, _, want) in zip(paths, sizes, gold):
        with open(p, "rb") as f:
            assert f.read() == want and n == len(want)
    import mmr_amd

    assert mmr_amd.encode_jpeg is jpeg.encode_jpeg and mmr_amd.save_jpeg is jpeg.save_jpeg and mmr_amd.JpegEncodePlan is jpeg.JpegEncodePlan
