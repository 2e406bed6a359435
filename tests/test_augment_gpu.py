"""GPU: the train-time augmentation (device-built coefficient tables, crop-aware resample) against Pillow.  Everything
is equality: the chain is integer arithmetic or correctly rounded fp32 / fp64 operations."""
import numpy as np
import pytest
import torch

import augment_helpers as AH

pytestmark = pytest.mark.gpu

BAND = 256                                   # bytes of 0xA5 on each side of a guarded buffer (keeps 16-byte alignment)


def _banded(nbytes, device, band=BAND):
    """(whole, inner): a uint8 buffer of nbytes with `band` guard bytes before and after it, everything 0xA5."""
    whole = torch.full((band + nbytes + band,), AH.GUARD, dtype=torch.uint8, device=device)
    return whole, whole[band:band + nbytes]


def _bands_intact(whole, nbytes, band=BAND):
    return bool((whole[:band] == AH.GUARD).all()) and bool((whole[band + nbytes:] == AH.GUARD).all())


# ------------------------------------------------------------------ tables

IN_SIZES = lambda S: [1, 2, 3, 4, S - 1, S, S + 1, 2 * S, 2 * S + 1, 333, 1000, 4000]


@pytest.mark.parametrize("S", [224, 64, 30, 336])
def test_device_tables_are_the_host_tables(device, S):
    """One launch over mixed sizes (so kmax, set by the 4000-px side, exceeds most rows' own ksize): every size on both
    axes, flipped and not.  Bounds and every coefficient equal resample_tables(in, S, 0, S); the padded taps are zero; a
    flip reverses the horizontal rows and leaves the vertical ones alone; nothing is written outside the tables."""
    from mmr_amd import _lib, preprocess as P
    sizes = IN_SIZES(S)
    n = len(sizes)
    crops = [(sizes[i], sizes[(i + 3) % n], f) for f in (0, 1) for i in range(n)]            # (ch, cw, flip)
    boxes = np.array([[0, 0, ch, cw, f] for ch, cw, f in crops], dtype=np.int64)
    src = torch.zeros(16, dtype=torch.uint8, device=device)                                  # never read by this call
    desc, kmax, _, _, _ = P.crop_descriptors(np.full(len(crops), src.data_ptr()), boxes[:, 2:4], boxes, S)
    assert kmax == P.resample_tables(4000, S, 0, S)[2]
    B = len(crops)
    nbytes = P.augment_tables_bytes(B, S, kmax)
    L = _lib.lib()
    assert L.mmr_augment_tables_bytes(B, S, kmax) == nbytes
    whole, tables = _banded(nbytes, device)
    desc_d = torch.from_numpy(desc).to(device)
    _lib.check(L.mmr_augment_tables(desc_d.data_ptr(), B, S, kmax, tables.data_ptr(), nbytes, _lib.stream_ptr(device)))
    torch.cuda.synchronize()
    assert _bands_intact(whole, nbytes)
    t = tables.cpu().numpy().view(np.int32)
    bounds = t[:B * 2 * S * 2].reshape(B, 2, S, 2)
    coeffs = t[B * 2 * S * 2:].reshape(B, 2, S, kmax)
    for b, (ch, cw, flip) in enumerate(crops):
        for axis, size in ((0, cw), (1, ch)):
            wb, wc, k = P.resample_tables(size, S, 0, S)
            if axis == 0 and flip:
                wb, wc = wb[::-1], wc[::-1]
            assert np.array_equal(bounds[b, axis], wb), (S, size, axis, flip)
            assert np.array_equal(coeffs[b, axis, :, :k], wc), (S, size, axis, flip)
            assert not coeffs[b, axis, :, k:].any(), (S, size, axis, flip)
            taps = bounds[b, axis, :, 1]
            assert all(not coeffs[b, axis, j, taps[j]:].any() for j in range(S))


def test_tables_entry_point_checks_its_arguments(device):
    from mmr_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
    st = _lib.stream_ptr(device)
    assert L.mmr_augment_tables(buf.data_ptr(), 1, 32, 8, buf.data_ptr(), 16, st) != 0          # tables too small
    assert L.mmr_augment_tables(buf.data_ptr(), 1, 32, 9, buf.data_ptr(), 1 << 16, st) != 0     # kmax not padded
    assert L.mmr_augment_tables(buf.data_ptr(), 1, 32, 8, buf.data_ptr() + 4, 1 << 15, st) != 0  # misaligned
    assert L.mmr_augment_tables(buf.data_ptr(), 70000, 32, 8, buf.data_ptr(), 1 << 16, st) != 0
    assert L.mmr_augment_tables(buf.data_ptr(), 0, 32, 8, buf.data_ptr(), 0, st) == 0
    assert L.mmr_augment_tables_bytes(-1, 32, 8) == 0


# ------------------------------------------------------------------ bytes vs Pillow

SOURCES = {(301, 457): AH.image(301, 457, 1), (64, 64): AH.image(64, 64, 2)}
_pil_cache = {}


def _want(hw, box, S):
    key = (hw, tuple(int(v) for v in box), S)
    if key not in _pil_cache:
        _pil_cache[key] = AH.pil_crop(SOURCES[hw], box, S)
    return _pil_cache[key]


@pytest.mark.parametrize("hw", list(SOURCES))
@pytest.mark.parametrize("S", [64, 30, 224])
def test_bytes_equal_pillow(device, hw, S):
    from mmr_amd import augment_batch
    if S == 224:
        if hw == (64, 64):
            cases = [(0, 0, 64, 64), (10, 20, 37, 41)]
        else:
            cases = [(0, 0, 301, 457), (301 - 224, 457 - 224, 224, 224), (301 - 100, 457 - 224, 100, 224), (77, 0, 224, 150)]
    else:
        cases = AH.boxes_for(hw[0], hw[1], S)
    boxes = AH.with_flips(cases)
    img = torch.from_numpy(SOURCES[hw]).to(device)
    bt = torch.tensor(boxes, dtype=torch.int32)
    idx = [0] * len(boxes)
    want = np.stack([_want(hw, b, S) for b in boxes])
    out, u8 = augment_batch([img], bt, n_px=S, return_u8=True, image_index=idx)
    assert out.shape == (len(boxes), 3, S, S) and out.dtype == torch.float32 and u8.shape == (len(boxes), S, S, 3)
    got = u8.cpu().numpy()
    for i, b in enumerate(boxes):
        assert np.array_equal(got[i], want[i]), (hw, S, b, int(np.abs(got[i].astype(int) - want[i]).max()))
    assert torch.equal(out.cpu(), AH.normalise(want))
    bf = augment_batch([img], bt, n_px=S, out_dtype=torch.bfloat16, image_index=idx)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf.cpu(), AH.normalise(want, torch.bfloat16))
    assert torch.equal(img.cpu(), torch.from_numpy(SOURCES[hw]))


def test_narrow_crop_of_a_wide_image(device):
    from mmr_amd import augment_batch
    src = AH.image(300, 4000, 7)
    boxes = [(38, 3776, 224, 224, 0), (38, 3776, 224, 224, 1)]
    out, u8 = augment_batch([torch.from_numpy(src).to(device)], torch.tensor(boxes, dtype=torch.int32), n_px=224,
                            return_u8=True, image_index=[0, 0])
    want = np.stack([AH.pil_crop(src, b, 224) for b in boxes])
    assert np.array_equal(u8.cpu().numpy(), want)
    assert torch.equal(out.cpu(), AH.normalise(want))


def test_chunked_batches_give_the_same_bytes(device):
    """A workspace cap of one byte puts every crop in its own launch group."""
    from mmr_amd import augment_batch
    hw, S = (301, 457), 64
    boxes = AH.with_flips(AH.boxes_for(301, 457, S))[:9]
    img = torch.from_numpy(SOURCES[hw]).to(device)
    bt = torch.tensor(boxes, dtype=torch.int32)
    _, u8 = augment_batch([img], bt, n_px=S, return_u8=True, image_index=[0] * 9, workspace_cap=1)
    assert np.array_equal(u8.cpu().numpy(), np.stack([_want(hw, b, S) for b in boxes]))


# ------------------------------------------------------------------ read safety

@pytest.mark.parametrize("layout", ["one allocation", "tail of its own allocation"])
@pytest.mark.parametrize("S", [64, 30])
def test_nothing_outside_the_buffers_is_written_and_sources_at_an_allocations_end_are_fine(device, layout, S):
    """Through the C ABI with caller-made buffers.  The sources lie at odd addresses between 0xA5 guard bands of one
    allocation, or each as the very last bytes of an allocation of its own (the bottom-right boxes then make the 12- and
    16-byte loads meet the end of the allocation).  Bytes equal Pillow's; sources, their guards and the guard bands around
    out, out_u8, the tables and the scratch are unchanged."""
    from mmr_amd import _lib, preprocess as P
    srcs = [SOURCES[(301, 457)], SOURCES[(64, 64)]]
    gap = 4099                                                      # odd: the sources start unaligned
    if layout == "one allocation":
        total = gap + sum(s.size + gap for s in srcs)
        pool = torch.full((total,), AH.GUARD, dtype=torch.uint8, device=device)
        views, at = [], gap
        for s in srcs:
            views.append(pool[at:at + s.size])
            at += s.size + gap
        pools = [pool]
    else:
        pools = [torch.full((gap + s.size,), AH.GUARD, dtype=torch.uint8, device=device) for s in srcs]
        views = [p[gap:] for p in pools]
    for v, s in zip(views, srcs):
        v.copy_(torch.from_numpy(s.reshape(-1)))
    before = [p.clone() for p in pools]

    boxes, idx = [], []
    for i, s in enumerate(srcs):
        bs = AH.with_flips(AH.boxes_for(s.shape[0], s.shape[1], S))
        boxes += bs
        idx += [i] * len(bs)
    bx = np.array(boxes, dtype=np.int64)
    idx = np.array(idx)
    sizes = np.array([[s.shape[0], s.shape[1]] for s in srcs], dtype=np.int64)[idx]
    ptrs = np.array([v.data_ptr() for v in views], dtype=np.int64)[idx]
    desc, kmax, max_ch, max_cw, scratch_bytes = P.crop_descriptors(ptrs, sizes, bx, S)
    B = len(boxes)
    tb = P.augment_tables_bytes(B, S, kmax)
    w_tab, tables = _banded(tb, device)
    w_scr, scratch = _banded(scratch_bytes, device)
    w_out, out = _banded(B * 3 * S * S * 4, device)
    w_u8, u8 = _banded(B * S * S * 3, device)
    desc_d = torch.from_numpy(desc).to(device)
    L, st = _lib.lib(), _lib.stream_ptr(device)
    _lib.check(L.mmr_augment_tables(desc_d.data_ptr(), B, S, kmax, tables.data_ptr(), tb, st))
    _lib.check(L.mmr_augment_resample(desc_d.data_ptr(), B, S, kmax, max_ch, max_cw, tables.data_ptr(), tb, scratch.data_ptr(),
                                      scratch_bytes, *[float(v) for v in AH.MEAN], *[float(v) for v in AH.STD], out.data_ptr(),
                                      _lib.MMR_F32, u8.data_ptr(), st))
    torch.cuda.synchronize()
    want = np.stack([AH.pil_crop(srcs[i], b, S) for i, b in zip(idx, boxes)])
    assert np.array_equal(u8.cpu().numpy().reshape(B, S, S, 3), want)
    assert torch.equal(out.cpu().view(torch.float32).view(B, 3, S, S), AH.normalise(want))
    for p, b in zip(pools, before):
        assert torch.equal(p, b)
    assert _bands_intact(w_tab, tb) and _bands_intact(w_scr, scratch_bytes)
    assert _bands_intact(w_out, B * 3 * S * S * 4) and _bands_intact(w_u8, B * S * S * 3)


def test_resample_entry_point_skips_what_it_must_not_touch(device):
    """A crop outside its image, or whose rows would leave the scratch, is not processed: its outputs keep their bytes."""
    from mmr_amd import _lib, preprocess as P
    S = 32
    src = torch.from_numpy(AH.image(40, 50, 3)).to(device)
    bx = np.array([[0, 0, 40, 50, 0], [30, 0, 11, 50, 0], [0, 45, 10, 6, 0], [0, 0, 20, 20, 1]], dtype=np.int64)   # 1, 2: outside
    sizes = np.array([[40, 50]] * 4, dtype=np.int64)
    desc, kmax, max_ch, max_cw, scratch_bytes = P.crop_descriptors(np.full(4, src.data_ptr()), sizes, bx, S)
    tb = P.augment_tables_bytes(4, S, kmax)
    tables = torch.zeros(tb, dtype=torch.uint8, device=device)
    scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device=device)
    w_out, out = _banded(4 * 3 * S * S * 4, device)
    w_u8, u8 = _banded(4 * S * S * 3, device)
    desc_d = torch.from_numpy(desc).to(device)
    L, st = _lib.lib(), _lib.stream_ptr(device)
    norm = [float(v) for v in AH.MEAN] + [float(v) for v in AH.STD]
    _lib.check(L.mmr_augment_tables(desc_d.data_ptr(), 4, S, kmax, tables.data_ptr(), tb, st))
    # the last crop's rows end 16 bytes short of the scratch the call is told about: it is skipped as well
    _lib.check(L.mmr_augment_resample(desc_d.data_ptr(), 4, S, kmax, max_ch, max_cw, tables.data_ptr(), tb, scratch.data_ptr(),
                                      scratch_bytes - 16, *norm, out.data_ptr(), _lib.MMR_F32, u8.data_ptr(), st))
    torch.cuda.synchronize()
    got = u8.cpu().numpy().reshape(4, S, S, 3)
    assert np.array_equal(got[0], AH.pil_crop(src.cpu().numpy(), bx[0], S))
    assert (got[1:] == AH.GUARD).all()
    assert _bands_intact(w_out, 4 * 3 * S * S * 4) and _bands_intact(w_u8, 4 * S * S * 3)
    assert L.mmr_augment_resample(desc_d.data_ptr(), 4, S, kmax, max_ch, max_cw, tables.data_ptr(), tb - 16, scratch.data_ptr(),
                                  scratch_bytes, *norm, out.data_ptr(), _lib.MMR_F32, u8.data_ptr(), st) != 0


# ------------------------------------------------------------------ batch independence

def test_a_crop_does_not_depend_on_its_batch(device):
    from mmr_amd import augment_batch, random_resized_crop_params
    S = 64
    shapes = [(120, 160), (301, 457), (64, 64), (97, 33), (200, 640)]
    imgs = [torch.from_numpy(AH.image(h, w, 20 + i)).to(device) for i, (h, w) in enumerate(shapes)]
    idx = [0] * 8 + [1 + i % 4 for i in range(32)]
    boxes = random_resized_crop_params([shapes[i] for i in idx], scale=(0.08, 1.0), generator=torch.Generator().manual_seed(9))
    assert 0 < int(boxes[:, 4].sum()) < 40
    out, u8 = augment_batch(imgs, boxes, n_px=S, return_u8=True, image_index=idx)
    for b in range(40):
        o1, u1 = augment_batch(imgs, boxes[b:b + 1], n_px=S, return_u8=True, image_index=idx[b:b + 1])
        assert torch.equal(u1[0], u8[b]) and torch.equal(o1[0], out[b]), b
    rev = list(range(39, -1, -1))
    o2, u2 = augment_batch(imgs, boxes[rev], n_px=S, return_u8=True, image_index=[idx[i] for i in rev])
    assert torch.equal(u2[rev], u8) and torch.equal(o2[rev], out)
    # and the default index: one crop per image, in order
    per_image = random_resized_crop_params(shapes, generator=torch.Generator().manual_seed(10))
    o4 = augment_batch(imgs, per_image, n_px=S)
    o5 = augment_batch(imgs, per_image, n_px=S, image_index=[0, 1, 2, 3, 4])
    assert torch.equal(o4, o5)


def test_the_launches_can_be_captured_in_a_graph(device):
    """No allocation and no synchronisation inside the two calls: they are captured once and replayed on new boxes."""
    from mmr_amd import _lib, preprocess as P
    S = 64
    src_np = SOURCES[(301, 457)]
    src = torch.from_numpy(src_np).to(device)
    first = np.array([[0, 0, 301, 457, 0], [100, 200, 150, 200, 1]], dtype=np.int64)
    second = np.array([[1, 7, 300, 450, 1], [120, 210, 140, 180, 0]], dtype=np.int64)
    sizes = np.array([[301, 457]] * 2, dtype=np.int64)
    ptrs = np.full(2, src.data_ptr())
    desc, kmax, max_ch, max_cw, scratch_bytes = P.crop_descriptors(ptrs, sizes, first, S)
    desc2, kmax2, _, _, _ = P.crop_descriptors(ptrs, sizes, second, S)
    assert kmax2 == kmax and (second[:, 2] <= first[:, 2]).all() and (second[:, 3] <= max_cw).all()
    desc2[:, 1] = desc[:, 1]                                        # the same scratch ranges
    tb = P.augment_tables_bytes(2, S, kmax)
    tables = torch.zeros(tb, dtype=torch.uint8, device=device)
    scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device=device)
    out = torch.zeros(2, 3, S, S, device=device)
    u8 = torch.zeros(2, S, S, 3, dtype=torch.uint8, device=device)
    desc_d = torch.from_numpy(desc).to(device)
    L = _lib.lib()
    norm = [float(v) for v in AH.MEAN] + [float(v) for v in AH.STD]

    def enqueue():
        st = _lib.stream_ptr(device)
        _lib.check(L.mmr_augment_tables(desc_d.data_ptr(), 2, S, kmax, tables.data_ptr(), tb, st))
        _lib.check(L.mmr_augment_resample(desc_d.data_ptr(), 2, S, kmax, max_ch, max_cw, tables.data_ptr(), tb,
                                          scratch.data_ptr(), scratch_bytes, *norm, out.data_ptr(), _lib.MMR_F32,
                                          u8.data_ptr(), st))

    enqueue()                                                       # once outside the capture: one-time kernel attributes
    torch.cuda.synchronize()
    out.zero_()
    u8.zero_()
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            enqueue()
    torch.cuda.current_stream(device).wait_stream(side)
    for boxes, d in ((first, desc), (second, desc2)):
        desc_d.copy_(torch.from_numpy(d))
        graph.replay()
        torch.cuda.synchronize()
        want = np.stack([AH.pil_crop(src_np, b, S) for b in boxes])
        assert np.array_equal(u8.cpu().numpy(), want)
        assert torch.equal(out.cpu(), AH.normalise(want))


# ------------------------------------------------------------------ end to end

@pytest.fixture(scope="module")
def few_shot(device):
    import mmr_amd
    model, _ = mmr_amd.load("tiny-test", device=device)
    shapes = [(90, 120), (64, 64), (150, 100), (77, 131), (200, 200), (65, 97)]
    imgs_np = [AH.image(h, w, 40 + i) for i, (h, w) in enumerate(shapes)]
    imgs = [torch.from_numpy(a).to(device) for a in imgs_np]
    targets = torch.tensor([0, 1, 2, 0, 1, 2])
    return model, shapes, imgs_np, imgs, targets


def _pil_batches(model, shapes, imgs_np, targets, generator, batch_size):
    """The host loader: the SAME boxes (one sampler call per epoch on an equally seeded generator), applied with PIL."""
    from mmr_amd import random_resized_crop_params
    S = model.cfg.vision.image_size
    boxes = random_resized_crop_params(shapes, generator=generator).numpy()
    for s in range(0, len(shapes), batch_size):
        u8 = np.stack([AH.pil_crop(imgs_np[i], boxes[i], S) for i in range(s, min(s + batch_size, len(shapes)))])
        yield AH.normalise(u8), targets[s:s + batch_size]


def test_augmented_cache_equals_the_pil_loader(few_shot):
    from mmr_amd import gallery
    model, shapes, imgs_np, imgs, targets = few_shot
    keys, vals = gallery.build_cache_model_augmented(model, imgs, targets, 2, 3, generator=torch.Generator().manual_seed(77), batch_size=4)
    g = torch.Generator().manual_seed(77)
    rk, rv = gallery.build_cache_model(model, lambda: _pil_batches(model, shapes, imgs_np, targets, g, 4), 2, 3)
    assert keys.shape == (model.cfg.embed_dim, 6) and vals.shape == (6, 3)
    assert torch.equal(keys, rk) and torch.equal(vals, rv)
    other, _ = gallery.build_cache_model_augmented(model, imgs, targets, 2, 3, generator=torch.Generator().manual_seed(78), batch_size=4)
    assert not torch.equal(other, keys)                         # the boxes do reach the features


def test_augmented_features_equal_encoding_the_pil_crops(few_shot):
    from mmr_amd import gallery
    model, shapes, imgs_np, imgs, targets = few_shot
    feats, lab = gallery.augmented_features(model, imgs, targets, torch.Generator().manual_seed(5), batch_size=4)
    g = torch.Generator().manual_seed(5)
    want, wl = gallery.encode_gallery(model, _pil_batches(model, shapes, imgs_np, targets, g, 4), normalize=True,
                                      out_dtype=torch.bfloat16, return_labels=True)
    assert feats.dtype == torch.bfloat16 and feats.shape == (6, model.cfg.embed_dim)
    assert torch.equal(feats, want) and torch.equal(lab.cpu(), wl) and lab.is_cuda and lab.dtype == torch.int64
