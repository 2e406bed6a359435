"""CPU: the two facts the device augmentation rests on (full-box tables applied to the crop window are Pillow's
crop().resize(); a flip is the horizontal table read backwards), the box sampler, and augment_batch's host validation.
Nothing here launches a kernel."""
import numpy as np
import pytest
import torch

import augment_helpers as AH

SOURCES = {(301, 457): AH.image(301, 457, 1), (64, 64): AH.image(64, 64, 2)}


# ------------------------------------------------------------------ numpy application of the full-box tables vs Pillow

@pytest.mark.parametrize("hw", list(SOURCES))
@pytest.mark.parametrize("S", [64, 30])
def test_full_box_tables_on_the_window_are_pillows_crop_resize(hw, S):
    img = SOURCES[hw]
    for box in AH.with_flips(AH.boxes_for(hw[0], hw[1], S)):
        got, want = AH.apply_full_box_tables(img, box, S), AH.pil_crop(img, box, S)
        assert np.array_equal(got, want), (hw, S, box, int(np.abs(got.astype(int) - want).max()))


def test_full_box_tables_at_224():
    img = SOURCES[(301, 457)]
    for box in AH.with_flips([(0, 0, 301, 457), (301 - 224, 457 - 224, 224, 224), (3, 9, 224, 150)]):
        assert np.array_equal(AH.apply_full_box_tables(img, box, 224), AH.pil_crop(img, box, 224)), box


def test_crop_ksize_is_the_table_builders():
    from mmr_amd import preprocess as P
    for S in (224, 64, 30, 336):
        sizes = [1, 2, 3, 4, S - 1, S, S + 1, 2 * S, 2 * S + 1, 333, 1000, 4000]
        want = [(P.resample_tables(n, S, 0, S)[2]) for n in sizes]
        got = (P.crop_ksize(np.array(sizes), S) + 3) // 4 * 4
        assert got.tolist() == want, S


# ------------------------------------------------------------------ the sampler

def _draw(sizes, seed=0, **kw):
    from mmr_amd import random_resized_crop_params
    return random_resized_crop_params(sizes, generator=torch.Generator().manual_seed(seed), **kw).numpy().astype(np.int64)


MIXED = [(480, 640), (640, 480), (500, 500), (37, 41), (224, 224), (300, 400), (1, 1), (2, 3), (10, 1000), (1000, 10),
         (1200, 1600), (75, 100)] * 50


def test_boxes_lie_inside_their_images():
    sz = np.array(MIXED)
    b = _draw(MIXED, seed=3)
    assert b.shape == (len(MIXED), 5) and b.dtype == np.int64
    assert (b[:, 2] >= 1).all() and (b[:, 3] >= 1).all()
    assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all()
    assert (b[:, 0] + b[:, 2] <= sz[:, 0]).all() and (b[:, 1] + b[:, 3] <= sz[:, 1]).all()
    assert set(np.unique(b[:, 4])) <= {0, 1}
    from mmr_amd import random_resized_crop_params
    assert random_resized_crop_params(MIXED, generator=torch.Generator().manual_seed(3)).dtype == torch.int32


@pytest.mark.parametrize("scale, ratio", [((0.5, 1.0), (3 / 4, 4 / 3)), ((0.08, 1.0), (3 / 4, 4 / 3)), ((0.3, 0.6), (0.5, 2.0))])
def test_scale_and_ratio_hold_up_to_the_two_roundings(scale, ratio):
    # sources whose own aspect ratio lies inside the ratio range: their fallback is the whole image, which satisfies
    # the ratio bounds too, and the area bounds whenever scale[1] == 1; with scale[1] < 1 a try always succeeds at
    # these sizes (the largest target area fits at the source's own aspect ratio ... not at every ratio, so those
    # fallbacks are told apart below: a fallback box is the whole image)
    sizes = [(480, 640), (640, 480), (500, 500), (300, 400), (1200, 1600), (75, 100)] * 200
    sz = np.array(sizes, dtype=np.float64)
    b = _draw(sizes, seed=11, scale=scale, ratio=ratio).astype(np.float64)
    h, w, area = b[:, 2], b[:, 3], sz[:, 0] * sz[:, 1]
    whole = (h == sz[:, 0]) & (w == sz[:, 1])
    tried = ~whole if scale[1] < 1.0 else np.ones(len(sizes), bool)
    assert tried.mean() > 0.95
    assert ((w + 0.5) * (h + 0.5) >= scale[0] * area)[tried].all()
    assert ((w - 0.5) * (h - 0.5) <= scale[1] * area)[tried].all()
    assert ((w + 0.5) / (h - 0.5) >= ratio[0])[tried].all()
    assert ((w - 0.5) / (h + 0.5) <= ratio[1])[tried].all()
    assert len(np.unique(b[:, :4], axis=0)) > len(sizes) // 2          # and they are random, not one box


def test_same_seed_same_boxes_other_seed_other_boxes():
    a, b, c = _draw(MIXED, seed=5), _draw(MIXED, seed=5), _draw(MIXED, seed=6)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)
    # the stream is consumed: a second call on the same generator draws new boxes
    from mmr_amd import random_resized_crop_params
    g = torch.Generator().manual_seed(5)
    first, second = random_resized_crop_params(MIXED, generator=g), random_resized_crop_params(MIXED, generator=g)
    assert np.array_equal(first.numpy(), a) and not torch.equal(first, second)


def test_flip_rate():
    sizes = [(480, 640)] * 2000
    assert _draw(sizes, p_flip=0.0)[:, 4].sum() == 0
    assert _draw(sizes, p_flip=1.0)[:, 4].sum() == 2000
    n = int(_draw(sizes, p_flip=0.5)[:, 4].sum())
    assert 800 <= n <= 1200, n


def test_fallbacks():
    for seed in range(5):
        b = _draw([(10, 1000), (1000, 10), (1, 1)], seed=seed)
        assert b[0, :4].tolist() == [0, 493, 10, 13]
        assert b[1, :4].tolist() == [493, 0, 13, 10]
        assert b[2, :4].tolist() == [0, 0, 1, 1]


def test_sampler_needs_a_generator_and_sane_ranges():
    from mmr_amd import random_resized_crop_params
    with pytest.raises(ValueError):
        random_resized_crop_params([(4, 4)])
    with pytest.raises(ValueError):
        random_resized_crop_params([(0, 4)], generator=torch.Generator())
    with pytest.raises(ValueError):
        random_resized_crop_params([(4, 4)], scale=(1.0, 0.5), generator=torch.Generator())


# ------------------------------------------------------------------ validation, before anything touches the device

@pytest.mark.parametrize("box", [
    (0, 0, 0, 5, 0), (0, 0, 5, 0, 0), (0, 0, -3, 5, 0),            # empty
    (-1, 0, 5, 5, 0), (0, -1, 5, 5, 0),                             # starts outside
    (0, 0, 21, 5, 0), (0, 0, 5, 31, 0), (16, 0, 5, 5, 0), (0, 26, 5, 5, 0),   # ends outside a 20 x 30 image
])
def test_augment_batch_rejects_bad_boxes_on_the_host(box):
    from mmr_amd import augment_batch
    imgs = [torch.zeros(20, 30, 3, dtype=torch.uint8), torch.zeros(40, 40, 3, dtype=torch.uint8)]   # CPU: the device check is unreachable
    good = (0, 0, 5, 5, 0)
    with pytest.raises(ValueError):
        augment_batch(imgs, torch.tensor([box, good], dtype=torch.int32), n_px=32)
    with pytest.raises(ValueError):
        augment_batch(imgs, torch.tensor([good, good, box], dtype=torch.int32), n_px=32, image_index=[1, 1, 0])


def test_augment_batch_rejects_malformed_arguments():
    from mmr_amd import augment_batch
    imgs = [torch.zeros(20, 30, 3, dtype=torch.uint8)]
    good = torch.tensor([[0, 0, 5, 5, 0]], dtype=torch.int32)
    with pytest.raises(ValueError):
        augment_batch(imgs, good.repeat(2, 1), n_px=32)                      # two boxes, one image, no image_index
    with pytest.raises(ValueError):
        augment_batch(imgs, good, n_px=32, image_index=[1])                  # no such image
    with pytest.raises(ValueError):
        augment_batch(imgs, good[:, :4], n_px=32)
    with pytest.raises(ValueError):
        augment_batch(imgs, good.float(), n_px=32)
    with pytest.raises(ValueError):
        augment_batch([torch.zeros(20, 30, 3)], good, n_px=32)               # not uint8
    with pytest.raises(RuntimeError):
        augment_batch(imgs, good, n_px=32)                                   # a good box on a CPU image: there is no CPU path


def test_descriptors_and_chunks():
    from mmr_amd import preprocess as P
    boxes = np.array([[0, 0, 10, 7, 0], [2, 3, 33, 200, 1], [0, 0, 1, 1, 0]], dtype=np.int64)
    sizes = np.array([[10, 7], [50, 300], [1, 1]], dtype=np.int64)
    desc, kmax, max_ch, max_cw, scratch = P.crop_descriptors(np.array([1 << 40, 2 << 40, 3 << 40]), sizes, boxes, 32)
    assert desc.shape == (3, 6) and desc.dtype == np.int64 and desc.nbytes == 3 * 48
    spans = [(h * 32 * 3 + 15) // 16 * 16 for h in (10, 33, 1)]
    assert desc[:, 1].tolist() == [0, spans[0], spans[0] + spans[1]] and scratch == sum(spans) + 16
    assert desc[1].view(np.int32)[4:].tolist() == [50, 300, 2, 3, 33, 200, 1, 0]
    assert (max_ch, max_cw) == (33, 200)
    assert kmax == (int(np.ceil(2 * 200 / 32)) * 2 + 1 + 3) // 4 * 4 == 28
    # chunks: consecutive, cover every crop, and respect the cap wherever more than one crop shares a chunk
    many = np.tile(boxes, (20, 1))
    per = (many[:, 2] * 32 * 3 + 15) // 16 * 16 + P.augment_tables_bytes(1, 32, 28)
    chunks = P._augment_chunks(many, 32, cap=3 * int(per.max()))
    assert chunks[0][0] == 0 and chunks[-1][1] == 60 and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    assert len(chunks) > 1 and all(int(per[s:e].sum()) <= 3 * int(per.max()) for s, e in chunks)
    assert P._augment_chunks(many, 32, cap=1) == [(i, i + 1) for i in range(60)]
