"""Preprocess at output sizes above one 256-pixel column block (ViT-L/14@336px and larger) vs the Pillow oracle.

The fast vertical pass gives one wave 4 pixels per lane, 256 pixels per row step; rows wider than that must be walked in
several column blocks.  n_px = 256 is the one-block control, 260 / 336 / 512 / 1000 need two to four blocks (S % 4 == 0:
the fast pass), 338 is not a multiple of 4 (the generic pass).  Every output buffer that the API lets the caller pass is
pre-filled with NaN, so a pixel the kernels never write cannot equal the oracle by luck."""
import numpy as np
import pytest
import torch

from test_preprocess import _img

pytestmark = pytest.mark.gpu

N_PX = [256, 260, 336, 338, 512, 1000]
SOURCES = {"landscape": (480, 640), "portrait": (640, 480), "tiny": (40, 33), "wide": (50, 7000), "odd-view": (301, 207)}

_oracle_cache = {}


def _source(name):
    h, w = SOURCES[name]
    return _img(h, w, seed=h * 5 + w)


def _oracle(name, n_px):
    """(u8 [n,n,3], fp32 [3,n,n]) of the CPU oracle; cached, the wide source at 1000 px resizes to 140000 x 1000."""
    from oracle import preprocess_ref
    key = (name, n_px)
    if key not in _oracle_cache:
        img = _source(name)
        _oracle_cache[key] = (preprocess_ref.preprocess_u8(img, n_px), preprocess_ref.preprocess(img, n_px))
    return _oracle_cache[key]


def _device_image(name, device):
    img = _source(name)
    if name != "odd-view":
        return torch.from_numpy(img).to(device)
    # bytes start at an odd address and end at the last byte of their allocation (as test_fast_preprocess_paths_edge_cases)
    n = img.size
    flat = torch.zeros(n + 1, dtype=torch.uint8, device=device)
    flat[1:] = torch.from_numpy(img).reshape(-1).to(device)
    view = flat[1:].view(img.shape)
    assert view.data_ptr() % 2 == 1
    return view


@pytest.mark.parametrize("n_px", N_PX)
def test_preprocess_image_large_sizes_bit_exact(device, n_px):
    from mmr_amd import preprocess as P
    for name in SOURCES:
        want_u8, want = _oracle(name, n_px)
        img = _device_image(name, device)
        out = torch.full((3, n_px, n_px), float("nan"), dtype=torch.float32, device=device)
        got, u8 = P.preprocess_image(img, n_px, out=out, return_u8=True)
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(u8.cpu().numpy(), want_u8), (name, n_px)
        got = got.cpu()
        assert not torch.isnan(got).any(), (name, n_px, "unwritten pixels, first column", int(torch.isnan(got).any(1).any(0).nonzero()[0]))
        assert torch.equal(got, want), (name, n_px)
        outb = torch.full((3, n_px, n_px), float("nan"), dtype=torch.bfloat16, device=device)
        P.preprocess_image(img, n_px, out=outb)
        assert torch.equal(outb.cpu(), want.bfloat16()), (name, n_px)


@pytest.mark.parametrize("n_px", [336, 1000])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_preprocess_batch_large_sizes_mixed_sources(device, n_px, dtype):
    """One launch pair for sources of five different shapes (the LDS-staged horizontal pass is sized for the widest)."""
    from mmr_amd import preprocess as P
    names = list(SOURCES)
    got = P.preprocess_batch([_device_image(nm, device) for nm in names], n_px, out_dtype=dtype)
    want = torch.stack([_oracle(nm, n_px)[1] for nm in names]).to(dtype)
    assert torch.equal(got.cpu(), want), n_px


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_uniform_batch_preprocessor_336(device, dtype):
    """The path build_gallery_overlapped takes for an @336px model, both slots, output buffers pre-filled with NaN."""
    from mmr_amd import preprocess as P
    from oracle import preprocess_ref
    H, W, n_px = 240, 320, 336
    same = np.stack([_img(H, W, seed=40 + s) for s in range(5)])
    want = torch.stack([preprocess_ref.preprocess(a, n_px) for a in same]).to(dtype)
    pre = P.UniformBatchPreprocessor(6, H, W, n_px, out_dtype=dtype, device=device, slots=2)
    dev_imgs = torch.from_numpy(same).to(device)
    for slot in (0, 1):
        pre.slots[slot]["out"].fill_(float("nan"))
        got = pre(dev_imgs, slot)
        assert torch.equal(got.cpu(), want), slot
