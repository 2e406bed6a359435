"""Shared by tests/test_augment_host.py and tests/test_augment_gpu.py: the Pillow reference of one augmented crop, the
numpy application of the product's full-box tables, the boxes the issue lists, and a deterministic image."""
import numpy as np
import torch
from PIL import Image

MEAN = np.array([0.48145466, 0.4578275, 0.40821073], np.float32)
STD = np.array([0.26862954, 0.26130258, 0.27577711], np.float32)
GUARD = 0xA5


def image(h, w, seed):
    """uint8 [h,w,3]: smooth gradients plus noise, so that neither clamp nor rounding is trivially satisfied."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 7) % 256], axis=2)
    noise = rng.integers(-60, 61, size=(h, w, 3))
    img = np.clip(base + noise, 0, 255).astype(np.uint8)
    img[rng.random((h, w)) < 0.05] = 255                       # saturated specks: bicubic overshoot has to clip
    img[rng.random((h, w)) < 0.05] = 0
    return img


def pil_crop(img, box, S):
    """The reference: crop, resize with Pillow's BICUBIC, then mirror when flipped -> uint8 [S,S,3]."""
    top, left, h, w, flip = (int(v) for v in box)
    out = Image.fromarray(img).crop((left, top, left + w, top + h)).resize((S, S), Image.BICUBIC)
    if flip:
        out = out.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(out)


def normalise(u8, dtype=torch.float32):
    """ToTensor (x/255 in fp32) then Normalize ((x-mean)/std in fp32), as oracle/preprocess_ref.preprocess; [..,S,S,3] ->
    [..,3,S,S]."""
    x = torch.from_numpy(np.ascontiguousarray(u8)).movedim(-1, -3).to(torch.float32).div(255)
    y = x.sub(torch.from_numpy(MEAN).view(3, 1, 1)).div(torch.from_numpy(STD).view(3, 1, 1))
    return y.to(dtype)


def apply_full_box_tables(img, box, S):
    """Numpy application (int64 sums) of resample_tables(w, S, 0, S) / (h, S, 0, S) to the crop WINDOW, the horizontal
    table's rows reversed on flip: what the device kernels compute."""
    from mmr_amd import preprocess as P
    top, left, h, w, flip = (int(v) for v in box)
    hb, hc, _ = P.resample_tables(w, S, 0, S)
    vb, vc, _ = P.resample_tables(h, S, 0, S)
    if flip:
        hb, hc = hb[::-1], hc[::-1]
    half = 1 << (P.PRECISION_BITS - 1)
    src = img[top:top + h, left:left + w].astype(np.int64)
    tmp = np.zeros((h, S, 3), np.int64)
    for x in range(S):
        x0, n = hb[x]
        acc = half + (src[:, x0:x0 + n, :] * hc[x, :n, None].astype(np.int64)).sum(axis=1)
        tmp[:, x, :] = np.clip(acc >> P.PRECISION_BITS, 0, 255)
    out = np.zeros((S, S, 3), np.uint8)
    for y in range(S):
        y0, n = vb[y]
        acc = half + (tmp[y0:y0 + n] * vc[y, :n, None, None].astype(np.int64)).sum(axis=0)
        out[y] = np.clip(acc >> P.PRECISION_BITS, 0, 255)
    return out


def boxes_for(H, W, S):
    """(top, left, h, w) of the cases the bytes-vs-Pillow checks list, for an H x W source and output size S; the boxes
    that do not fit the source are left out (a 64x64 source has no room for h != S at w == S == 64 ... it has: h < S)."""
    hs, ws = min(H, 40), min(W, 52)
    cases = [
        (0, 0, H, W),                                  # the whole image
        (0, 0, hs, ws), (0, W - ws, hs, ws),           # the four corners
        (H - hs, 0, hs, ws), (H - hs, W - ws, hs, ws), # ... bottom-right: the over-read case
        (0, 0, 1, W), (H - 1, 0, 1, W),                # one pixel high
        (0, 0, H, 1), (0, W - 1, H, 1),                # one pixel wide
    ]
    if S <= W and S <= H:
        h_other = S - 7 if S > 7 else S + 1
        if h_other <= H:
            cases += [(H - h_other, W - S, h_other, S), (H - S, W - h_other, S, h_other)]   # w == S, h != S and the reverse
        cases.append((H - S, W - S, S, S))             # w == h == S
    if H >= 37 + 5 and W >= 41 + 3:
        cases.append((5, 3, 37, 41))                   # the upscaling crop, 37 x 41 -> 64
    return cases


def with_flips(cases):
    return [c + (f,) for c in cases for f in (0, 1)]
