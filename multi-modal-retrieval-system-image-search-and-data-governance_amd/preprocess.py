"""On-device CLIP preprocessing: bicubic resize of the shorter side, centre crop, /255, normalise.

The step immediately before ``encode_image``.  The reference gets it
from ``clip.load``'s ``preprocess`` -- torchvision ``Resize(n_px, BICUBIC)`` -> ``CenterCrop(n_px)`` ->
``ToTensor`` -> ``Normalize(mean, std)`` on a PIL image (use sites code/search_image.py:127,155;
constants code/custom.py:28).  The resize inside that is Pillow's ``Image.resize(..., BICUBIC)``:
8-bit fixed-point separable convolution, horizontal pass then vertical pass, each rounded back to
uint8 (Pillow src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
ImagingResampleHorizontal_8bpc / Vertical_8bpc).  That is integer/byte arithmetic, so the device
path reproduces it BIT-EXACTLY: the coefficient tables are built here on the host with the same
double-precision steps Pillow takes, and csrc/preprocess.hip applies them in int32.

Only the crop window is computed (same pixels as resize-then-crop, less work).
"""
import math
from functools import lru_cache
from typing import Sequence, Tuple

import numpy as np
import torch

from . import _lib

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 32 - 8 - 2      # Pillow Resample.c


def _bicubic(x: float) -> float:
    a = -0.5                      # Pillow's bicubic_filter
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    if -3.0 <= x < 3.0:           # Pillow's lanczos_filter: truncated sinc
        return _sinc(x) * _sinc(x / 3)
    return 0.0


_FILTERS = {"bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}      # name -> (weight, support), Pillow's struct filter


@lru_cache(maxsize=2048)
def resample_tables(in_size: int, out_size: int, first: int, count: int,
                    filter: str = "bicubic") -> Tuple[np.ndarray, np.ndarray, int]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for outputs [first, first+count) of a
    full-box resize in_size -> out_size with ``filter`` ("bicubic", or "lanczos": the perceptual hashes' resize).
    Returns (bounds int32[count,2] = (xmin, taps), coeffs int32[count, ksize], ksize); ksize is Pillow's, rounded up to
    a multiple of 4 (zero taps).  Cached per argument tuple: image sizes repeat."""
    if filter not in _FILTERS:
        raise ValueError(f"resample_tables: filter {filter!r}, expected one of {sorted(_FILTERS)}")
    weight, filter_support = _FILTERS[filter]
    scale = float(np.float32(in_size) - np.float32(0.0)) / out_size      # (double)(in1 - in0) / outSize, box is float
    filterscale = max(scale, 1.0)
    support = filter_support * filterscale                               # bicubic 2, lanczos 3
    ksize = int(math.ceil(support)) * 2 + 1
    ksize = (ksize + 3) // 4 * 4          # rows padded with zero taps to whole groups of 4: the kernels read 4 taps per load
    bounds = np.zeros((count, 2), np.int32)
    coeffs = np.zeros((count, ksize), np.int32)
    ss = 1.0 / filterscale
    for j in range(count):
        xx = first + j
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = [weight((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        for x, w in enumerate(k):
            coeffs[j, x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
        bounds[j] = (xmin, xmax)
    # the kernels multiply with the 24-bit integer multiplier: |coefficient| <= 2^22 * |weight|, |weight| <= ~1.2 for bicubic, <= 1 for lanczos
    assert int(np.abs(coeffs).max(initial=0)) < (1 << 23), "resample coefficient outside the 24-bit multiplier's range"
    return bounds, coeffs, ksize


def resize_geometry(h: int, w: int, n_px: int):
    """torchvision Resize(int) + CenterCrop(int) geometry: shorter side -> n_px, the other
    int(n_px * long / short); crop offsets int(round((size - n_px) / 2.0)) (Python round)."""
    if w <= h:
        nw, nh = n_px, int(n_px * h / w)
    else:
        nh, nw = n_px, int(n_px * w / h)
    top = int(round((nh - n_px) / 2.0))
    left = int(round((nw - n_px) / 2.0))
    return nh, nw, top, left


_table_cache = {}


def _device_tables(h, w, n_px, device):
    key = (h, w, n_px, str(device))
    hit = _table_cache.get(key)
    if hit is not None:
        return hit
    nh, nw, top, left = resize_geometry(h, w, n_px)
    hb, hc, hk = resample_tables(w, nw, left, n_px)       # horizontal: columns of the crop window
    vb, vc, vk = resample_tables(h, nh, top, n_px)        # vertical: rows of the crop window
    row0 = int(vb[:, 0].min())
    row1 = int((vb[:, 0] + vb[:, 1]).max())               # input rows the vertical pass touches
    t = dict(hb=torch.from_numpy(hb).to(device), hc=torch.from_numpy(hc).to(device), hk=hk,
             vb=torch.from_numpy(vb).to(device), vc=torch.from_numpy(vc).to(device), vk=vk, row0=row0, row1=row1)
    if len(_table_cache) > 512:
        _table_cache.clear()
    _table_cache[key] = t
    return t


@torch.no_grad()
def preprocess_image(img_u8: torch.Tensor, n_px: int = 224, out: torch.Tensor = None,
                     out_dtype: torch.dtype = torch.float32, mean: Sequence[float] = CLIP_MEAN,
                     std: Sequence[float] = CLIP_STD, return_u8: bool = False):
    """uint8 RGB image [H,W,3] on the GPU -> normalised [3,n_px,n_px] (fp32 or bf16).

    Equals ``Normalize(ToTensor(CenterCrop(Resize(PIL image))))`` bit for bit in the uint8 stage and in
    fp32 arithmetic after it.  ``return_u8`` also returns the resized+cropped uint8 [n_px,n_px,3].
    """
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3:
        raise ValueError(f"expected a uint8 [H,W,3] tensor, got {img_u8.dtype} {tuple(img_u8.shape)}")
    if not img_u8.is_cuda:
        raise RuntimeError("image must live on the GPU (there is no CPU path); upload the decoded bytes first")
    img_u8 = img_u8.contiguous()
    h, w = int(img_u8.shape[0]), int(img_u8.shape[1])
    dev = img_u8.device
    t = _device_tables(h, w, n_px, dev)
    rows = t["row1"] - t["row0"]
    tmp = torch.empty(rows, n_px, 3, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(3, n_px, n_px, dtype=out_dtype, device=dev)
    u8 = torch.empty(n_px, n_px, 3, dtype=torch.uint8, device=dev) if return_u8 else None
    L = _lib.lib()
    _lib.check(L.mmr_preprocess_image(img_u8.data_ptr(), h, w, n_px, t["row0"], rows,
                                      t["hb"].data_ptr(), t["hc"].data_ptr(), t["hk"],
                                      t["vb"].data_ptr(), t["vc"].data_ptr(), t["vk"],
                                      float(mean[0]), float(mean[1]), float(mean[2]),
                                      float(std[0]), float(std[1]), float(std[2]),
                                      tmp.data_ptr(), out.data_ptr(), _lib.dtype_code(out.dtype), _lib.ptr(u8),
                                      _lib.stream_ptr(dev)))
    return (out, u8) if return_u8 else out


def preprocess_batch(images: Sequence[torch.Tensor], n_px: int = 224, out_dtype: torch.dtype = torch.float32,
                     mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD) -> torch.Tensor:
    """A list of uint8 [H_i,W_i,3] GPU tensors (any sizes) -> [B,3,n_px,n_px] in ONE launch pair
    (mmr_preprocess_batch): per-image descriptors (pointers, geometry, coefficient tables) are built on
    the host and uploaded as one small array."""
    import numpy as np

    if not images:
        raise ValueError("empty batch")
    dev = images[0].device
    imgs, tabs, rows = [], [], []
    for im in images:
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError(f"expected uint8 [H,W,3] tensors, got {im.dtype} {tuple(im.shape)}")
        if not im.is_cuda:
            raise RuntimeError("images must live on the GPU (there is no CPU path)")
        im = im.contiguous()
        t = _device_tables(int(im.shape[0]), int(im.shape[1]), n_px, dev)
        imgs.append(im)
        tabs.append(t)
        rows.append(t["row1"] - t["row0"])
    B = len(imgs)
    offs = np.concatenate([[0], np.cumsum([r * n_px * 3 for r in rows])]).astype(np.int64)
    tmp = torch.empty(int(offs[-1]) + 16, dtype=torch.uint8, device=dev)
    desc = np.zeros((B, 9), dtype=np.int64)              # 6 pointers + 6 int32 packed as 3 int64 = 72 bytes
    for i, (im, t) in enumerate(zip(imgs, tabs)):
        desc[i, 0] = im.data_ptr()
        desc[i, 1], desc[i, 2] = t["hb"].data_ptr(), t["hc"].data_ptr()
        desc[i, 3], desc[i, 4] = t["vb"].data_ptr(), t["vc"].data_ptr()
        desc[i, 5] = tmp.data_ptr() + int(offs[i])
        ints = np.array([im.shape[0], im.shape[1], t["row0"], rows[i], t["hk"], t["vk"]], dtype=np.int32)
        desc[i, 6:9] = ints.view(np.int64)
    desc_d = torch.from_numpy(desc).to(dev)
    out = torch.empty(B, 3, n_px, n_px, dtype=out_dtype, device=dev)
    L = _lib.lib()
    _lib.check(L.mmr_preprocess_batch_ex(desc_d.data_ptr(), B, n_px, int(max(rows)), int(max(im.shape[1] for im in imgs)),
                                         float(mean[0]), float(mean[1]), float(mean[2]), float(std[0]), float(std[1]),
                                         float(std[2]), out.data_ptr(), _lib.dtype_code(out_dtype), _lib.stream_ptr(dev)))
    # descriptors, tables and images must outlive the launch: tie them to the output's lifetime
    out._mmr_keepalive = (desc_d, tmp, imgs)
    return out


class UniformBatchPreprocessor:
    """``preprocess`` for batches of SAME-SIZE images held as one uint8 tensor [B,H,W,3] on the GPU (a decoded video
    frame stack, a dataset stored at one resolution): the per-image descriptors differ only in two pointers, so they are
    built with three numpy array ops instead of a Python loop, staged in PINNED host memory and uploaded asynchronously --
    the call returns at once and can run on a side stream under the previous batch's ``encode_image``
    (``gallery.build_gallery_overlapped``).  Same kernels (``mmr_preprocess_batch``), same bytes as
    ``preprocess_image`` / Pillow.  One instance owns ``slots`` sets of buffers (descriptors, vertical-pass scratch,
    output pixels): slot ``i`` may be reused once the consumer of its previous output has finished."""

    def __init__(self, batch: int, height: int, width: int, n_px: int = 224, out_dtype: torch.dtype = torch.bfloat16,
                 device="cuda", slots: int = 2, mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD):
        self.B, self.H, self.W, self.S = int(batch), int(height), int(width), int(n_px)
        self.device = torch.device(device)
        self.mean, self.std, self.out_dtype = tuple(mean), tuple(std), out_dtype
        self.t = _device_tables(self.H, self.W, self.S, self.device)
        self.rows = self.t["row1"] - self.t["row0"]
        self.tmp_stride = self.rows * self.S * 3
        self.slots = []
        for _ in range(slots):
            self.slots.append(dict(
                desc_h=torch.zeros(self.B, 9, dtype=torch.int64).pin_memory(),
                desc_d=torch.zeros(self.B, 9, dtype=torch.int64, device=self.device),
                tmp=torch.empty(self.B * self.tmp_stride + 16, dtype=torch.uint8, device=self.device),
                out=torch.empty(self.B, 3, self.S, self.S, dtype=out_dtype, device=self.device)))
        ints = np.array([self.H, self.W, self.t["row0"], self.rows, self.t["hk"], self.t["vk"]], dtype=np.int32).view(np.int64)
        for sl in self.slots:                                  # everything but the image pointers is fixed per slot
            d = sl["desc_h"].numpy()
            d[:, 1], d[:, 2] = self.t["hb"].data_ptr(), self.t["hc"].data_ptr()
            d[:, 3], d[:, 4] = self.t["vb"].data_ptr(), self.t["vc"].data_ptr()
            d[:, 5] = sl["tmp"].data_ptr() + np.arange(self.B, dtype=np.int64) * self.tmp_stride
            d[:, 6:9] = ints

    @torch.no_grad()
    def __call__(self, images_u8: torch.Tensor, slot: int = 0) -> torch.Tensor:
        """[b,H,W,3] uint8 (b <= batch) -> the slot's pixel buffer [b,3,S,S]; enqueued on the CURRENT stream."""
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or tuple(images_u8.shape[1:]) != (self.H, self.W, 3):
            raise ValueError(f"expected uint8 [b,{self.H},{self.W},3], got {images_u8.dtype} {tuple(images_u8.shape)}")
        if not images_u8.is_cuda:
            raise RuntimeError("images must live on the GPU (there is no CPU path)")
        b = int(images_u8.shape[0])
        if not 1 <= b <= self.B:
            raise ValueError(f"batch {b} outside [1,{self.B}]")
        images_u8 = images_u8.contiguous()
        sl = self.slots[slot]
        key = (images_u8.data_ptr(), b)
        if sl.get("key") != key:               # same buffer as last time (a staging ring): the device descriptors still hold
            ev = sl.get("copied")
            if ev is not None:
                ev.synchronize()               # the previous upload FROM this pinned block must have left before it is rewritten
            sl["desc_h"].numpy()[:b, 0] = images_u8.data_ptr() + np.arange(b, dtype=np.int64) * (self.H * self.W * 3)
            sl["desc_d"][:b].copy_(sl["desc_h"][:b], non_blocking=True)
            sl["copied"] = torch.cuda.Event()
            sl["copied"].record()
            sl["key"] = key
        out = sl["out"][:b]
        L = _lib.lib()
        _lib.check(L.mmr_preprocess_batch_ex(sl["desc_d"].data_ptr(), b, self.S, int(self.rows), self.W, float(self.mean[0]),
                                             float(self.mean[1]), float(self.mean[2]), float(self.std[0]), float(self.std[1]),
                                             float(self.std[2]), out.data_ptr(), _lib.dtype_code(self.out_dtype),
                                             _lib.stream_ptr(self.device)))
        return out


# ------------------------------------------------------------------------------------------------------------------
# Train-time augmentation: RandomResizedCrop(n_px, BICUBIC) -> RandomHorizontalFlip -> ToTensor -> Normalize of the
# reference's few-shot loader (reference code/custom.py:24-29), from decoded images on the GPU.  The boxes are drawn on the
# host (a few numpy array operations per batch); the coefficient tables of every crop are built on the device
# (csrc/augment.hip) and applied by the crop-aware resample launches (csrc/preprocess.hip).  DESIGN.md section 3.
# ------------------------------------------------------------------------------------------------------------------
AUGMENT_TRIES = 10                         # torchvision's RandomResizedCrop.get_params
AUGMENT_WORKSPACE_CAP = 1 << 30            # bytes of tables + scratch one launch group may take; larger batches are split
AUGMENT_MAX_BATCH = 65535                  # crops per launch (the grid's second dimension)
AUGMENT_MAX_SIDE = 1 << 20                 # longest crop side the device tables are built for


def random_resized_crop_params(sizes, n_px_unused=None, scale=(0.5, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip: float = 0.5,
                               generator: torch.Generator = None) -> torch.Tensor:
    """Boxes of torchvision's ``RandomResizedCrop.get_params`` plus the coin of ``RandomHorizontalFlip(p_flip)`` for B
    images: ``sizes`` is [B,2] = (H, W); returns int32 [B,5] = (top, left, h, w, flip) on the host.  The output size does
    not enter the box (``n_px_unused`` is accepted and ignored).

    Per image, up to 10 tries: target area = H * W * U(scale), aspect ratio = exp(U(log ratio)),
    w = round(sqrt(area * r)), h = round(sqrt(area / r)); the first try with 0 < w <= W and 0 < h <= H is taken and its
    offset drawn uniformly over the positions that keep it inside.  After 10 failures the central crop clamped to the ratio
    range: W / H < min(ratio) -> full width, h = round(W / min); W / H > max(ratio) -> full height, w = round(H * max);
    otherwise the whole image; centred with ``// 2``.  The crop is flipped iff U(0, 1) < p_flip.

    Every variate comes from ``generator`` (a CPU ``torch.Generator``), as float64, in this fixed order:
    ``rand(B, 10)`` for the areas, ``rand(B, 10)`` for the log-ratios, ``rand(B, 2)`` for (top, left) -- an offset is
    ``floor(u * (H - h + 1))`` -- and ``rand(B)`` for the flips.  The same seed therefore gives the same boxes, whichever
    tries succeed.  The rule is torchvision's; the random STREAM is not (torchvision draws per image and per try from the
    global generator): equality with torchvision's own boxes for a seed is unpinned, torchvision being absent here."""
    if generator is None:
        raise ValueError("random_resized_crop_params: pass a CPU torch.Generator (the boxes are its function alone)")
    sz = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    if sz.size and sz.min() < 1:
        raise ValueError("random_resized_crop_params: image sizes must be >= 1")
    if not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
        raise ValueError(f"random_resized_crop_params: scale {scale} / ratio {ratio} must be positive and ordered")
    B = sz.shape[0]
    u_area = torch.rand(B, AUGMENT_TRIES, generator=generator, dtype=torch.float64).numpy()
    u_ratio = torch.rand(B, AUGMENT_TRIES, generator=generator, dtype=torch.float64).numpy()
    u_off = torch.rand(B, 2, generator=generator, dtype=torch.float64).numpy()
    u_flip = torch.rand(B, generator=generator, dtype=torch.float64).numpy()
    H, W = sz[:, 0], sz[:, 1]
    area = (H * W).astype(np.float64)[:, None] * (scale[0] + u_area * (scale[1] - scale[0]))
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    r = np.exp(lo + u_ratio * (hi - lo))
    w_try = np.rint(np.sqrt(area * r)).astype(np.int64)           # Python's round(): half to even
    h_try = np.rint(np.sqrt(area / r)).astype(np.int64)
    ok = (w_try > 0) & (w_try <= W[:, None]) & (h_try > 0) & (h_try <= H[:, None])
    first = ok.argmax(axis=1)
    hit = ok.any(axis=1)
    rows = np.arange(B)
    w, h = w_try[rows, first], h_try[rows, first]
    top = np.minimum(np.floor(u_off[:, 0] * (H - h + 1)).astype(np.int64), H - h)
    left = np.minimum(np.floor(u_off[:, 1] * (W - w + 1)).astype(np.int64), W - w)
    # the fallback: central crop, clamped to the ratio range
    in_ratio = W / H
    fw, fh = W.copy(), H.copy()
    narrow, wide = in_ratio < min(ratio), in_ratio > max(ratio)
    fh[narrow] = np.rint(W[narrow] / min(ratio)).astype(np.int64)
    fw[wide] = np.rint(H[wide] * max(ratio)).astype(np.int64)
    fw, fh = np.clip(fw, 1, W), np.clip(fh, 1, H)
    out = np.empty((B, 5), np.int32)
    out[:, 0] = np.where(hit, top, (H - fh) // 2)
    out[:, 1] = np.where(hit, left, (W - fw) // 2)
    out[:, 2] = np.where(hit, h, fh)
    out[:, 3] = np.where(hit, w, fw)
    out[:, 4] = u_flip < p_flip
    return torch.from_numpy(out)


def crop_ksize(in_size, n_px: int) -> np.ndarray:
    """Pillow's ksize of the full-box bicubic resize in_size -> n_px, for an array of sizes, with the fp32-box /
    double-division sequence ``resample_tables`` uses for ``scale``."""
    scale = np.asarray(in_size).astype(np.float32).astype(np.float64) / n_px
    return np.ceil(2.0 * np.maximum(scale, 1.0)).astype(np.int64) * 2 + 1


def _checked_boxes(images, boxes, image_index):
    """(boxes int64 [B,5], image_index int64 [B], sizes int64 [n,2]) after every host check of augment_batch."""
    if not images:
        raise ValueError("augment_batch: no images")
    for im in images:
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError(f"augment_batch: expected uint8 [H,W,3] tensors, got {im.dtype} {tuple(im.shape)}")
    bx = np.asarray(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes)
    if bx.ndim != 2 or bx.shape[1] != 5 or bx.dtype.kind not in "iu":
        raise ValueError(f"augment_batch: boxes must be integers [B,5] = (top, left, h, w, flip), got {bx.dtype} {bx.shape}")
    bx = bx.astype(np.int64)
    B = bx.shape[0]
    if image_index is None:
        if B != len(images):
            raise ValueError(f"augment_batch: {B} boxes for {len(images)} images; pass image_index to name each crop's source")
        idx = np.arange(B, dtype=np.int64)
    else:
        idx = np.asarray(image_index.cpu() if isinstance(image_index, torch.Tensor) else image_index).astype(np.int64).reshape(-1)
        if idx.shape[0] != B or (B and (idx.min() < 0 or idx.max() >= len(images))):
            raise ValueError(f"augment_batch: image_index must hold {B} indices into the {len(images)} images")
    sizes = np.array([[im.shape[0], im.shape[1]] for im in images], dtype=np.int64)
    H, W = sizes[idx, 0], sizes[idx, 1]
    top, left, h, w = bx[:, 0], bx[:, 1], bx[:, 2], bx[:, 3]
    bad = (h < 1) | (w < 1) | (top < 0) | (left < 0) | (top + h > H) | (left + w > W)
    if bad.any():
        b = int(np.flatnonzero(bad)[0])
        raise ValueError(f"augment_batch: box {b} = (top {top[b]}, left {left[b]}, h {h[b]}, w {w[b]}) is empty or outside its "
                         f"{H[b]}x{W[b]} image ({int(bad.sum())} such boxes)")
    if B and max(h.max(), w.max()) > AUGMENT_MAX_SIDE:
        raise ValueError(f"augment_batch: crop side above {AUGMENT_MAX_SIDE}")
    return bx, idx, sizes


def crop_descriptors(ptrs, sizes, boxes, n_px: int):
    """The ``mmr_crop_desc`` array of B crops, built with array operations: ``ptrs`` int64 [B] source addresses,
    ``sizes`` int64 [B,2] their (H, W), ``boxes`` int64 [B,5].  Returns (desc int64 [B,6] -- 48 bytes a crop --, kmax,
    max_ch, max_cw, scratch_bytes): the intermediate rows are packed, each crop's ``h * n_px * 3`` bytes rounded up to 16,
    plus 16 of slack; kmax is the batch's largest Pillow ksize rounded up to a multiple of 4."""
    B = boxes.shape[0]
    h, w = boxes[:, 2], boxes[:, 3]
    span = (h * n_px * 3 + 15) // 16 * 16
    offs = np.concatenate([[0], np.cumsum(span)]).astype(np.int64)
    desc = np.zeros((B, 6), dtype=np.int64)
    desc[:, 0] = ptrs
    desc[:, 1] = offs[:-1]
    ints = np.zeros((B, 8), dtype=np.int32)
    ints[:, 0], ints[:, 1] = sizes[:, 0], sizes[:, 1]
    ints[:, 2], ints[:, 3], ints[:, 4], ints[:, 5] = boxes[:, 0], boxes[:, 1], h, w
    ints[:, 6] = boxes[:, 4] != 0
    desc[:, 2:6] = ints.view(np.int64)
    kmax = int((max(crop_ksize(h, n_px).max(), crop_ksize(w, n_px).max()) + 3) // 4 * 4)
    return desc, kmax, int(h.max()), int(w.max()), int(offs[-1]) + 16


def augment_tables_bytes(B: int, n_px: int, kmax: int) -> int:
    """Bytes of the device tables of B crops: bounds int32 [B,2,n_px,2] then coefficients int32 [B,2,n_px,kmax]."""
    return B * 2 * n_px * (8 + 4 * kmax)


def _augment_chunks(boxes, n_px, cap):
    """Half-open ranges of crops whose tables + scratch stay within ``cap`` bytes (one crop always fits its own chunk)."""
    B = boxes.shape[0]
    kmax = int((max(crop_ksize(boxes[:, 2], n_px).max(), crop_ksize(boxes[:, 3], n_px).max()) + 3) // 4 * 4)
    per_crop = (boxes[:, 2] * n_px * 3 + 15) // 16 * 16 + augment_tables_bytes(1, n_px, kmax)
    ends = np.cumsum(per_crop)
    out, s = [], 0
    while s < B:
        base = int(ends[s - 1]) if s else 0
        e = int(np.searchsorted(ends, base + cap, side="right"))
        e = min(max(e, s + 1), s + AUGMENT_MAX_BATCH, B)
        out.append((s, e))
        s = e
    return out


@torch.no_grad()
def augment_batch(images: Sequence[torch.Tensor], boxes, n_px: int = 224, out_dtype: torch.dtype = torch.float32,
                  mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD, return_u8: bool = False,
                  image_index=None, workspace_cap: int = AUGMENT_WORKSPACE_CAP):
    """Crop, resize to n_px x n_px (Pillow's BICUBIC), flip and normalise B boxes of uint8 [H_i,W_i,3] GPU images ->
    [B,3,n_px,n_px] (fp32 or bf16): ``Normalize(ToTensor(RandomHorizontalFlip(RandomResizedCrop(...))))`` for the given
    boxes, bit for bit -- the uint8 stage equals ``img.crop(box).resize((n_px, n_px), BICUBIC)`` (then
    ``transpose(FLIP_LEFT_RIGHT)`` when flipped), the rest is the same fp32 operations.  ``boxes`` is integer [B,5] =
    (top, left, h, w, flip), as ``random_resized_crop_params`` returns; ``image_index[b]`` names the source of crop b
    (default: one crop per image, in order), so many crops may share a source.  ``return_u8`` also returns the uint8 crops
    [B,n_px,n_px,3].

    One tables launch (mmr_augment_tables) and one resample launch pair (mmr_augment_resample); nothing is built per crop
    on the host.  Tables and intermediate rows live in a workspace allocated here; a batch that would need more than
    ``workspace_cap`` bytes of it (1 GiB by default), or more than 65535 crops, is split into consecutive chunks, each its
    own launch group.  A box that is empty or not inside its image raises ``ValueError`` before anything touches the device."""
    bx, idx, sizes = _checked_boxes(images, boxes, image_index)
    if not 1 <= int(n_px) <= 4096:
        raise ValueError(f"augment_batch: n_px {n_px} outside [1,4096]")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"augment_batch: out_dtype {out_dtype}, expected float32 or bfloat16")
    for im in images:
        if not im.is_cuda:
            raise RuntimeError("images must live on the GPU (there is no CPU path); upload the decoded bytes first")
    n_px, B = int(n_px), bx.shape[0]
    dev = images[0].device
    imgs = [im.contiguous() for im in images]
    out = torch.empty(B, 3, n_px, n_px, dtype=out_dtype, device=dev)
    u8 = torch.empty(B, n_px, n_px, 3, dtype=torch.uint8, device=dev) if return_u8 else None
    if B == 0:
        return (out, u8) if return_u8 else out
    ptrs = np.array([im.data_ptr() for im in imgs], dtype=np.int64)[idx]
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    keep = [imgs]
    for s, e in _augment_chunks(bx, n_px, int(workspace_cap)):
        desc, kmax, max_ch, max_cw, scratch_bytes = crop_descriptors(ptrs[s:e], sizes[idx[s:e]], bx[s:e], n_px)
        tables_bytes = augment_tables_bytes(e - s, n_px, kmax)
        desc_d = torch.from_numpy(desc).to(dev)
        tables = torch.empty(tables_bytes, dtype=torch.uint8, device=dev)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        _lib.check(L.mmr_augment_tables(desc_d.data_ptr(), e - s, n_px, kmax, tables.data_ptr(), tables_bytes, st))
        _lib.check(L.mmr_augment_resample(desc_d.data_ptr(), e - s, n_px, kmax, max_ch, max_cw, tables.data_ptr(), tables_bytes,
                                          scratch.data_ptr(), scratch_bytes, float(mean[0]), float(mean[1]), float(mean[2]),
                                          float(std[0]), float(std[1]), float(std[2]), out[s:e].data_ptr(),
                                          _lib.dtype_code(out_dtype), _lib.ptr(u8[s:e] if return_u8 else None), st))
        keep.append((desc_d, tables, scratch))
    # descriptors, workspace and images must outlive the launches: tie them to the output's lifetime
    out._mmr_keepalive = keep
    return (out, u8) if return_u8 else out
