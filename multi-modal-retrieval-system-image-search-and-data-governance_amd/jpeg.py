"""Baseline JPEG files -> uint8 RGB tensors on the GPU, every byte Pillow's.

Every image flow of the reference starts with ``Image.open(f).convert("RGB")`` (code/search_image.py:127,155,
CLIP/lab3.py:28, tool/find_repeated_in_same_folder.py:12, tool/find_repeated.py:11-15).  ``decode_jpeg`` replaces that call
for the files the reference's own converter writes (tool/Image format conversion.py:62, baseline JPEG): the serial Huffman
stage runs on host threads (csrc/jpeg_host.cpp), dequantisation, the inverse DCT, chroma upsampling and the colour
conversion run in two HIP kernels (csrc/jpeg.hip) -- libjpeg-turbo's integer algorithms restated, so the pixels, and every
hash, preprocessed byte and feature computed from them, are those of Pillow.  What is outside the decoder's scope
(progressive files, CMYK, ...; ``include/mmr.h`` lists it) is reported per image and, by default, handed to Pillow.
"""
import ctypes
import io
import os
from typing import Iterable, List, Optional

import numpy as np
import torch

from . import _lib

JPEG_OK, JPEG_UNSUPPORTED, JPEG_CORRUPT = 0, 1, 2
STATUS_NAMES = {JPEG_OK: "ok", JPEG_UNSUPPORTED: "unsupported", JPEG_CORRUPT: "corrupt"}
MAX_THREADS = 16
_ON_UNSUPPORTED = ("pillow", "none", "raise")


def _library():
    L = _lib.lib()
    if not hasattr(L, "mmr_jpeg_entropy_decode"):
        raise RuntimeError("this libmmr_hip.so has no JPEG decode: rebuild it")
    return L


def _read(f, what: str) -> bytes:
    if isinstance(f, bytes):
        return f
    if isinstance(f, (str, os.PathLike)):
        with open(f, "rb") as fh:
            return fh.read()
    raise ValueError(f"{what} must be bytes or a path, got {type(f).__name__}")


def _file_list(files) -> List[bytes]:
    if isinstance(files, (bytes, str, os.PathLike)) or not isinstance(files, Iterable):
        raise ValueError("files must be a list of bytes objects or paths (one file: pass [file])")
    files = list(files)
    if not files:
        raise ValueError("empty batch")
    if len(files) > 65535:
        raise ValueError(f"{len(files)} files in one call; at most 65535 (decode_jpeg_batches takes any number of batches)")
    return [_read(f, f"files[{i}]") for i, f in enumerate(files)]


def _check_options(device, on_unsupported, threads):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"device={device!r}: the decode runs on the GPU (there is no CPU path)")
    if on_unsupported not in _ON_UNSUPPORTED:
        raise ValueError(f"on_unsupported={on_unsupported!r}: expected one of {_ON_UNSUPPORTED}")
    _check_threads(threads)
    return dev


def _check_threads(threads):
    if threads is not None and (isinstance(threads, bool) or not isinstance(threads, (int, np.integer)) or not 1 <= threads <= MAX_THREADS):
        raise ValueError(f"threads={threads!r}: expected None or an int in 1..{MAX_THREADS}")


def jpeg_info(file) -> dict:
    """The probe: the headers of one file (bytes or a path) up to its first scan, no decoding and no device.
    Returns ``dict(status, status_name, W, H, ncomp, hmax, vmax, mcus_x, mcus_y, blocks, coef_bytes)``: ``status`` 0, or
    1 (a valid file the device decoder does not cover) or 2 (corrupt) with only W and H filled as far as they were read;
    ``hmax x vmax`` is the luma sampling (1x1: 4:4:4, 2x1: 4:2:2, 2x2: 4:2:0), ``blocks`` the 8 x 8 blocks of each
    component's padded grid and ``coef_bytes`` the int16 coefficients the entropy stage writes for it."""
    data = _read(file, "file")
    info = np.zeros(1, dtype=_lib.struct_dtype("mmr_jpeg_info"))
    st = _library().mmr_jpeg_probe(data, len(data), info.ctypes.data)
    i = info[0]
    out = {k: int(i[k]) for k in ("W", "H", "ncomp", "hmax", "vmax", "mcus_x", "mcus_y", "coef_bytes")}
    out.update(status=int(st), status_name=STATUS_NAMES[int(st)], blocks=tuple(int(i[k]) for k in ("blocks0", "blocks1", "blocks2"))[:out["ncomp"]])
    return out


class EntropyResult:
    """What the host stage leaves: ``infos`` (numpy records of mmr_jpeg_info), ``status`` int32 [B], ``coef`` int16 (one
    flat buffer), ``coef_off`` int64 [B] byte offsets into it, ``qt`` uint16 [B, 3, 64], and the files themselves."""

    def __init__(self, datas, infos, status, coef, coef_off, qt, coef_bytes):
        self.datas, self.infos, self.status, self.coef, self.coef_off, self.qt, self.coef_bytes = datas, infos, status, coef, coef_off, qt, coef_bytes

    def blocks(self, row: int):
        """Test aid: the coefficients of image ``row`` as one int16 ``[blocks_c, 64]`` array per component."""
        i = self.infos[row]
        counts = [int(i["blocks0"]), int(i["blocks1"]), int(i["blocks2"])][:int(i["ncomp"])]
        at, out = int(self.coef_off[row]) // 2, []
        for n in counts:
            out.append(self.coef[at: at + n * 64].reshape(n, 64))
            at += n * 64
        return out


def entropy_decode(files, threads: Optional[int] = None, alloc=None) -> EntropyResult:
    """The host stage alone (no device): probe every file, then Huffman-decode the batch on ``threads`` threads
    (default ``min(16, B)``).  ``alloc(n)`` returns the int16 numpy array of at least n elements that receives the
    coefficients (the device path passes pinned memory); default ``np.empty``."""
    _check_threads(threads)
    datas = _file_list(files)
    L = _library()
    B = len(datas)
    infos = np.zeros(B, dtype=_lib.struct_dtype("mmr_jpeg_info"))
    for i, d in enumerate(datas):
        L.mmr_jpeg_probe(d, len(d), infos[i:].ctypes.data)
    nbytes = np.where(infos["status"] == 0, infos["coef_bytes"], 0).astype(np.int64)
    coef_off = np.zeros(B, dtype=np.int64)
    np.cumsum(nbytes[:-1], out=coef_off[1:])
    total = int(nbytes.sum())
    coef = (alloc or (lambda n: np.empty(n, dtype=np.int16)))(max(total // 2, 8))
    if coef.dtype != np.int16 or coef.ndim != 1 or coef.size < total // 2 or not coef.flags.c_contiguous:
        raise ValueError("alloc must return a contiguous one-dimensional int16 array of at least the size asked for")
    qt = np.zeros((B, 3, 64), dtype=np.uint16)
    status = np.zeros(B, dtype=np.int32)
    ptrs = (ctypes.c_char_p * B)(*datas)
    sizes = np.array([len(d) for d in datas], dtype=np.int64)
    _lib.check(L.mmr_jpeg_entropy_decode(ptrs, sizes.ctypes.data, B, infos.ctypes.data, coef.ctypes.data, coef_off.ctypes.data,
                                         qt.ctypes.data, status.ctypes.data, int(threads) if threads else min(MAX_THREADS, B)))
    return EntropyResult(datas, infos, status, coef, coef_off, qt, total)


class JpegPlan:
    """One ``mmr_jpeg_decode_device`` call, prepared from the host stage's result: descriptors uploaded, the output buffer,
    the coefficient and table buffers and the workspace allocated.  ``upload()`` copies coefficients and tables to the device
    (asynchronously when they are pinned), ``run()`` enqueues the two kernels on the current stream; ``run()`` allocates and
    copies nothing, so it can be captured in a graph and replayed after ``coef_dev`` was overwritten in place.
    ``images()`` are views of ``out``, one uint8 ``[H, W, 3]`` per decoded row and None for the others.
    Test aids: ``guard`` bytes follow every image in ``out`` (``offsets[i]`` is where image i starts), ``fill`` presets the
    whole buffer, ``planes(row)`` reads the component planes back from the workspace."""

    def __init__(self, host: EntropyResult, device, guard: int = 0, fill: Optional[int] = None):
        L = _library()
        self.host, self.device = host, torch.device(device)
        B = len(host.status)
        ok = host.status == 0
        desc = np.zeros(B, dtype=_lib.struct_dtype("mmr_jpeg_desc"))
        inf = host.infos
        nblocks = np.where(ok, inf["blocks0"].astype(np.int64) + inf["blocks1"] + inf["blocks2"], 0)
        nruns = np.where(ok, (inf["H"].astype(np.int64) * inf["W"] + 3) // 4, 0)
        sizes = np.where(ok, inf["H"].astype(np.int64) * inf["W"] * 3, 0)
        slots = (sizes + int(guard) + 15) // 16 * 16
        self.offsets = np.zeros(B, dtype=np.int64)
        np.cumsum(slots[:-1], out=self.offsets[1:])
        self.sizes = sizes
        self.out = torch.empty(max(int(slots.sum()), 16), dtype=torch.uint8, device=self.device)
        if fill is not None:
            self.out.fill_(int(fill))
        desc["block_first"][1:] = np.cumsum(nblocks[:-1])
        desc["run_first"][1:] = np.cumsum(nruns[:-1])
        desc["plane_off"] = desc["block_first"] * 64
        desc["coef_off"] = np.where(ok, host.coef_off, 0)
        desc["qt_off"] = np.arange(B, dtype=np.int64) * 384
        desc["out"] = self.out.data_ptr() + self.offsets
        for k in ("W", "H", "ncomp", "hmax", "vmax", "mcus_x", "mcus_y"):
            desc[k] = np.where(ok, inf[k], 0)
        self.total_blocks = int(nblocks.sum())
        self.coef_dev = torch.empty(max(host.coef_bytes // 2, 8), dtype=torch.int16, device=self.device)
        self.qt_dev = torch.empty(B * 192, dtype=torch.int16, device=self.device)
        nbytes = L.mmr_jpeg_workspace_bytes(desc.ctypes.data, B)
        if nbytes == 0:
            raise ValueError(L.mmr_last_error().decode())
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.desc_host = desc
        self.desc = torch.from_numpy(desc.view(np.uint8).reshape(B, -1)).to(self.device)

    def upload(self, coef: Optional[torch.Tensor] = None):
        """``coef``: the host coefficients as an int16 tensor (pinned for an asynchronous copy); default ``host.coef``."""
        n = self.host.coef_bytes // 2
        if n:
            src = torch.from_numpy(self.host.coef) if coef is None else coef
            self.coef_dev[:n].copy_(src[:n], non_blocking=True)
        self.qt_dev.copy_(torch.from_numpy(self.host.qt.view(np.int16).reshape(-1)), non_blocking=False)
        return self

    def run(self):
        if self.total_blocks:
            _lib.check(_library().mmr_jpeg_decode_device(self.desc.data_ptr(), len(self.host.status), self.coef_dev.data_ptr(),
                                                         self.qt_dev.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(),
                                                         _lib.stream_ptr(self.device)))
        return self

    def images(self):
        out = []
        for i, st in enumerate(self.host.status):
            if st != 0:
                out.append(None)
                continue
            h, w, at = int(self.host.infos[i]["H"]), int(self.host.infos[i]["W"]), int(self.offsets[i])
            out.append(self.out[at: at + h * w * 3].view(h, w, 3))
        return out

    def planes(self, row: int):
        """Test aid: the uint8 component planes of image ``row`` after ``run()``, padded to whole blocks, copied out of the workspace."""
        d = self.desc_host[row]
        at, out = int(d["plane_off"]), []
        for c in range(int(d["ncomp"])):
            h = int(d["mcus_y"]) * (int(d["vmax"]) if c == 0 else 1) * 8
            w = int(d["mcus_x"]) * (int(d["hmax"]) if c == 0 else 1) * 8
            out.append(self.workspace[at: at + h * w].view(h, w).clone())
            at += h * w
        return out


def _pillow_rgb(data: bytes, device) -> torch.Tensor:
    from PIL import Image

    with Image.open(io.BytesIO(data)) as im:
        return torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8)).to(device)


def _finish(plan: JpegPlan, on_unsupported: str, return_status: bool):
    imgs, host = plan.images(), plan.host
    for i in np.flatnonzero(host.status != 0):
        if on_unsupported == "raise":
            raise ValueError(f"files[{i}] is {STATUS_NAMES[int(host.status[i])]} for the device decoder (status {int(host.status[i])})")
        if on_unsupported == "pillow":
            imgs[i] = _pillow_rgb(host.datas[i], plan.device)
    return (imgs, host.status.copy()) if return_status else imgs


class _Staging:
    """A pinned int16 buffer that grows, and the event after which the copy out of it is done."""

    def __init__(self):
        self.buf, self.event = None, None

    def alloc(self, n: int) -> np.ndarray:
        if self.event is not None:
            self.event.synchronize()
            self.event = None
        if self.buf is None or self.buf.numel() < n:
            self.buf = torch.empty(max(n, 2 * (0 if self.buf is None else self.buf.numel())), dtype=torch.int16, pin_memory=True)
        return self.buf.numpy()


def decode_jpeg(files, device="cuda", on_unsupported: str = "pillow", return_status: bool = False, threads: Optional[int] = None):
    """``[Image.open(f).convert("RGB") for f in files]`` with the pixels on the GPU: a list of uint8 ``[H_i, W_i, 3]`` tensors,
    the type ``image_hashes``, ``find_image_duplicates``, ``augment_batch``, ``build_cache_model_augmented``,
    ``preprocess_batch`` and ``build_gallery_overlapped`` take.  Every byte equals Pillow's (libjpeg-turbo's defaults:
    the slow integer DCT and fancy upsampling) for any file an encoder wrote from 8-bit pixels ("JPEG decode").

    ``files``: a list of ``bytes`` objects or paths, at most 65535.  Baseline and extended-sequential Huffman files, greyscale
    or YCbCr at 4:4:4, 4:2:2 or 4:2:0, with or without restart markers, are decoded here: the entropy stage on ``threads`` host
    threads (default ``min(16, len(files))``, at most 16), everything after it in two kernels.  The others -- progressive,
    CMYK, corrupt: status 1 (unsupported) or 2 (corrupt) -- follow ``on_unsupported``: ``"pillow"`` decodes them with Pillow
    on the host and uploads the result, so the list is complete (Pillow raises for what it cannot read either); ``"none"``
    leaves None in their places; ``"raise"`` raises a ValueError that names the first.  ``return_status`` adds the int32
    ``[B]`` numpy status.  The tensors are views of one buffer.

    Rate (profiles/jpeg_decode.json, tools/time_jpeg_decode.py; MI355X, 256 VGA 4:2:0 quality-85 files, one run):
    ``decode_jpeg_batches`` end to end 27.6 k images/s against 2.2 k images/s for ``Image.open().convert("RGB")`` on 16
    threads plus the upload, a ratio of 12.7; the host entropy stage (31.9 k images/s) bounds it, the two kernels take 0.50 ms
    per 256 images."""
    dev = _check_options(device, on_unsupported, threads)
    datas = _file_list(files)
    stage = _Staging()
    host = entropy_decode(datas, threads, stage.alloc)
    plan = JpegPlan(host, dev)
    plan.upload(stage.buf).run()
    return _finish(plan, on_unsupported, return_status)


def decode_jpeg_batches(batches, device="cuda", on_unsupported: str = "pillow", return_status: bool = False, threads: Optional[int] = None):
    """``decode_jpeg`` over an iterable of batches, as a generator of its results: while the device decodes batch i, a worker
    thread runs the entropy stage of batch i + 1 (the library call releases the GIL).  Two pinned staging buffers take turns;
    the coefficient copies are asynchronous on the current stream."""
    dev = _check_options(device, on_unsupported, threads)
    if isinstance(batches, (bytes, str, os.PathLike)) or not isinstance(batches, Iterable):
        raise ValueError("batches must be an iterable of lists of files")

    def gen():
        from concurrent.futures import ThreadPoolExecutor

        stages = (_Staging(), _Staging())

        def host_stage(batch, stage):
            return entropy_decode(_file_list(batch), threads, stage.alloc)

        it = iter(batches)
        with ThreadPoolExecutor(max_workers=1) as pool:
            first = next(it, None)
            fut = None if first is None else pool.submit(host_stage, first, stages[0])
            i = 0
            while fut is not None:
                host = fut.result()
                nxt = next(it, None)
                fut = None if nxt is None else pool.submit(host_stage, nxt, stages[(i + 1) % 2])
                stage = stages[i % 2]
                plan = JpegPlan(host, dev)
                plan.upload(stage.buf)
                stage.event = torch.cuda.Event()
                stage.event.record(torch.cuda.current_stream(dev))
                plan.run()
                yield _finish(plan, on_unsupported, return_status)
                i += 1

    return gen()
