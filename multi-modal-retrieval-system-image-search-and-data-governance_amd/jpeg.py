"""Baseline JPEG files -> uint8 RGB tensors on the GPU, every byte Pillow's.

Every image flow of the reference starts with ``Image.open(f).convert("RGB")`` (code/search_image.py:127,155,
CLIP/lab3.py:28, tool/find_repeated_in_same_folder.py:12, tool/find_repeated.py:11-15).  ``decode_jpeg`` replaces that call
for the files the reference's own converter writes (tool/Image format conversion.py:62, baseline JPEG): the serial Huffman
stage runs on host threads (csrc/jpeg_host.cpp), dequantisation, the inverse DCT, chroma upsampling and the colour
conversion run in two HIP kernels (csrc/jpeg.hip) -- libjpeg-turbo's integer algorithms restated, so the pixels, and every
hash, preprocessed byte and feature computed from them, are those of Pillow.  What is outside the decoder's scope
(progressive files, CMYK, ...; ``include/mmr.h`` lists it) is reported per image and, by default, handed to Pillow.

And back: ``encode_jpeg`` writes uint8 pixels that are on the GPU as the baseline JPEG bytes Pillow's ``save`` writes (the
second half of this file; csrc/jpeg_encode.hip, csrc/jpeg_encode_host.cpp).
"""
import ctypes
import io
import os
from typing import Iterable, List, Optional

import numpy as np
import torch

from . import _lib

JPEG_OK, JPEG_UNSUPPORTED, JPEG_CORRUPT, JPEG_DECLINED = 0, 1, 2, 3
STATUS_NAMES = {JPEG_OK: "ok", JPEG_UNSUPPORTED: "unsupported", JPEG_CORRUPT: "corrupt", JPEG_DECLINED: "declined"}
MAX_THREADS = 16
_ON_UNSUPPORTED = ("pillow", "none", "raise")
_ENTROPY = ("host", "device")
SUBSEQ_BYTES = 128            # default subsequence size of the device Huffman stage
MAX_ROUNDS = 64               # default cap on its rounds; a row that needs more is declined and goes to the host stage


def _library(symbol: str = "mmr_jpeg_entropy_decode"):
    """The library, once it is seen to export ``symbol`` -- the entropy coder of the direction (decode, encode) the caller needs."""
    L = _lib.lib()
    if not hasattr(L, symbol):
        raise RuntimeError(f"this libmmr_hip.so has no JPEG {symbol.rsplit('_', 1)[1]}: rebuild it")
    return L


def _cuda_device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"device={device!r}: the decode runs on the GPU (there is no CPU path)")
    return dev


def _check_guard(guard):
    if guard < 0 or guard % 16:
        raise ValueError(f"guard={guard!r}: expected a non-negative multiple of 16")


def _offsets(spans) -> np.ndarray:
    """Where each of ``spans`` starts when they lie end to end: their exclusive prefix sum, int64."""
    off = np.zeros(len(spans), dtype=np.int64)
    np.cumsum(spans[:-1], out=off[1:])
    return off


def _workspace(L, nbytes: int, device, extra: int = 0) -> torch.Tensor:
    """The uint8 workspace a ``*_workspace_bytes`` call sized; 0 is how it refuses descriptors, with the reason in the last error."""
    if nbytes == 0:
        raise ValueError(L.mmr_last_error().decode())
    return torch.empty(nbytes + extra, dtype=torch.uint8, device=device)


def _component_blocks(info, flat, at: int):
    """The coefficients of the image ``info`` (an mmr_jpeg_info record) describes, which start at element ``at`` of ``flat``:
    one ``[blocks_c, 64]`` view per component."""
    out = []
    for n in [int(info["blocks0"]), int(info["blocks1"]), int(info["blocks2"])][:int(info["ncomp"])]:
        out.append(flat[at: at + n * 64].reshape(n, 64))
        at += n * 64
    return out


def _component_planes(desc_row, workspace):
    """The uint8 component planes of one descriptor row, padded to whole blocks, copied out of ``workspace``."""
    d = desc_row
    at, out = int(d["plane_off"]), []
    for c in range(int(d["ncomp"])):
        h = int(d["mcus_y"]) * (int(d["vmax"]) if c == 0 else 1) * 8
        w = int(d["mcus_x"]) * (int(d["hmax"]) if c == 0 else 1) * 8
        out.append(workspace[at: at + h * w].view(h, w).clone())
        at += h * w
    return out


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


def _check_options(device, on_unsupported, threads, entropy):
    dev = _cuda_device(device)
    if on_unsupported not in _ON_UNSUPPORTED:
        raise ValueError(f"on_unsupported={on_unsupported!r}: expected one of {_ON_UNSUPPORTED}")
    _check_threads(threads)
    if entropy not in _ENTROPY:
        raise ValueError(f"entropy={entropy!r}: expected one of {_ENTROPY}")
    return dev


def _check_subseq(subseq_bytes, max_rounds):
    for name, v in (("subseq_bytes", subseq_bytes), ("max_rounds", max_rounds)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise ValueError(f"{name}={v!r}: expected None or an int")
    S = SUBSEQ_BYTES if subseq_bytes is None else int(subseq_bytes)
    R = MAX_ROUNDS if max_rounds is None else int(max_rounds)
    if not 16 <= S <= 1024 or S & (S - 1):
        raise ValueError(f"subseq_bytes={subseq_bytes!r}: expected a power of two in 16..1024")
    if not 1 <= R <= 1024:
        raise ValueError(f"max_rounds={max_rounds!r}: expected 1..1024")
    return S, R


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
        return _component_blocks(self.infos[row], self.coef, int(self.coef_off[row]) // 2)


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
    coef_off = _offsets(nbytes)
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


class ScanBatch:
    """What ``mmr_jpeg_scan_prepare`` leaves, all on the host: ``infos``, ``desc`` (numpy records of mmr_jpeg_scan_desc),
    ``tables`` uint8 [B, MMR_JPEG_TABLE_BYTES], ``qt`` uint16 [B, 3, 64], ``prepared`` int32 [B] (the probe's status, or 3 for a
    scan longer than the device takes) and ``scan`` -- the rows' entropy-coded bytes packed at ``desc["bytes_off"]``, as a
    uint8 torch tensor (pinned when a staging buffer was given)."""

    def __init__(self, datas, stage=None):
        L = _library()
        B = len(datas)
        self.datas = datas
        self.infos = np.zeros(B, dtype=_lib.struct_dtype("mmr_jpeg_info"))
        self.desc = np.zeros(B, dtype=_lib.struct_dtype("mmr_jpeg_scan_desc"))
        self.tables = np.zeros((B, _lib.HEADER.constants["MMR_JPEG_TABLE_BYTES"]), dtype=np.uint8)
        self.qt = np.zeros((B, 3, 64), dtype=np.uint16)
        self.prepared = np.zeros(B, dtype=np.int32)
        ptrs = (ctypes.c_char_p * B)(*datas)
        sizes = np.array([len(d) for d in datas], dtype=np.int64)
        _lib.check(L.mmr_jpeg_scan_prepare(ptrs, sizes.ctypes.data, B, self.infos.ctypes.data, self.desc.ctypes.data, self.tables.ctypes.data,
                                           self.qt.ctypes.data, self.prepared.ctypes.data))
        ready = self.prepared == 0
        padded = np.where(ready, (self.desc["scan_bytes"] + 15) // 16 * 16, 0)
        total = max(int(padded.sum()), 16)
        if stage is None:
            self.scan = torch.empty(total, dtype=torch.uint8)
        else:
            stage.alloc((total + 1) // 2)
            self.scan = stage.buf.view(torch.uint8)[:total]
        flat = self.scan.numpy()
        for i in np.flatnonzero(ready):
            at, n = int(self.desc["bytes_off"][i]), int(self.desc["scan_bytes"][i])
            flat[at: at + n] = np.frombuffer(datas[i], dtype=np.uint8, count=n, offset=int(self.desc["scan_start"][i]))


class DeviceEntropyResult:
    """The device Huffman stage of one batch: buffers allocated at construction, ``upload()`` copies scan bytes, Huffman tables
    and descriptors (nothing else ever goes up), ``run()`` enqueues ``mmr_jpeg_entropy_decode_device`` on the current stream
    (no allocation, no copy: it can be captured in a graph).  ``coef_dev`` int16 holds the coefficients in the host stage's
    layout at ``coef_off`` (bytes); ``status``, ``rounds`` and ``subsequences`` (int32 [B]) are read back on first use after a
    run, which synchronises.  Status 3 (declined) asks for the host stage; ``ready`` marks the rows the device stage took on.
    Test aids: ``blocks(row)`` as on ``EntropyResult``; ``guard`` bytes (a multiple of 16) follow every coefficient span and
    ``fill`` presets the whole coefficient buffer."""

    def __init__(self, prep: ScanBatch, device, subseq_bytes: Optional[int] = None, max_rounds: Optional[int] = None, guard: int = 0,
                 fill: Optional[int] = None):
        L = _library()
        self.subseq_bytes, self.max_rounds = _check_subseq(subseq_bytes, max_rounds)
        _check_guard(guard)
        self.prep, self.device, self.datas, self.infos, self.qt = prep, torch.device(device), prep.datas, prep.infos, prep.qt
        self.ready = prep.prepared == 0
        B = len(self.ready)
        spans = np.where(self.ready, prep.infos["coef_bytes"] + int(guard), 0).astype(np.int64)
        self.coef_off = _offsets(spans)
        self.coef_bytes = int(spans.sum())
        self.desc_host = prep.desc.copy()
        self.desc_host["coef_off"] = self.coef_off
        self.coef_dev = torch.empty(max(self.coef_bytes // 2, 8), dtype=torch.int16, device=self.device)
        if fill is not None:
            self.coef_dev.fill_(int(fill))
        self.workspace = _workspace(L, L.mmr_jpeg_entropy_workspace_bytes(self.desc_host.ctypes.data, B, self.subseq_bytes), self.device)
        self.scan_dev = torch.empty(prep.scan.numel(), dtype=torch.uint8, device=self.device)
        self.tables_dev = torch.empty(prep.tables.size, dtype=torch.uint8, device=self.device)
        self.desc = torch.empty(self.desc_host.nbytes, dtype=torch.uint8, device=self.device)
        self.stat_dev = torch.zeros(B * 4, dtype=torch.int32, device=self.device)
        self._stat = None

    def upload(self):
        self.scan_dev.copy_(self.prep.scan, non_blocking=True)
        self.tables_dev.copy_(torch.from_numpy(self.prep.tables.reshape(-1)))
        self.desc.copy_(torch.from_numpy(self.desc_host.view(np.uint8).reshape(-1)))
        return self

    def run(self):
        self._stat = None
        _lib.check(_library().mmr_jpeg_entropy_decode_device(self.desc.data_ptr(), len(self.ready), self.scan_dev.data_ptr(), self.tables_dev.data_ptr(),
                                                            self.coef_dev.data_ptr(), self.stat_dev.data_ptr(), self.subseq_bytes, self.max_rounds,
                                                            self.workspace.data_ptr(), self.workspace.numel(), _lib.stream_ptr(self.device)))
        return self

    def _read_stat(self):
        if self._stat is None:
            self._stat = self.stat_dev.cpu().numpy().reshape(-1, 4)
        return self._stat

    @property
    def status(self):
        return self._read_stat()[:, 0]

    @property
    def rounds(self):
        return self._read_stat()[:, 1]

    @property
    def subsequences(self):
        return self._read_stat()[:, 2]

    def blocks(self, row: int):
        """Test aid: the coefficients of image ``row`` as one int16 ``[blocks_c, 64]`` array per component, read back."""
        at, n = int(self.coef_off[row]) // 2, int(self.infos[row]["coef_bytes"]) // 2
        return _component_blocks(self.infos[row], self.coef_dev[at: at + n].cpu().numpy(), 0)


def entropy_decode_device(files, device="cuda", subseq_bytes: Optional[int] = None, max_rounds: Optional[int] = None, guard: int = 0,
                          fill: Optional[int] = None) -> DeviceEntropyResult:
    """The Huffman stage on the device: probe every file on the host (headers only), upload the entropy-coded bytes and the
    Huffman tables, and decode one image per workgroup into the int16 coefficient layout of ``entropy_decode``.  A scan is cut
    into subsequences of ``subseq_bytes`` (a power of two in 16..1024, default 128) that lanes decode speculatively in rounds
    until their entry states agree -- JPEG streams self-synchronise -- at most ``max_rounds`` (1..1024, default 64) times; a
    final pass decodes under the host stage's rules.  A row is status 0 with exactly the host stage's coefficients, or keeps
    its probe status, or is 3 (declined: any irregularity, no convergence, a scan over 4 MiB) and belongs to the host stage.
    ``guard`` and ``fill`` are test aids (``DeviceEntropyResult``)."""
    dev = _cuda_device(device)
    _check_subseq(subseq_bytes, max_rounds)
    return DeviceEntropyResult(ScanBatch(_file_list(files)), dev, subseq_bytes, max_rounds, guard, fill).upload().run()


class JpegPlan:
    """One ``mmr_jpeg_decode_device`` call, prepared from the host stage's result (or from a ``DeviceEntropyResult``, whose
    coefficients are already on the device: then only the quantisation tables are uploaded): descriptors uploaded, the output
    buffer, the coefficient and table buffers and the workspace allocated.  ``upload()`` copies coefficients and tables to the device
    (asynchronously when they are pinned), ``run()`` enqueues the two kernels on the current stream; ``run()`` allocates and
    copies nothing, so it can be captured in a graph and replayed after ``coef_dev`` was overwritten in place.
    ``images()`` are views of ``out``, one uint8 ``[H, W, 3]`` per decoded row and None for the others.
    Test aids: ``guard`` bytes follow every image in ``out`` (``offsets[i]`` is where image i starts), ``fill`` presets the
    whole buffer, ``planes(row)`` reads the component planes back from the workspace."""

    def __init__(self, host, device, guard: int = 0, fill: Optional[int] = None):
        L = _library()
        self.host, self.device = host, torch.device(device)
        self.on_device = isinstance(host, DeviceEntropyResult)
        # a device result is planned before its status is read: every row the device stage took gets its planes and its output
        ok = self.ok = host.ready if self.on_device else host.status == 0
        B = len(ok)
        desc = np.zeros(B, dtype=_lib.struct_dtype("mmr_jpeg_desc"))
        inf = host.infos
        nblocks = np.where(ok, inf["blocks0"].astype(np.int64) + inf["blocks1"] + inf["blocks2"], 0)
        nruns = np.where(ok, (inf["H"].astype(np.int64) * inf["W"] + 3) // 4, 0)
        sizes = np.where(ok, inf["H"].astype(np.int64) * inf["W"] * 3, 0)
        slots = (sizes + int(guard) + 15) // 16 * 16
        self.offsets = _offsets(slots)
        self.sizes = sizes
        self.out = torch.empty(max(int(slots.sum()), 16), dtype=torch.uint8, device=self.device)
        if fill is not None:
            self.out.fill_(int(fill))
        desc["block_first"], desc["run_first"] = _offsets(nblocks), _offsets(nruns)
        desc["plane_off"] = desc["block_first"] * 64
        desc["coef_off"] = np.where(ok, host.coef_off, 0)
        desc["qt_off"] = np.arange(B, dtype=np.int64) * 384
        desc["out"] = self.out.data_ptr() + self.offsets
        for k in ("W", "H", "ncomp", "hmax", "vmax", "mcus_x", "mcus_y"):
            desc[k] = np.where(ok, inf[k], 0)
        self.total_blocks = int(nblocks.sum())
        self.coef_dev = host.coef_dev if self.on_device else torch.empty(max(host.coef_bytes // 2, 8), dtype=torch.int16, device=self.device)
        self.qt_dev = torch.empty(B * 192, dtype=torch.int16, device=self.device)
        self.workspace = _workspace(L, L.mmr_jpeg_workspace_bytes(desc.ctypes.data, B), self.device)
        self.desc_host = desc
        self.desc = torch.from_numpy(desc.view(np.uint8).reshape(B, -1)).to(self.device)

    def upload(self, coef: Optional[torch.Tensor] = None):
        """``coef``: the host coefficients as an int16 tensor (pinned for an asynchronous copy); default ``host.coef``."""
        n = 0 if self.on_device else self.host.coef_bytes // 2       # a device result's coefficients never left the device
        if n:
            src = torch.from_numpy(self.host.coef) if coef is None else coef
            self.coef_dev[:n].copy_(src[:n], non_blocking=True)
        self.qt_dev.copy_(torch.from_numpy(self.host.qt.view(np.int16).reshape(-1)), non_blocking=False)
        return self

    def run(self):
        if self.total_blocks:
            _lib.check(_library().mmr_jpeg_decode_device(self.desc.data_ptr(), len(self.ok), self.coef_dev.data_ptr(),
                                                         self.qt_dev.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(),
                                                         _lib.stream_ptr(self.device)))
        return self

    def images(self):
        out = []
        for i, ok in enumerate(self.ok):
            if not ok:
                out.append(None)
                continue
            h, w, at = int(self.host.infos[i]["H"]), int(self.host.infos[i]["W"]), int(self.offsets[i])
            out.append(self.out[at: at + h * w * 3].view(h, w, 3))
        return out

    def planes(self, row: int):
        """Test aid: the uint8 component planes of image ``row`` after ``run()``, padded to whole blocks, copied out of the workspace."""
        return _component_planes(self.desc_host[row], self.workspace)


def _pillow_rgb(data: bytes, device) -> torch.Tensor:
    from PIL import Image

    with Image.open(io.BytesIO(data)) as im:
        return torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8)).to(device)


def _finish_lists(imgs, status, datas, device, on_unsupported: str, return_status: bool):
    for i in np.flatnonzero(status != 0):
        if on_unsupported == "raise":
            raise ValueError(f"files[{i}] is {STATUS_NAMES[int(status[i])]} for the device decoder (status {int(status[i])})")
        if on_unsupported == "pillow":
            imgs[i] = _pillow_rgb(datas[i], device)
    return (imgs, status.copy()) if return_status else imgs


def _finish(plan: JpegPlan, on_unsupported: str, return_status: bool):
    return _finish_lists(plan.images(), plan.host.status, plan.host.datas, plan.device, on_unsupported, return_status)


def _decode_on_device(prep, dev, on_unsupported, return_status, threads):
    """entropy="device": entropy kernel, the two decode kernels, then the status; declined rows go through the host stage."""
    res = DeviceEntropyResult(prep, dev).upload().run()
    plan = JpegPlan(res, dev).upload().run()
    status = res.status.copy()
    imgs = plan.images()
    redo = np.flatnonzero(status == JPEG_DECLINED)
    if redo.size:
        host = entropy_decode([prep.datas[i] for i in redo], threads)
        again = JpegPlan(host, dev).upload().run().images()
        for j, i in enumerate(redo):
            imgs[i], status[i] = again[j], host.status[j]
    return _finish_lists(imgs, status, prep.datas, dev, on_unsupported, return_status)


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


def decode_jpeg(files, device="cuda", on_unsupported: str = "pillow", return_status: bool = False, threads: Optional[int] = None,
                entropy: str = "host"):
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
    per 256 images.

    ``entropy="device"`` runs the Huffman stage on the GPU as well (``entropy_decode_device``): only the compressed scan
    bytes and the Huffman tables are uploaded, one workgroup decodes one image.  Rows the device stage declines (any
    irregularity in the scan) are decoded by the host stage afterwards, so images and statuses are those of
    ``entropy="host"`` in every case.  Measured in one later run on the same files (same profile, keys e_ and f_): the device
    entropy stage alone 3.33 ms per 256 files (77.0 k images/s, 5 to 10 rounds per image), ``decode_jpeg_batches`` end to end
    42.9 k images/s with ``entropy="device"`` against 27.2 k images/s with ``"host"`` in that run.  The default stays ``"host"``."""
    dev = _check_options(device, on_unsupported, threads, entropy)
    datas = _file_list(files)
    if entropy == "device":
        return _decode_on_device(ScanBatch(datas), dev, on_unsupported, return_status, threads)
    stage = _Staging()
    host = entropy_decode(datas, threads, stage.alloc)
    plan = JpegPlan(host, dev)
    plan.upload(stage.buf).run()
    return _finish(plan, on_unsupported, return_status)


def decode_jpeg_batches(batches, device="cuda", on_unsupported: str = "pillow", return_status: bool = False, threads: Optional[int] = None,
                        entropy: str = "host"):
    """``decode_jpeg`` over an iterable of batches, as a generator of its results: while the device decodes batch i, a worker
    thread runs the entropy stage of batch i + 1 (the library call releases the GIL).  Two pinned staging buffers take turns;
    the coefficient copies are asynchronous on the current stream.  With ``entropy="device"`` the worker thread only reads
    the headers and packs the scan bytes of batch i + 1 into the staging buffer."""
    dev = _check_options(device, on_unsupported, threads, entropy)
    if isinstance(batches, (bytes, str, os.PathLike)) or not isinstance(batches, Iterable):
        raise ValueError("batches must be an iterable of lists of files")

    def gen():
        from concurrent.futures import ThreadPoolExecutor

        stages = (_Staging(), _Staging())

        def host_stage(batch, stage):
            if entropy == "device":
                return ScanBatch(_file_list(batch), stage)
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
                if entropy == "device":
                    result = _decode_on_device(host, dev, on_unsupported, return_status, threads)      # reads the status: the copies are done
                    yield result
                    i += 1
                    continue
                plan = JpegPlan(host, dev)
                plan.upload(stage.buf)
                stage.event = torch.cuda.Event()
                stage.event.record(torch.cuda.current_stream(dev))
                plan.run()
                yield _finish(plan, on_unsupported, return_status)
                i += 1

    return gen()


# ------------------------------------------------------------------------------------------------ encode
#
# The other direction: uint8 pixels on the GPU -> the bytes ``Image.fromarray(x).save(f, "JPEG", quality=q, subsampling=s)``
# writes, which is what the reference's converter calls (tool/Image format conversion.py:41-62).  Colour conversion,
# chroma downsampling, the forward DCT and the quantisation run in two kernels (csrc/jpeg_encode.hip), the Huffman coder
# and the framing on host threads (csrc/jpeg_encode_host.cpp).

JPEG_NO_ROOM = 4
STATUS_NAMES[JPEG_NO_ROOM] = "no room"
_SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), 0: (1, 1), 1: (2, 1), 2: (2, 2)}


_ENCODE = "mmr_jpeg_entropy_encode"       # what _library looks for on behalf of the encode


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _check_encode_options(quality, subsampling, restart_interval, background, threads):
    if not _is_int(quality) or not 1 <= quality <= 100:
        raise ValueError(f"quality={quality!r}: expected an int in 1..100")
    if isinstance(subsampling, bool) or not isinstance(subsampling, (str, int, np.integer)) or subsampling not in _SUBSAMPLING:
        raise ValueError(f"subsampling={subsampling!r}: expected '4:4:4', '4:2:2', '4:2:0' or Pillow's 0, 1, 2")
    if not _is_int(restart_interval) or not 0 <= restart_interval <= 65535:
        raise ValueError(f"restart_interval={restart_interval!r}: expected an int in 0..65535 (MCUs; 0: no restart markers)")
    if (isinstance(background, (str, bytes)) or not isinstance(background, Iterable) or len(tuple(background)) != 3
            or not all(_is_int(c) and 0 <= c <= 255 for c in background)):
        raise ValueError(f"background={background!r}: expected three ints in 0..255")
    _check_threads(threads)
    r, g, b = (int(c) for c in background)
    return int(quality), _SUBSAMPLING[subsampling], int(restart_interval), r | (g << 8) | (b << 16)


def _image_list(images) -> list:
    if isinstance(images, torch.Tensor):
        images = [images]
    elif isinstance(images, (str, bytes)) or not isinstance(images, Iterable):
        raise ValueError("images must be a uint8 CUDA tensor or a list of them")
    images = list(images)
    if not images:
        raise ValueError("empty batch")
    if len(images) > 65535:
        raise ValueError(f"{len(images)} images in one call; at most 65535 (encode_jpeg_batches takes any number of batches)")
    side = _lib.HEADER.constants["MMR_JPEG_MAX_SIDE"]
    for i, t in enumerate(images):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"images[{i}] must be a torch tensor, got {type(t).__name__}")
        if t.dtype != torch.uint8:
            raise ValueError(f"images[{i}] must be uint8, got {t.dtype}")
        if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] not in (3, 4)):
            raise ValueError(f"images[{i}] must be [H, W] (greyscale), [H, W, 3] (RGB) or [H, W, 4] (RGBA), got {tuple(t.shape)}")
        if not 1 <= t.shape[0] <= side or not 1 <= t.shape[1] <= side:
            raise ValueError(f"images[{i}]: sides must be 1..{side}, got {t.shape[0]} x {t.shape[1]}")
    for i, t in enumerate(images):
        if not t.is_cuda:
            raise RuntimeError(f"images[{i}] is on {t.device}: the encode runs on the GPU (there is no CPU path)")
        if t.device != images[0].device:
            raise ValueError(f"images[{i}] is on {t.device}, images[0] on {images[0].device}")
        if not t.is_contiguous():
            raise ValueError(f"images[{i}] is not contiguous")
    return images


def jpeg_quant_tables(quality: int):
    """libjpeg's quality scaling of the Annex K tables: (luma, chroma) as uint16 [64] numpy arrays in natural order."""
    luma, chroma = np.zeros(64, dtype=np.uint16), np.zeros(64, dtype=np.uint16)
    _lib.check(_library(_ENCODE).mmr_jpeg_quant_tables(int(quality) if _is_int(quality) else -1, luma.ctypes.data, chroma.ctypes.data))
    return luma, chroma


def encode_infos(shapes, sampling=(2, 2)) -> np.ndarray:
    """mmr_jpeg_info records for images of ``shapes`` -- (H, W) greyscale, (H, W, 3 or 4) colour at luma ``sampling``."""
    infos = np.zeros(len(shapes), dtype=_lib.struct_dtype("mmr_jpeg_info"))
    for i, s in enumerate(shapes):
        nc = 1 if len(s) == 2 else 3
        h, v = (1, 1) if nc == 1 else sampling
        mx, my = -(-int(s[1]) // (8 * h)), -(-int(s[0]) // (8 * v))
        chroma = mx * my if nc == 3 else 0
        infos[i] = (int(s[1]), int(s[0]), nc, h, v, mx, my, 0, mx * my * h * v, chroma, chroma, 0, (mx * my * h * v + 2 * chroma) * 128)
    return infos


def entropy_encode(coef: np.ndarray, coef_off, infos, qt, restart_interval: int = 0, threads: Optional[int] = None, capacities=None):
    """The host stage alone (no device): Huffman-code and frame B images on ``threads`` threads (default ``min(16, B)``).
    ``coef``: one flat int16 array holding every image's coefficients at ``coef_off`` (int64 [B], bytes) in the layout
    ``entropy_decode`` writes; ``infos``: mmr_jpeg_info records (``encode_infos``); ``qt``: uint16 [B, 3, 64].
    Returns ``(files, status)``: a list of ``bytes`` (None where status is not 0) and the int32 [B] status.  ``capacities``
    (int64 [B], a test aid) caps every file; by default a file that outgrows a first guess of one byte per coefficient is
    coded again with ``mmr_jpeg_encode_bound`` bytes of room."""
    _check_threads(threads)
    L = _library(_ENCODE)
    B = len(infos)
    coef_off = np.ascontiguousarray(coef_off, dtype=np.int64)
    qt = np.ascontiguousarray(qt, dtype=np.uint16)
    if coef.dtype != np.int16 or coef.ndim != 1 or not coef.flags.c_contiguous or qt.shape != (B, 3, 64) or coef_off.shape != (B,):
        raise ValueError("coef must be a contiguous one-dimensional int16 array, qt uint16 [B, 3, 64], coef_off int64 [B]")
    if B and int((coef_off + infos["coef_bytes"]).max()) > coef.nbytes:
        raise ValueError("a coefficient span ends past the coefficient array")
    T = int(threads) if threads else max(1, min(MAX_THREADS, B))
    files, status = [None] * B, np.zeros(B, dtype=np.int32)

    def code(rows, caps):
        offs = _offsets(caps)
        out = np.empty(max(int(caps.sum()), 1), dtype=np.uint8)
        sizes, st = np.zeros(len(rows), dtype=np.int64), np.zeros(len(rows), dtype=np.int32)
        inf, off, q = np.ascontiguousarray(infos[rows]), np.ascontiguousarray(coef_off[rows]), np.ascontiguousarray(qt[rows])
        _lib.check(L.mmr_jpeg_entropy_encode(coef.ctypes.data, off.ctypes.data, inf.ctypes.data, q.ctypes.data, len(rows), int(restart_interval),
                                             out.ctypes.data, offs.ctypes.data, caps.ctypes.data, sizes.ctypes.data, st.ctypes.data, T))
        for j, i in enumerate(rows):
            status[i] = st[j]
            files[i] = out[offs[j]: offs[j] + sizes[j]].tobytes() if st[j] == 0 else None

    rows = np.arange(B)
    if capacities is not None:
        code(rows, np.ascontiguousarray(capacities, dtype=np.int64))
        return files, status
    if B:
        code(rows, 1024 + infos["coef_bytes"].astype(np.int64) // 2)
        again = np.flatnonzero(status == JPEG_NO_ROOM)
        if again.size:
            code(again, np.array([L.mmr_jpeg_encode_bound(infos[i:].ctypes.data) for i in again], dtype=np.int64))
    return files, status


class JpegEncodePlan:
    """One ``mmr_jpeg_encode_device`` call over a list of uint8 CUDA tensors: descriptors uploaded, the quantisation tables,
    the coefficient buffer and the workspace allocated.  ``run()`` enqueues the two kernels on the current stream and
    allocates and copies nothing, so it can be captured in a graph and replayed after the pixels were overwritten in place
    (the descriptors hold the tensors' addresses; the plan keeps the tensors alive).  ``coef_dev`` holds int16 coefficients
    at ``coef_off`` (bytes) in the layout ``entropy_decode`` writes; ``infos`` and ``qt`` are what ``entropy_encode`` takes.
    Test aids: ``guard`` bytes (a multiple of 16) follow every plane span and every coefficient span, ``fill`` presets both
    buffers, ``planes(row)`` and ``blocks(row)`` read the two kernels' results back."""

    def __init__(self, images, quality: int = 95, subsampling="4:2:0", background=(255, 255, 255), guard: int = 0, fill: Optional[int] = None):
        quality, sampling, _, bg = _check_encode_options(quality, subsampling, 0, background, None)
        _check_guard(guard)
        self.images = _image_list(images)
        L = _library(_ENCODE)
        B = len(self.images)
        self.device = self.images[0].device
        self.infos = inf = encode_infos([tuple(t.shape) for t in self.images], sampling)
        nblocks = inf["blocks0"].astype(np.int64) + inf["blocks1"] + inf["blocks2"]
        luma, chroma = jpeg_quant_tables(quality)
        self.qt = np.broadcast_to(np.stack([luma, chroma, chroma])[None], (B, 3, 64))
        desc = np.zeros(B, dtype=_lib.struct_dtype("mmr_jpeg_encode_desc"))
        desc["block_first"] = _offsets(nblocks)
        desc["run_first"] = desc["block_first"] * 16
        desc["plane_off"] = _offsets(nblocks * 64 + int(guard))
        spans = nblocks * 128 + int(guard)
        desc["coef_off"] = _offsets(spans)
        self.coef_off, self.coef_bytes = desc["coef_off"].copy(), int(spans.sum())
        desc["src"] = [t.data_ptr() for t in self.images]
        desc["channels"] = [1 if t.dim() == 2 else t.shape[2] for t in self.images]
        desc["row_stride"] = [t.stride(0) for t in self.images]
        desc["background"] = bg
        for k in ("W", "H", "ncomp", "hmax", "vmax", "mcus_x", "mcus_y"):
            desc[k] = inf[k]
        self.total_blocks = int(nblocks.sum())
        self.workspace = _workspace(L, L.mmr_jpeg_encode_workspace_bytes(desc.ctypes.data, B), self.device, int(guard))
        self.coef_dev = torch.empty(self.coef_bytes // 2, dtype=torch.int16, device=self.device)
        if fill is not None:
            self.workspace.fill_(int(fill))
            self.coef_dev.view(torch.uint8).fill_(int(fill))
        self.qt_dev = torch.from_numpy(np.stack([luma, chroma, chroma]).view(np.int16).reshape(-1)).to(self.device)
        self.desc_host = desc
        self.desc = torch.from_numpy(desc.view(np.uint8).reshape(B, -1)).to(self.device)

    def run(self):
        _lib.check(_library(_ENCODE).mmr_jpeg_encode_device(self.desc.data_ptr(), len(self.images), self.qt_dev.data_ptr(), self.coef_dev.data_ptr(),
                                                            self.workspace.data_ptr(), self.workspace.numel(), self.total_blocks,
                                                            self.total_blocks * 16, _lib.stream_ptr(self.device)))
        return self

    def planes(self, row: int):
        """Test aid: the uint8 component planes of image ``row`` after ``run()``, padded to whole blocks, copied out of the workspace."""
        return _component_planes(self.desc_host[row], self.workspace)

    def blocks(self, row: int, coef: Optional[np.ndarray] = None):
        """Test aid: the coefficients of image ``row`` as one int16 numpy ``[blocks_c, 64]`` per component (``coef``: a host copy of ``coef_dev``)."""
        at, n = int(self.coef_off[row]) // 2, int(self.infos[row]["coef_bytes"]) // 2
        if coef is None:
            return _component_blocks(self.infos[row], self.coef_dev[at: at + n].cpu().numpy(), 0)
        return _component_blocks(self.infos[row], coef, at)


def _encode_finish(files, status):
    for i in np.flatnonzero(status != 0):
        raise RuntimeError(f"images[{i}]: the entropy stage answered status {int(status[i])} ({STATUS_NAMES.get(int(status[i]), '?')})")
    return files


def encode_jpeg(images, quality: int = 95, subsampling="4:2:0", restart_interval: int = 0, background=(255, 255, 255),
                threads: Optional[int] = None, return_coefficients: bool = False):
    """``Image.fromarray(x).save(f, "JPEG", quality=quality, subsampling=subsampling)`` for pixels that are on the GPU: a list
    of ``bytes``, one baseline JPEG file per image, every byte Pillow's (libjpeg-turbo's defaults: the slow integer DCT,
    the standard Huffman tables; DESIGN.md, "JPEG encode").

    ``images``: a uint8 CUDA tensor or a list of at most 65535, each ``[H, W, 3]`` (RGB), ``[H, W]`` (greyscale, written as a
    one-component file) or ``[H, W, 4]`` (RGBA, composited over ``background`` as ``Image.paste(img, mask=alpha)`` does --
    the reference converter's flow for RGBA sources), contiguous, sides 1..16384.  All images of a call share the options:
    ``quality`` 1..100, ``subsampling`` ``"4:4:4"``, ``"4:2:2"``, ``"4:2:0"`` or Pillow's 0 / 1 / 2 (ignored for
    greyscale), ``restart_interval`` in MCUs (0: none; Pillow's ``restart_marker_blocks``).  Colour conversion, downsampling,
    forward DCT and quantisation run in two kernels; the coefficients are downloaded and Huffman-coded on ``threads`` host
    threads (default ``min(16, B)``, at most 16).  The inputs are not modified.  ``return_coefficients`` adds a list with,
    per image, one int16 numpy ``[blocks_c, 64]`` array per component (natural order, padded block grid in raster order).

    Rate (profiles/jpeg_encode.json, tools/time_jpeg_encode.py; MI355X, 256 VGA images, quality 95, 4:2:0, one run):
    ``encode_jpeg_batches`` end to end 8.5 k images/s against 1.09 k images/s for the download plus ``Image.save`` on 16
    threads, a ratio of 7.8; the host Huffman stage (14.5 k images/s on its own) bounds it, the two kernels take 0.76 ms per
    256 images.

    Optimised Huffman tables, progressive output, metadata and custom tables are not offered."""
    quality, _, restart_interval, _ = _check_encode_options(quality, subsampling, restart_interval, background, threads)
    plan = JpegEncodePlan(images, quality, subsampling, background).run()
    coef = plan.coef_dev.cpu().numpy()
    files = _encode_finish(*entropy_encode(coef, plan.coef_off, plan.infos, plan.qt, restart_interval, threads))
    if return_coefficients:
        return files, [plan.blocks(i, coef) for i in range(len(files))]
    return files


def save_jpeg(images, paths, **options):
    """``encode_jpeg(images, **options)`` written to ``paths`` (one path per image); returns the byte counts."""
    if isinstance(images, torch.Tensor):
        images = [images]
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    images, paths = list(images), list(paths)
    if len(images) != len(paths):
        raise ValueError(f"{len(images)} images but {len(paths)} paths")
    for i, p in enumerate(paths):
        if not isinstance(p, (str, os.PathLike)):
            raise ValueError(f"paths[{i}] must be a path, got {type(p).__name__}")
    if options.get("return_coefficients"):
        raise ValueError("save_jpeg writes files; return_coefficients belongs to encode_jpeg")
    files = encode_jpeg(images, **options)
    for p, data in zip(paths, files):
        with open(p, "wb") as f:
            f.write(data)
    return [len(d) for d in files]


def encode_jpeg_batches(batches, quality: int = 95, subsampling="4:2:0", restart_interval: int = 0, background=(255, 255, 255),
                        threads: Optional[int] = None):
    """``encode_jpeg`` over an iterable of batches, as a generator of its results: while a worker thread Huffman-codes
    batch i (the library call releases the GIL), the kernels of batch i + 1 run on the current stream and its coefficients
    come down on a second stream into one of two pinned staging buffers."""
    quality, _, restart_interval, _ = _check_encode_options(quality, subsampling, restart_interval, background, threads)
    if isinstance(batches, (torch.Tensor, bytes, str)) or not isinstance(batches, Iterable):
        raise ValueError("batches must be an iterable of lists of images")

    def gen():
        from concurrent.futures import ThreadPoolExecutor

        stages = (_Staging(), _Staging())
        copy_stream = None

        def host_stage(plan, coef, done):
            done.synchronize()
            return _encode_finish(*entropy_encode(coef, plan.coef_off, plan.infos, plan.qt, restart_interval, threads))

        with ThreadPoolExecutor(max_workers=1) as pool:
            pending = None
            for i, batch in enumerate(batches):
                plan = JpegEncodePlan(batch, quality, subsampling, background).run()
                if copy_stream is None:
                    copy_stream = torch.cuda.Stream(plan.device)
                n = plan.coef_dev.numel()
                coef = stages[i % 2].alloc(n)[:n]                 # batch i - 2 used it; its result was yielded already
                copy_stream.wait_stream(torch.cuda.current_stream(plan.device))
                with torch.cuda.stream(copy_stream):
                    stages[i % 2].buf[:n].copy_(plan.coef_dev, non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(copy_stream)
                fut = pool.submit(host_stage, plan, coef, done)
                if pending is not None:
                    yield pending.result()
                pending = fut
            if pending is not None:
                yield pending.result()

    return gen()
