"""Recordings as they are stored: interleaved integer or float PCM, the data chunk of a WAV file, decoded on the GPU into the
planar float rows [S, T] that the batch classes and the Resampler read (pcm.hip, frt_pcm_*; the definition:
include/friture_hip.h, R2).

A PCM buffer is frames of `channels` interleaved little-endian samples; FORMATS names the sample formats.  Full scale is
[-1, 1): u8 (b - 128) 2^-7, s16 v 2^-15, s24 v 2^-23, s32 v 2^-31, f32 and f64 the value itself.  The float64 output is the
exact value, the float32 output one round-to-nearest-even of it.  The raw bytes go to the device once (host data in slabs
through page-locked memory); one kernel de-interleaves, selects channels, sign-extends and scales.  wav_info reads a WAV
header without the `wave` module (which refuses WAVE_FORMAT_EXTENSIBLE and float files on older interpreters); load_wav maps
the file, decodes it and brings it to SAMPLING_RATE.  There is no CPU fallback: decode_pcm goes to the HIP library."""
from __future__ import annotations

import ctypes
import operator
import os
import struct
import threading
from typing import NamedTuple

import numpy as np

from . import _batchio, _lib
from .constants import SAMPLING_RATE

FORMATS = {"u8": (0, 1), "s16": (1, 2), "s24": (2, 3), "s32": (3, 4), "f32": (4, 4), "f64": (5, 8)}      # name -> (code, bytes)
MAX_CHANNELS = 64
MAX_SELECT = 65535


class WavInfo(NamedTuple):
    fmt: str              # a key of FORMATS: the container decides
    channels: int
    rate: int
    n_frames: int         # whole frames present in the file
    data_offset: int      # of the first sample byte in the file
    valid_bits: int       # at most 8 * width; fewer are left-justified in the container, which decides the scale
    truncated: bool       # the data chunk's size was 0, 0xFFFFFFFF or more than the file holds


class Recording(NamedTuple):
    samples: object       # [S, T'] at the requested rate
    rate_in: int          # the file's rate
    info: WavInfo


def _check_format(fmt, channels):
    if not isinstance(fmt, str) or fmt not in FORMATS:
        raise ValueError(f"format {fmt!r} (one of {', '.join(FORMATS)})")
    if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"channels {channels!r} (1 .. {MAX_CHANNELS})")
    return FORMATS[fmt][0], FORMATS[fmt][1], int(channels)


def tile_frames(fmt, channels):
    """Frames per workgroup of the decode kernel (frt_pcm_tile_frames): a multiple of 64 whose raw bytes fit 32 KB."""
    code, _, channels = _check_format(fmt, channels)
    f = _lib.load().frt_pcm_tile_frames(code, channels)
    if f < 0:
        _lib.check(f)
    return f


def _dtype_name(d):
    try:
        name = str(d).split(".")[-1] if type(d).__module__.startswith("torch") else np.dtype(d).name
    except TypeError:
        name = repr(d)
    if name not in ("float32", "float64"):
        raise TypeError(f"dtype must be float32 or float64, got {d!r}")
    return name


def _bytes_of(data):
    """(1-D uint8 data, is_np): a CUDA uint8 tensor as it is, anything with the buffer protocol as a numpy view."""
    if type(data).__module__.startswith("torch"):
        import torch
        if not data.is_cuda or data.dtype != torch.uint8 or data.ndim != 1:
            raise TypeError(f"a tensor of PCM bytes is a 1-D CUDA uint8 tensor, got {data.dtype} {tuple(data.shape)} on {data.device}")
        return (data if data.stride(0) == 1 or data.numel() < 2 else data.contiguous()), False
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise TypeError(f"an array of PCM bytes is 1-D uint8, got {data.dtype} {data.shape}")
        return (data if data.size < 2 or data.strides[0] == 1 else np.ascontiguousarray(data)), True
    try:
        view = memoryview(data).cast("B")
    except TypeError as e:
        raise TypeError(f"PCM bytes: a numpy uint8 array, a buffer or a CUDA uint8 tensor, got {type(data).__name__}") from e
    return np.frombuffer(view, np.uint8), True


def decode_pcm(data, fmt, channels, select=None, start=0, count=None, dtype=np.float32, to=None, slab_bytes=None):
    """[len(select), count]: row s is channel select[s] of the frames start .. start + count - 1 of `data`, whole frames of
    `channels` interleaved samples of format `fmt` (1-D bytes at any address: a numpy uint8 array, np.memmap or any buffer, or a
    CUDA uint8 tensor).  select: channel indices in any order, repeats allowed (None: every channel in order).  The result is a
    numpy array for host data and a tensor for a tensor; to="cuda" gives a CUDA tensor from host data, the normal way into the
    chains: the float copy never exists on the host.  Host data goes up in slabs of at most slab_bytes (None: 64 MB); the
    result does not depend on it.  Calls from several threads share one set of staging buffers and run one after the other."""
    code, width, channels = _check_format(fmt, channels)
    data, is_np = _bytes_of(data)
    n_bytes = int(data.shape[0])
    if n_bytes % (channels * width):
        raise ValueError(f"{n_bytes} bytes are no whole number of frames of {channels} x {width} bytes")
    n_total = n_bytes // (channels * width)
    try:
        sel = np.arange(channels, dtype=np.int64) if select is None else np.array([operator.index(c) for c in select], np.int64)
    except TypeError as e:
        raise ValueError(f"select {select!r}: a sequence of integer channel indices") from e
    if not 1 <= sel.size <= MAX_SELECT:
        raise ValueError(f"{sel.size} selected channels (1 .. {MAX_SELECT})")
    if sel.min() < 0 or sel.max() >= channels:
        raise ValueError(f"select {sel.tolist()} of {channels} channels")
    sel = np.ascontiguousarray(sel, np.int32)
    start = int(start)
    count = n_total - start if count is None else int(count)
    if not (0 <= start <= n_total and 0 <= count <= n_total - start):
        raise ValueError(f"frames {start} .. {start + count} of {n_total}")
    name = _dtype_name(dtype)
    if to not in (None, "cuda"):
        raise ValueError(f"to={to!r} (None or 'cuda')")
    slab = 0 if slab_bytes is None else int(slab_bytes)
    if slab < 0:
        raise ValueError(f"slab_bytes {slab_bytes!r}")
    h, vp, S = _handle(), ctypes.c_void_p, int(sel.size)

    def call(y):
        _lib.check(h.lib.frt_pcm_decode(h.h, vp(_batchio.ptr(data)) if count else None, code, channels, n_total, start, count,
                                        vp(sel.ctypes.data), S, vp(_batchio.ptr(y)) if count else None, int(name == "float64"),
                                        max(count, 1), slab))

    if is_np and to is None:
        y = np.empty((S, count), name)
        with h.lock:
            _lib.check(h.lib.frt_pcm_set_stream(h.h, None))
            call(y)
        return y
    import torch
    with _batchio.null_stream(data, is_np) as dev:
        y = torch.empty((S, count), dtype=getattr(torch, name), device=dev)
        with h.lock:
            _lib.check(h.lib.frt_pcm_set_stream(h.h, None))
            call(y)
    return y


class _Handle:
    """One frt_pcm object: the page-locked slabs and the device staging of decode_pcm, kept from call to call and shared by every
    caller of the process.  A frt_pcm serves one call at a time, so calls from several threads take `lock` in turn."""

    def __init__(self):
        self.lock = threading.Lock()
        self.lib = _lib.init()
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.frt_pcm_create(ctypes.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.frt_pcm_destroy(self.h)
            self.h = ctypes.c_void_p()


_shared = None
_shared_lock = threading.Lock()


def _handle():
    global _shared
    with _shared_lock:
        if _shared is None:
            _shared = _Handle()
        return _shared


# ---- WAV files ------------------------------------------------------------------------------------------------------------------

_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")          # KSDATAFORMAT_SUBTYPE_*: the tag, then these 14 bytes
_INT_FORMATS = {1: "u8", 2: "s16", 3: "s24", 4: "s32"}
_FLOAT_FORMATS = {4: "f32", 8: "f64"}


def _parse_fmt(body, path):
    if len(body) < 16:
        raise ValueError(f"{path}: a fmt chunk of {len(body)} bytes")
    tag, channels, rate, _, block_align, bits = struct.unpack("<HHIIHH", body[:16])
    valid = bits
    if tag == 0xFFFE:
        if len(body) < 40:
            raise ValueError(f"{path}: an extensible fmt chunk of {len(body)} bytes")
        valid = struct.unpack("<H", body[18:20])[0] or bits
        tag = struct.unpack("<H", body[24:26])[0]
        if body[26:40] != _GUID_TAIL or tag not in (1, 3):
            raise ValueError(f"{path}: extensible sub-format {body[24:40].hex()} is neither PCM nor IEEE float (compressed?)")
    elif tag not in (1, 3):
        raise ValueError(f"{path}: format tag 0x{tag:04x} is neither PCM (1), IEEE float (3) nor extensible (0xfffe): compressed?")
    if channels > MAX_CHANNELS:
        raise ValueError(f"{path}: {channels} channels (more than {MAX_CHANNELS} channels are not supported)")
    if channels < 1:
        raise ValueError(f"{path}: {channels} channels")
    width = block_align // channels
    if block_align != channels * width or 8 * width < bits:
        raise ValueError(f"{path}: block_align {block_align} is not channels * width ({channels} channels of {bits} bits)")
    fmt = (_INT_FORMATS if tag == 1 else _FLOAT_FORMATS).get(width)
    if fmt is None:
        raise ValueError(f"{path}: {'integer' if tag == 1 else 'float'} samples of {width} bytes are not supported")
    if not 1 <= valid <= 8 * width:
        raise ValueError(f"{path}: {valid} valid bits in a container of {8 * width}")
    return fmt, channels, rate, valid, block_align


def wav_info(path):
    """WavInfo of a RIFF/WAVE file: a walk over its chunks (odd sizes padded; LIST, fact and the like skipped) to `fmt ` — tag 1
    PCM, 3 IEEE float, or 0xFFFE extensible with a PCM or float sub-format — and `data`.  The container width is block_align /
    channels: 8 / 16 / 24 / 32-bit integers, 32 / 64-bit floats; fewer valid bits are left-justified and the container decides
    the scale.  A data size of 0 or 0xFFFFFFFF, or one past the end of the file, is clamped to the whole frames present
    (truncated=True).  ValueError naming the cause for anything else."""
    path = os.fspath(path)
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(12)
        if head[:4] in (b"RF64", b"BW64"):
            raise ValueError(f"{path}: {head[:4].decode()} files are not supported")
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        fmt, pos = None, 12
        while True:
            f.seek(pos)
            hdr = f.read(8)
            if len(hdr) < 8:
                raise ValueError(f"{path}: no data chunk")
            cid, csize = hdr[:4], struct.unpack("<I", hdr[4:])[0]
            if cid == b"fmt ":
                fmt = _parse_fmt(f.read(min(csize, 40)), path)
            elif cid == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: no fmt chunk before the data chunk")
                name, channels, rate, valid, block_align = fmt
                present = size - (pos + 8)
                truncated = csize in (0, 0xFFFFFFFF) or csize > present
                return WavInfo(name, channels, rate, (present if truncated else csize) // block_align, pos + 8, valid, truncated)
            pos += 8 + csize + (csize & 1)


def load_wav(path, select=None, dtype=np.float32, rate=SAMPLING_RATE, to="cuda", slab_bytes=None):
    """Recording(samples, rate_in, info) of a WAV file: wav_info, an np.memmap of the data chunk, decode_pcm in slabs, then
    Resampler(info.rate, rate) when the rates differ.  samples: [S, T'] (S = len(select), or every channel), a CUDA tensor
    (to="cuda") or a numpy array (to=None).  The rows are planar and contiguous: the pairs of channels that
    DelayEstimatorBatch or a dual_channels chain take as [S / 2, 2, T'] are a view the caller takes,
    samples.reshape(S // 2, 2, -1)."""
    info = wav_info(path)
    name = _dtype_name(dtype)
    width = FORMATS[info.fmt][1]
    n_bytes = info.n_frames * info.channels * width
    raw = np.memmap(path, np.uint8, "r", offset=info.data_offset, shape=(n_bytes,)) if n_bytes else np.empty(0, np.uint8)
    samples = decode_pcm(raw, info.fmt, info.channels, select=select, dtype=name, to=to, slab_bytes=slab_bytes)
    if info.rate != int(rate):
        from .resample import Resampler
        samples = Resampler(info.rate, int(rate)).run(samples, dtype=name).y
    return Recording(samples, info.rate, info)
