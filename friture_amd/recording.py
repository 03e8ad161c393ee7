"""Recordings as they are stored: interleaved integer or float PCM, the data chunk of a WAV file, decoded on the GPU into the
planar float rows [S, T] that the batch classes and the Resampler read (pcm.hip, frt_pcm_*; the definition:
include/friture_hip.h, R2).

A PCM buffer is frames of `channels` interleaved little-endian samples; FORMATS names the sample formats.  Full scale is
[-1, 1): u8 (b - 128) 2^-7, s16 v 2^-15, s24 v 2^-23, s32 v 2^-31, f32 and f64 the value itself.  The float64 output is the
exact value, the float32 output one round-to-nearest-even of it.  The raw bytes go to the device once (host data in slabs
through page-locked memory); one kernel de-interleaves, selects channels, sign-extends and scales.  wav_info reads a WAV
header without the `wave` module (which refuses WAVE_FORMAT_EXTENSIBLE and float files on older interpreters); load_wav maps
the file, decodes it and brings it to SAMPLING_RATE.  There is no CPU fallback: decode_pcm goes to the HIP library.

The way out is the mirror (pcmenc.hip, frt_pcmenc_*; include/friture_hip.h, R3): encode_pcm routes rows to output channels,
rounds half to even, saturates (counting what it clipped), optionally dithers, and interleaves on the device; wav_header and
save_wav write the file that wav_info and load_wav read back; player_route and mode="player" are the routing and the int16
block arithmetic of the reference's playback (friture/playback/player.py:148-182)."""
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
            h.set_stream()
            call(y)
        return y
    import torch
    with _batchio.null_stream(data, is_np) as dev:
        y = torch.empty((S, count), dtype=getattr(torch, name), device=dev)
        with h.lock:
            h.set_stream()
            call(y)
    return y


class _Locked(_lib.Handle):
    """One frt_pcm or frt_pcmenc object: the page-locked slabs and the device staging of decode_pcm or encode_pcm, kept from call
    to call and shared by every caller of the process.  It serves one call at a time, so calls from several threads take `lock`
    in turn."""

    def __init__(self, kind):
        self.lock = threading.Lock()
        super().__init__(kind)


_shared = None
_shared_lock = threading.Lock()


def _handle():
    global _shared
    with _shared_lock:
        if _shared is None:
            _shared = _Locked("pcm")
        return _shared


# ---- the way out: planar float rows to interleaved PCM (pcmenc.hip, frt_pcmenc_*; the definition: friture_hip.h, R3) ------------

MAX_ROWS = 65535
MAX_FRAME_INDEX = 1 << 50
MODES = {"nearest": 0, "player": 1}


class EncodedPcm(NamedTuple):
    data: object          # 1-D uint8: frames of `channels` interleaved little-endian samples
    clipped: np.ndarray   # int64 [channels]: samples per output channel that were out of range or NaN


def player_route(n_rows, out_channels):
    """The route of the reference's playback block (friture/playback/player.py:161-171): one row goes to every output;
    otherwise row c goes to output c and the outputs beyond the rows are silent (-1)."""
    n_rows, out_channels = operator.index(n_rows), operator.index(out_channels)
    if n_rows < 1 or out_channels < 1:
        raise ValueError(f"{n_rows} rows to {out_channels} outputs")
    return [0] * out_channels if n_rows == 1 else [c if c < n_rows else -1 for c in range(out_channels)]


def _rows_of(x):
    """(x as [S, T], is_np) of the float rows a numpy array or CUDA tensor holds."""
    is_np = isinstance(x, np.ndarray)
    if not is_np and not (type(x).__module__.startswith("torch") and x.is_cuda):
        raise TypeError(f"samples: a numpy array or a CUDA tensor, got {type(x).__name__}")
    if x.ndim not in (1, 2):
        raise ValueError(f"expected [S, T] or [T], got {tuple(x.shape)}")
    if str(x.dtype).split(".")[-1] not in ("float32", "float64"):
        raise TypeError(f"samples must be float32 or float64, got {x.dtype}")
    return (x[None] if x.ndim == 1 else x), is_np


def _check_route(route, channels, n_rows):
    try:
        rt = np.arange(n_rows, dtype=np.int64) if route is None else np.array([operator.index(r) for r in route], np.int64)
    except TypeError as e:
        raise ValueError(f"route {route!r}: a sequence of integer row indices (-1: silence)") from e
    if not 1 <= rt.size <= MAX_CHANNELS:
        raise ValueError(f"channels {rt.size} (1 .. {MAX_CHANNELS})")
    if channels is not None:
        if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or int(channels) != rt.size:
            raise ValueError(f"channels {channels!r} for a route of {rt.size} entries")
    if rt.min() < -1 or rt.max() >= n_rows:
        raise ValueError(f"route {rt.tolist()} of {n_rows} rows (-1: silence)")
    return np.ascontiguousarray(rt, np.int32)


def _destination(out, n_bytes):
    """(out, on the host?) of a caller's destination: a writable 1-D uint8 numpy array (np.memmap) or CUDA tensor of n_bytes."""
    if type(out).__module__.startswith("torch"):
        import torch
        if not out.is_cuda or out.dtype != torch.uint8 or out.ndim != 1 or (out.numel() > 1 and out.stride(0) != 1):
            raise TypeError(f"out: a 1-D unit-stride CUDA uint8 tensor, got {out.dtype} {tuple(out.shape)} on {out.device}")
        host = False
    elif isinstance(out, np.ndarray):
        if out.dtype != np.uint8 or out.ndim != 1 or (out.size > 1 and out.strides[0] != 1) or not out.flags.writeable:
            raise TypeError(f"out: a writable 1-D unit-stride uint8 array, got {out.dtype} {out.shape}")
        host = True
    else:
        raise TypeError(f"out: a numpy uint8 array, np.memmap or CUDA uint8 tensor, got {type(out).__name__}")
    if int(out.shape[0]) != n_bytes:
        raise ValueError(f"out holds {int(out.shape[0])} bytes, the encoding has {n_bytes}")
    return out, host


def encode_pcm(x, fmt, route=None, channels=None, frame0=0, dither=False, seed=0, mode="nearest", to=None, out=None, slab_bytes=None):
    """EncodedPcm(data, clipped): the rows x [S, T] (or [T]; float32 / float64, a numpy array or a CUDA tensor, read in place
    whatever the row stride) as T frames of interleaved little-endian samples of format `fmt`, the inverse of decode_pcm.
    route[c]: the row that output channel c carries, -1 for silence, repeats and any order allowed (None: every row in order);
    channels, when given, is len(route).  Integer formats round half to even and saturate; clipped[c] counts the samples of
    channel c that were out of range or NaN.  dither=True adds triangular dither of +-1 LSB before the rounding, a pure function
    of (seed, frame0 + frame, channel): a recording cut into pieces encodes to the same bytes when each piece is given its
    frame0.  mode="player" (s16, no dither) is the reference's output block, trunc(32767 * clip(v, -1, 1)).
    data is 1-D uint8: a numpy array for numpy rows, a CUDA tensor for a tensor (to="host": a numpy array, the bytes coming down
    in slabs — the float rows never exist on the host; to="cuda": a CUDA tensor from numpy rows), or `out`, a writable 1-D uint8
    numpy array, np.memmap or CUDA tensor of exactly T * channels * width bytes at any byte offset.  Host buffers move in slabs
    of at most slab_bytes (None: 64 MB); the result does not depend on it.  Calls from several threads share one set of staging
    buffers and run one after the other."""
    if not isinstance(fmt, str) or fmt not in FORMATS:
        raise ValueError(f"format {fmt!r} (one of {', '.join(FORMATS)})")
    code, width = FORMATS[fmt]
    x, is_np = _rows_of(x)
    S, T = int(x.shape[0]), int(x.shape[1])
    if not 1 <= S <= MAX_ROWS:
        raise ValueError(f"{S} rows (1 .. {MAX_ROWS})")
    rt = _check_route(route, channels, S)
    C = int(rt.size)
    frame0 = operator.index(frame0)
    if frame0 < 0 or frame0 + T > MAX_FRAME_INDEX:
        raise ValueError(f"frame0 {frame0} with {T} frames (0 .. 2^50)")
    if mode not in MODES:
        raise ValueError(f"mode {mode!r} (one of {', '.join(MODES)})")
    if not isinstance(dither, (bool, np.bool_)):
        raise TypeError(f"dither {dither!r} (True or False)")
    dither = bool(dither)
    if dither and code >= 4:
        raise ValueError(f"dither with the float format {fmt}")
    if mode == "player" and (fmt != "s16" or dither):
        raise ValueError(f"mode 'player' is for s16 without dither, got {fmt}{' with dither' if dither else ''}")
    seed = operator.index(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed {seed} (0 .. 2^64 - 1)")
    if to not in (None, "host", "cuda"):
        raise ValueError(f"to={to!r} (None, 'host' or 'cuda')")
    slab = 0 if slab_bytes is None else int(slab_bytes)
    if slab < 0:
        raise ValueError(f"slab_bytes {slab_bytes!r}")
    n_bytes = T * C * width
    if out is not None:
        if to is not None:
            raise ValueError("give `out` or `to`, not both")
        out, host_out = _destination(out, n_bytes)
        if not is_np and not host_out and out.device != x.device:
            raise ValueError(f"out is on {out.device}, the rows are on {x.device}")
    else:
        host_out = is_np if to is None else to == "host"
    clipped = np.zeros(C, np.int64)
    if is_np and host_out and out is None:
        out = np.empty(n_bytes, np.uint8)
    h, vp = _encoder(), ctypes.c_void_p

    def call(data):
        src, addr, x_dtype, strides = _batchio.source(x, strided=True)
        if S > 1 and strides[0] < T:                            # rows that overlap (an expanded tensor): read a copy
            src, addr, x_dtype, strides = _batchio.source(x, strided=False)
        with h.lock:
            h.set_stream()
            _lib.check(h.lib.frt_pcmenc_encode(h.h, vp(addr) if T else None, x_dtype, S, int(strides[0]) if S > 1 else max(T, 1), T,
                                               frame0, vp(rt.ctypes.data), C, code, MODES[mode], int(dither), seed,
                                               vp(_batchio.ptr(data)) if T else None, vp(clipped.ctypes.data), slab))
        del src                                                 # a copy lives until the call has synchronised

    if is_np and host_out:
        call(out)
        return EncodedPcm(out, clipped)
    import torch
    anchor = x if not is_np else out                            # the tensor whose device and stream the call joins, if there is one
    with _batchio.null_stream(anchor, anchor is None) as dev:
        if out is None:
            out = np.empty(n_bytes, np.uint8) if host_out else torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        call(out)
    return EncodedPcm(out, clipped)


_shared_encoder = None


def _encoder():
    global _shared_encoder
    with _shared_lock:
        if _shared_encoder is None:
            _shared_encoder = _Locked("pcmenc")
        return _shared_encoder


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


def _chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def wav_header(fmt, channels, rate, n_frames):
    """The bytes of a RIFF/WAVE file in front of its samples, for n_frames frames of `channels` samples of format `fmt`: a
    plain `fmt ` chunk (tag 1) for u8 / s16 with at most 2 channels, otherwise WAVE_FORMAT_EXTENSIBLE with the PCM or IEEE-float
    sub-format, valid bits equal to the container's and channel mask 0; a `fact` chunk for the float formats; then the `data`
    chunk's header.  The file is these bytes, the n_frames * channels * width sample bytes and, when that count is odd, one
    pad byte.  ValueError when the RIFF size would pass 2^32 - 1 (RF64 is out of scope, as on the way in)."""
    code, width, channels = _check_format(fmt, channels)
    rate, n_frames = operator.index(rate), operator.index(n_frames)
    if not 1 <= rate < 1 << 32:
        raise ValueError(f"rate {rate}")
    if n_frames < 0:
        raise ValueError(f"{n_frames} frames")
    block, bits, tag = channels * width, 8 * width, 3 if code >= 4 else 1
    if block * rate >= 1 << 32:
        raise ValueError(f"{block * rate} bytes per second do not fit the fmt chunk")
    body = struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits)
    if not (fmt in ("u8", "s16") and channels <= 2):
        body = struct.pack("<H", 0xFFFE) + body[2:] + struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + _GUID_TAIL
    chunks = _chunk(b"fmt ", body)
    data = n_frames * block
    if tag == 3:
        if n_frames >= 1 << 32:
            raise ValueError(f"{n_frames} frames do not fit a RIFF file (RF64 is not supported)")
        chunks += _chunk(b"fact", struct.pack("<I", n_frames))
    riff = 4 + len(chunks) + 8 + data + (data & 1)
    if riff > 0xFFFFFFFF:
        raise ValueError(f"{data} bytes of samples do not fit a RIFF file (RF64 is not supported)")
    return b"RIFF" + struct.pack("<I", riff) + b"WAVE" + chunks + b"data" + struct.pack("<I", data)


def save_wav(path, samples, rate=SAMPLING_RATE, fmt="s16", route=None, dither=None, seed=0, slab_bytes=None):
    """Writes the rows `samples` [S, T] (or [T]; a numpy array or a CUDA tensor) as a WAV file of format `fmt` and returns its
    wav_info: wav_header, the file sized, its data region mapped with np.memmap and filled by encode_pcm (a CUDA tensor comes
    down as encoded bytes in slabs; the float rows never exist on the host).  route: as for encode_pcm, one output channel per
    entry.  dither: None means ON for u8 and s16 and OFF for every other format — say dither=False for the plain rounding of
    a 16-bit file; seed: the dither's.  When the encode fails the file is removed: no header over zeros stays behind."""
    path = os.fspath(path)
    x, _ = _rows_of(samples)
    if not isinstance(fmt, str) or fmt not in FORMATS:
        raise ValueError(f"format {fmt!r} (one of {', '.join(FORMATS)})")
    rt = _check_route(route, None, int(x.shape[0]))
    if dither is None:
        dither = fmt in ("u8", "s16")
    T, width = int(x.shape[1]), FORMATS[fmt][1]
    head = wav_header(fmt, int(rt.size), rate, T)
    n_bytes = T * int(rt.size) * width
    with open(path, "wb") as f:
        f.write(head)
        f.truncate(len(head) + n_bytes + (n_bytes & 1))
    if n_bytes:
        data = np.memmap(path, np.uint8, "r+", offset=len(head), shape=(n_bytes,))
        try:
            encode_pcm(x, fmt, route=rt.tolist(), dither=dither, seed=seed, out=data, slab_bytes=slab_bytes)
            data.flush()
        except BaseException:                   # no file of zeros with a valid header is left behind
            del data
            os.remove(path)
            raise
        del data
    return wav_info(path)
