"""The definition of the PCM ingest (include/friture_hip.h, R2) restated in numpy, what the GPU tests of recording.py compare
with bit for bit; `pack`, which writes test buffers; and a hand-built RIFF writer for the headers the stdlib `wave` writer
cannot produce.

decode: for an integer format (raw_as_int.astype(float64) * 2^-(bits - 1)).astype(dtype) — the float64 product is exact, the
cast is the one rounding; the 24-bit unpack is ((b0 | b1 << 8 | b2 << 16) ^ 0x800000) - 0x800000; f32 / f64 are one astype."""
import struct

import numpy as np

FORMATS = {"u8": (0, 1), "s16": (1, 2), "s24": (2, 3), "s32": (3, 4), "f32": (4, 4), "f64": (5, 8)}
INT_BITS = {"u8": 8, "s16": 16, "s24": 24, "s32": 32}
GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def raw_values(raw, fmt, channels):
    """[T, C] of the samples as stored: int64 for the integer formats (u8 with its offset removed), float32 / float64."""
    raw = np.ascontiguousarray(np.asarray(raw, np.uint8))
    w = FORMATS[fmt][1]
    b = raw.reshape(-1, channels, w)
    if fmt == "u8":
        return b[..., 0].astype(np.int64) - 128
    if fmt == "s24":
        v = b[..., 0].astype(np.int64) | (b[..., 1].astype(np.int64) << 8) | (b[..., 2].astype(np.int64) << 16)
        return (v ^ 0x800000) - 0x800000
    kind = {"s16": "<i2", "s32": "<i4", "f32": "<f4", "f64": "<f8"}[fmt]
    v = b.reshape(-1, channels * w).copy().view(kind)
    return v.astype(np.int64) if fmt in INT_BITS else v


def decode(raw, fmt, channels, select=None, start=0, count=None, dtype=np.float32):
    """[len(select), count] as decode_pcm defines it."""
    v = raw_values(raw, fmt, channels)
    count = v.shape[0] - start if count is None else count
    v = v[start:start + count][:, list(range(channels)) if select is None else list(select)].T
    if fmt in INT_BITS:
        return np.ascontiguousarray((v.astype(np.float64) * 2.0 ** -(INT_BITS[fmt] - 1)).astype(dtype))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(v.astype(dtype))


def pack(values, fmt):
    """uint8 bytes of `values` [T, C] (or [T]): integers as stored for the integer formats (u8: -128 .. 127, the offset is added
    here), floats for f32 / f64."""
    v = np.asarray(values)
    if fmt == "u8":
        return (v.astype(np.int64) + 128).astype(np.uint8).reshape(-1)
    if fmt == "s24":
        u = v.astype(np.int64) & 0xFFFFFF
        return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8).reshape(-1)
    kind = {"s16": "<i2", "s32": "<i4", "f32": "<f4", "f64": "<f8"}[fmt]
    return np.ascontiguousarray(v.astype(kind)).view(np.uint8).reshape(-1)


def int_range(fmt):
    bits = INT_BITS[fmt]
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


def edge_values(fmt, single):
    """The values the issue names, as `pack` takes them; single: the output is float32."""
    if fmt in INT_BITS:
        lo, hi = int_range(fmt)
        edges = [lo, hi, -1, 0, 1]
        if fmt == "s24":
            edges += [0x7FFFFF, -0x800000]
        if fmt == "s32":
            edges += [(1 << 24) + 1, (1 << 24) + 3, (1 << 31) - 65]          # two ties of the float32 grid, one just under full scale
        return np.array(edges, np.int64)
    edges = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -0.5]
    if fmt == "f64":
        edges += [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24,                   # ties of the float32 grid: to even, down and up
                  float(np.finfo(np.float32).max), 2.0 ** -140, 3 * 2.0 ** -150, 2.0 ** -150, 1e-320]
    else:
        edges += [float(np.finfo(np.float32).max), 2.0 ** -140, float(np.finfo(np.float32).tiny)]
    return np.array(edges, np.float64 if fmt == "f64" else np.float32)


def random_raw(fmt, channels, frames, seed, single=False):
    """Seeded random bytes of `frames` frames (for f32 / f64 random finite values of many magnitudes: random bytes would be
    mostly huge or NaN), uint8."""
    rng = np.random.default_rng(seed)
    n = frames * channels
    if fmt == "f32":
        return pack((rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32).reshape(frames, channels), fmt)
    if fmt == "f64":
        return pack((rng.standard_normal(n) * 10.0 ** rng.integers(-12, 6, n)).reshape(frames, channels), fmt)
    return rng.integers(0, 256, n * FORMATS[fmt][1], dtype=np.uint8)


def place(raw, fmt, channels, frame, values):
    """Writes `values` into consecutive samples of `raw` (uint8, in place) from channel 0 of `frame` on, as far as they fit."""
    w = FORMATS[fmt][1]
    b = pack(values, fmt)
    a = frame * channels * w
    n = min(len(b), len(raw) - a) // w * w
    if a >= 0 and n > 0:
        raw[a:a + n] = b[:n]


# ---- RIFF by hand ------------------------------------------------------------------------------------------------------------------

def chunk(cid, body, size=None):
    """A chunk with its pad byte; size: the size field to write instead of the true one."""
    return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")


def fmt_chunk(tag, channels, rate, width, bits=None, extensible=False, valid_bits=None, block_align=None, sub_tail=GUID_TAIL):
    bits = 8 * width if bits is None else bits
    block_align = channels * width if block_align is None else block_align
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * block_align, block_align, bits)
    if extensible:
        body += struct.pack("<HHI", 22, bits if valid_bits is None else valid_bits, 0) + struct.pack("<H", tag) + sub_tail
    return chunk(b"fmt ", body)


def riff(chunks, form=b"RIFF", kind=b"WAVE"):
    body = kind + b"".join(chunks)
    return form + struct.pack("<I", len(body) & 0xFFFFFFFF) + body


def write_wav(path, raw, fmt, channels, rate, extensible=False, before=(), data_size=None, valid_bits=None):
    """A WAV file of the bytes `raw`; before: chunks between fmt and data; data_size: the size field of the data chunk."""
    tag = 3 if fmt in ("f32", "f64") else 1
    width = FORMATS[fmt][1]
    bits = valid_bits if valid_bits is not None and not extensible else None
    head = fmt_chunk(tag, channels, rate, width, bits=bits, extensible=extensible, valid_bits=valid_bits)
    data = b"data" + struct.pack("<I", len(raw) if data_size is None else data_size) + bytes(raw)
    path.write_bytes(riff([head, *before, data]))
    return path
