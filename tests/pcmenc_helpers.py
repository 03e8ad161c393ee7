"""The definition of the PCM export (include/friture_hip.h, R3) restated in numpy: what the GPU tests of encode_pcm compare with
bit for bit.  The yardstick, never the code under test.

encode: for an integer format of b bits, t = float64(x) * 2^(b-1) (exact), t += d with dither, r = rint(t) (half to even),
q = clip(r, -2^(b-1), 2^(b-1) - 1), NaN -> 0, then recording_helpers.pack; clipped[c] counts r outside the range or NaN.  f32 /
f64 are one astype.  A route entry of -1 is silence: q = 0 (+0.0), not dithered, not counted.  mode "player" is player_block's
arithmetic.  philox4x32_10 is the generator as published (Salmon et al., SC'11), vectorised; dither builds d from it."""
import struct
import wave

import numpy as np

import recording_helpers as H

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (uint32 values, broadcast against each other) -> [..., 4] uint32."""
    c = np.asarray(counter, np.uint64)
    k = np.asarray(key, np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                      # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & np.uint64(MASK)
        k0, k1 = (k0 + np.uint64(W0)) & np.uint64(MASK), (k1 + np.uint64(W1)) & np.uint64(MASK)
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def dither(frames, channels, seed):
    """d [len(frames), channels] float64: counter (f lo, f hi, c, 0), key (seed lo, seed hi), d = ((o0 >> 8) - (o1 >> 8)) 2^-24."""
    f = np.asarray(frames, np.uint64).reshape(-1, 1)
    c = np.arange(channels, dtype=np.uint64).reshape(1, -1)
    f, c = np.broadcast_arrays(f, c)
    counter = np.stack([f & np.uint64(MASK), f >> np.uint64(32), c, np.zeros_like(f)], axis=-1)
    o = philox4x32_10(counter, np.array([seed & MASK, (seed >> 32) & MASK], np.uint64))
    return ((o[..., 0] >> 8).astype(np.int64) - (o[..., 1] >> 8).astype(np.int64)).astype(np.float64) * 2.0 ** -24


def quantise(v, fmt, d=None):
    """(q int64, clip bool) of float64 values v, elementwise, as R3 defines mode 0."""
    full = 2.0 ** (H.INT_BITS[fmt] - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(v, np.float64) * full
        if d is not None:
            t = t + d
        r = np.rint(t)
        nan = np.isnan(r)
        clip = nan | (r < -full) | (r > full - 1)
        q = np.where(nan, 0.0, np.clip(r, -full, full - 1)).astype(np.int64)
    return q, clip


def encode(x, fmt, route=None, frame0=0, dither_on=False, seed=0, mode="nearest"):
    """(bytes uint8 [T * C * width], clipped int64 [C]) of the rows x [S, T] as encode_pcm defines them."""
    x = np.asarray(x)
    x = x[None] if x.ndim == 1 else x
    S, T = x.shape
    route = list(range(S)) if route is None else list(route)
    C = len(route)
    live = np.array([r >= 0 for r in route])
    rows = np.stack([x[r] if r >= 0 else np.zeros(T, x.dtype) for r in route], axis=1) if T else np.zeros((0, C), x.dtype)      # [T, C]
    clipped = np.zeros(C, np.int64)
    if fmt in ("f32", "f64"):
        with np.errstate(over="ignore", invalid="ignore"):
            return H.pack(rows.astype(np.float32 if fmt == "f32" else np.float64), fmt), clipped
    v = rows.astype(np.float64)
    if mode == "player":
        assert fmt == "s16" and not dither_on
        q, clip = player_values(v)
    else:
        d = None
        if dither_on:
            d = dither(np.arange(T, dtype=np.uint64) + np.uint64(frame0), C, seed) * live[None, :]
        q, clip = quantise(v, fmt, d)
    clipped += (clip & live[None, :]).sum(axis=0)
    return H.pack(q, fmt), clipped


def player_values(v):
    """(q, clip) of the three statements of friture/playback/player.py:174-177 on float64 values; a NaN gives 0."""
    with np.errstate(invalid="ignore"):
        info = np.iinfo(np.int16)
        scale = min(abs(info.min), info.max)
        res = scale * np.clip(v, -1.0, 1.0)
        nan = np.isnan(res)
        q = np.where(nan, 0.0, np.trunc(res)).astype(np.int16).astype(np.int64)          # astype(int16) truncates toward zero
        return q, nan | (np.abs(v) > 1.0)


def player_block(rows, out_channels):
    """One block of friture/playback/player.py:148-182 with the whole block available: rows [in_channels, samples] (the
    float history), the result int16 [samples, out_channels] as the output stream takes it.  NaN, which the reference never
    meets, is 0 (R3)."""
    rows = np.asarray(rows)
    in_channels, samples = rows.shape
    res = np.zeros((out_channels, samples))
    if in_channels == 1:
        for i in range(out_channels):
            res[i, :] = rows[0, :]
    else:
        copy_channels = min(out_channels, in_channels)
        res[0:copy_channels, :] = rows[0:copy_channels, :]
    q, _ = player_values(res)
    return q.astype(np.int16).transpose()


def check_wav_header(head, fmt, channels, rate, n_frames):
    """The fields of a header wav_header wrote, read with struct alone: the RIFF size is what follows it in a file of the header,
    the data and its pad byte; the layout is the one R3 names."""
    width = H.FORMATS[fmt][1]
    data = n_frames * channels * width
    assert head[:4] == b"RIFF" and head[8:12] == b"WAVE" and head[12:16] == b"fmt "
    assert struct.unpack("<I", head[4:8])[0] == len(head) - 8 + data + (data & 1)
    plain = fmt in ("u8", "s16") and channels <= 2
    size = struct.unpack("<I", head[16:20])[0]
    assert size == (16 if plain else 40)
    tag, ch, r, byte_rate, block, bits = struct.unpack("<HHIIHH", head[20:36])
    sub = 3 if fmt in ("f32", "f64") else 1
    assert (tag, ch, r, byte_rate, block, bits) == (sub if plain else 0xFFFE, channels, rate, rate * channels * width, channels * width, 8 * width)
    pos = 20 + size
    if not plain:
        cb, valid, mask, subtag = struct.unpack("<HHIH", head[36:46])
        assert (cb, valid, mask, subtag) == (22, 8 * width, 0, sub) and head[46:60] == H.GUID_TAIL
    if sub == 3:
        assert head[pos:pos + 8] == b"fact" + struct.pack("<I", 4) and struct.unpack("<I", head[pos + 8:pos + 12])[0] == n_frames
        pos += 12
    assert head[pos:pos + 4] == b"data" and struct.unpack("<I", head[pos + 4:pos + 8])[0] == data and pos + 8 == len(head)


def read_with_wave_module(path):
    with wave.open(str(path), "rb") as w:
        return w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes(), w.readframes(w.getnframes())
