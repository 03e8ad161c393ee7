"""PCM export on the GPU (pcmenc.hip, recording.encode_pcm / save_wav) against the numpy restatement of tests/pcmenc_helpers.py,
which test_pcmenc_cpu.py checks against known answers and hand-written values.  The output is defined to the bit, so every
comparison is of bytes (for the float formats of values, NaN equal to NaN: a NaN's payload is not specified) and no tolerance
appears.  Shapes are a few tiles at most: F = tile_frames(fmt, C) frames is what one workgroup encodes."""
import functools

import numpy as np
import pytest

import pcmenc_helpers as E
import recording_helpers as H
from friture_amd.recording import FORMATS, decode_pcm, encode_pcm, load_wav, player_route, save_wav, tile_frames, wav_info

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
INT_FORMATS = ("u8", "s16", "s24", "s32")
ROUND_TRIPS = [(fmt, dtype) for fmt in INT_FORMATS for dtype in DTYPES if (fmt, dtype) != ("s32", np.float32)]


def planted(fmt):
    """The values the definition turns on, float64: exact ties for even and odd k, the clamp edges, infinities, NaN, -0.0 for
    the integer formats; the tie and subnormal lists of the ingest's tests for the float formats."""
    if fmt not in H.INT_BITS:
        return np.concatenate([H.edge_values("f64", False), H.edge_values("f32", True).astype(np.float64)])
    lsb = 2.0 ** -(H.INT_BITS[fmt] - 1)
    ties = [(k + 0.5) * lsb for k in (0, 1, 2, 3, -1, -2, -3, -4, 100, 101, -100, -101, 126, 127, -128, -129)]
    return np.array(ties + [1.0, -1.0, 1 - lsb, -1 - lsb, 1 - 0.5 * lsb, -1 - 0.5 * lsb, np.inf, -np.inf, np.nan, -0.0, 0.0, 1e300, -1e300, 5e-324])


@functools.lru_cache(maxsize=None)
def rows(fmt, S, T, dtype, seed=0):
    """Seeded noise of about 0.3 full scale [S, T] with the planted values at the start, across the seams of the first tile for
    1, 2, 3 and 6 channels, and at the end, each row starting the list elsewhere (read-only, shared)."""
    rng = np.random.default_rng(1000 * seed + 31 * S + T)
    x = 0.3 * rng.standard_normal((S, T))
    p = planted(fmt)
    seams = {0, T - len(p)} | {tile_frames(fmt, c) - len(p) // 2 for c in (1, 2, 3, 6)}
    for s in range(S):
        for at in seams:
            q = np.roll(p, 5 * s)[:max(0, min(len(p), T - at))]
            if at >= 0 and len(q):
                x[s, at:at + len(q)] = q
    with np.errstate(over="ignore"):
        x = x.astype(dtype)
    x.setflags(write=False)
    return x


def cuda(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same(got, ref, fmt):
    """the bytes; for f32 / f64 the values they hold, NaN equal to NaN, zeros with their signs"""
    got = host(got)
    if got.dtype != np.uint8 or got.shape != ref.shape:
        return False
    if fmt in H.INT_BITS:
        return np.array_equal(got, ref)
    kind = "<f4" if fmt == "f32" else "<f8"
    a, b = got.view(kind), ref.view(kind)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)]))


def check(x, fmt, route=None, **kw):
    """encode_pcm of the CUDA copy of x against the helper: bytes and clip counts"""
    ref, clipped = E.encode(x, fmt, route=route, frame0=kw.get("frame0", 0), dither_on=kw.get("dither", False), seed=kw.get("seed", 0),
                            mode=kw.get("mode", "nearest"))
    got = encode_pcm(cuda(x), fmt, route=route, **kw)
    assert got.data.is_cuda and got.data.ndim == 1 and got.clipped.dtype == np.int64
    assert same(got.data, ref, fmt), (fmt, x.shape, x.dtype, route, kw)
    assert got.clipped.tolist() == clipped.tolist(), (fmt, x.shape, x.dtype, route, kw)
    return ref, clipped


# ---- formats and dtypes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_every_format_dtype_and_length_is_bit_exact(hip, fmt, dtype):
    some_clip = False
    for C in (1, 2, 3, 6):
        F = tile_frames(fmt, C)
        for T in (1, 63, 64, 65, F - 1, F, F + 1, 2 * F + 3):
            _, clipped = check(rows(fmt, C, T, dtype), fmt)
            some_clip |= bool(clipped.any())
    assert some_clip == (fmt in H.INT_BITS)
    got = encode_pcm(cuda(rows(fmt, 2, 0, dtype)), fmt)
    assert got.data.numel() == 0 and got.clipped.tolist() == [0, 0]
    one = encode_pcm(cuda(rows(fmt, 1, 65, dtype)[0]), fmt)                          # [T] is one row
    assert same(one.data, E.encode(rows(fmt, 1, 65, dtype), fmt)[0], fmt)


# ---- destination alignment ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ("device", "host"))
@pytest.mark.parametrize("fmt,C", (("s24", 3), ("s16", 1), ("f64", 2)))
def test_destination_at_any_byte_offset_and_nothing_outside_it(hip, fmt, C, where):
    import torch
    F = tile_frames(fmt, C)
    x = rows(fmt, C, F + 5, np.float32)
    ref, clipped = E.encode(x, fmt)
    dev = cuda(x)
    for offset in (0, 1, 3, 8, 15):
        total = offset + len(ref) + 21
        block = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda") if where == "device" else np.full(total, 0xA5, np.uint8)
        got = encode_pcm(dev, fmt, out=block[offset:offset + len(ref)])
        assert got.data.data_ptr() == block.data_ptr() + offset if where == "device" else got.data.ctypes.data == block.ctypes.data + offset
        after = host(block)
        assert same(after[offset:offset + len(ref)], ref, fmt) and got.clipped.tolist() == clipped.tolist(), (fmt, offset)
        assert (after[:offset] == 0xA5).all() and (after[offset + len(ref):] == 0xA5).all(), (fmt, offset)
    # a short range inside one granule, and one that ends inside its first
    for T, offset in ((1, 5), (2, 14)):
        block = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
        n = T * C * FORMATS[fmt][1]
        encode_pcm(dev[:, :T], fmt, out=block[offset:offset + n])
        after = host(block)
        assert same(after[offset:offset + n], E.encode(x[:, :T], fmt)[0], fmt)
        assert (after[:offset] == 0xA5).all() and (after[offset + n:] == 0xA5).all()


# ---- routing ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ("u8", "s16", "s24", "f32"))
def test_routes(hip, fmt):
    F = tile_frames(fmt, 6)
    x = rows(fmt, 4, F + 9, np.float64)
    for route in ([-1, 0, -1], [2, 2, 0, 2], [3, 2, 1, 0], [1], [-1], [0, -1, 3, 3, -1, 1]):
        ref, clipped = check(x, fmt, route=route)
        silent = [c for c, r in enumerate(route) if r < 0]
        w = FORMATS[fmt][1]
        frames = ref.reshape(-1, len(route), w)
        assert (frames[:, silent] == (128 if fmt == "u8" else 0)).all() and not clipped[silent].any()
        assert host(encode_pcm(cuda(x), fmt, route=route, channels=len(route)).data).tobytes() == host(encode_pcm(cuda(x), fmt, route=route).data).tobytes()
    check(x[:1], fmt, route=[0] * 6)                                                  # one row to six outputs
    check(x[:1], fmt, route=player_route(1, 6))


def test_rows_are_read_in_place_whatever_their_stride(hip):
    import torch
    wide = cuda(rows("s16", 6, 700, np.float32))
    view, ref = wide[:, 5:5 + 600], E.encode(rows("s16", 6, 700, np.float32)[:, 5:605], "s16")
    assert view.stride(0) == 700 and same(encode_pcm(view, "s16").data, ref[0], "s16")
    every_other = wide[::2]
    assert every_other.stride(0) == 1400 and same(encode_pcm(every_other, "s16").data, E.encode(rows("s16", 6, 700, np.float32)[::2], "s16")[0], "s16")
    assert same(encode_pcm(wide[:, ::2], "s16").data, E.encode(rows("s16", 6, 700, np.float32)[:, ::2], "s16")[0], "s16")      # a copy
    x = rows("s24", 6, 700, np.float64)
    assert same(encode_pcm(x[:, 5:605], "s24").data, E.encode(x[:, 5:605], "s24")[0], "s24")                  # numpy rows, strided
    assert same(encode_pcm(x[::2], "s24").data, E.encode(x[::2], "s24")[0], "s24")
    expanded = wide[0, :600].expand(3, 600)                                                                    # row stride 0
    assert same(encode_pcm(expanded, "s16").data, E.encode(host(wide[0, :600])[None].repeat(3, 0), "s16")[0], "s16")
    assert np.array_equal(host(wide).view(np.uint32), rows("s16", 6, 700, np.float32).view(np.uint32))         # never written


@pytest.mark.parametrize("fmt", ("s32", "f64"))
def test_sixty_four_channels(hip, fmt):
    F = tile_frames(fmt, 64)
    x = rows(fmt, 64, F + 1, np.float64)
    route = list(range(63, -1, -1))
    for T in (F - 1, F, F + 1):
        check(x[:, :T], fmt, route=route)
    check(x[:5], fmt, route=[c % 5 if c % 7 else -1 for c in range(64)])
    ref = E.encode(x, fmt)[0]
    import torch
    block = torch.full((3 + len(ref) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    encode_pcm(cuda(x), fmt, out=block[3:3 + len(ref)])
    assert same(block[3:3 + len(ref)], ref, fmt) and (host(block)[:3] == 0xA5).all() and (host(block)[3 + len(ref):] == 0xA5).all()


@pytest.mark.parametrize("fmt", ("s24", "s32"))
def test_clip_counts_over_more_workgroups_than_counter_rows(hip, fmt):
    """forty tiles and a partial one: every workgroup's counts reach the sum, whichever row of the device's table it adds to"""
    F = tile_frames(fmt, 64)
    T = 40 * F + 5
    x = np.array(rows(fmt, 3, T, np.float32))
    x[:, ::7] *= 4.0                                                     # about 0.4 of every seventh sample clips, in every tile
    route = [c % 3 if c % 5 else -1 for c in range(64)]
    _, clipped = check(x, fmt, route=route)
    assert (clipped[[c for c in range(64) if c % 5]] > T // 30).all()
    got = encode_pcm(x, fmt, route=route, slab_bytes=3 * F * 64 * FORMATS[fmt][1])          # host rows in slabs: the counts add up over them
    assert got.clipped.tolist() == clipped.tolist()


# ---- buffers in any mix --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,C,dtype", (("s24", 3, np.float32), ("s16", 2, np.float64), ("f32", 6, np.float64), ("u8", 1, np.float32)))
def test_host_and_device_buffers_in_any_mix_and_any_slab(hip, fmt, C, dtype):
    import torch
    F = tile_frames(fmt, C)
    tile = F * C * FORMATS[fmt][1]
    x = np.array(rows(fmt, 4, 4 * F + 5, dtype))
    route = [3, -1, 0, 0, 2, 1][:C]
    ref, clipped = E.encode(x, fmt, route=route)
    dev = cuda(x)
    for slab in (tile, 3 * tile, None):
        got = [encode_pcm(x, fmt, route=route, slab_bytes=slab),                                  # host to host
               encode_pcm(x, fmt, route=route, slab_bytes=slab, to="cuda"),                       # host to device
               encode_pcm(dev, fmt, route=route, slab_bytes=slab, to="host"),                     # device to host
               encode_pcm(dev, fmt, route=route, slab_bytes=slab)]                                # device to device
        assert [type(g.data) for g in got] == [np.ndarray, torch.Tensor, np.ndarray, torch.Tensor] and got[1].data.is_cuda and got[3].data.is_cuda
        for g in got:
            assert same(g.data, ref, fmt) and g.clipped.tolist() == clipped.tolist(), (fmt, slab)
    out = np.full(len(ref) + 2, 0xA5, np.uint8)
    encode_pcm(x, fmt, route=route, out=out[1:-1], slab_bytes=1)                                   # a tile per slab at the least
    assert same(out[1:-1], ref, fmt) and out[0] == out[-1] == 0xA5
    dst = torch.zeros(len(ref), dtype=torch.uint8, device="cuda")
    assert encode_pcm(x, fmt, route=route, out=dst, slab_bytes=tile).data is dst and same(dst, ref, fmt)
    assert same(encode_pcm(x[:1], fmt, route=[-1, -1]).data, E.encode(x[:1], fmt, route=[-1, -1])[0], fmt)      # nothing to send up


def test_out_on_another_device_than_the_rows_is_refused(hip):
    import torch
    x = cuda(rows("s16", 2, 100, np.float32))
    same_device = torch.empty(400, dtype=torch.uint8, device=x.device)
    assert encode_pcm(x, "s16", out=same_device).data is same_device
    if torch.cuda.device_count() > 1:
        other = torch.empty(400, dtype=torch.uint8, device=f"cuda:{(x.device.index + 1) % torch.cuda.device_count()}")
        with pytest.raises(ValueError, match="out is on"):
            encode_pcm(x, "s16", out=other)


# ---- dither -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("fmt", ("u8", "s16", "s24"))
def test_dither_matches_the_helper_and_does_not_depend_on_the_cut(hip, fmt, dtype):
    C = 3
    F = tile_frames(fmt, C)
    T = 2 * F + 3
    x = rows(fmt, 2, T, dtype)
    route, seed, frame0 = [1, -1, 0], 0xFEDCBA9876543210, (1 << 32) - F - 7                  # the frame index crosses 2^32 inside the call
    ref, clipped = check(x, fmt, route=route, dither=True, seed=seed, frame0=frame0)
    plain = E.encode(x, fmt, route=route)[0]
    assert not np.array_equal(ref, plain)
    w = FORMATS[fmt][1]
    assert (ref.reshape(-1, C, w)[:, 1] == (128 if fmt == "u8" else 0)).all()               # silence is not dithered
    dev = cuda(x)
    cuts = (0, 77, F + 64 + 5, T)                                                            # inside the first and the second tile
    parts, counts = [], np.zeros(C, np.int64)
    for a, b in zip(cuts, cuts[1:]):
        got = encode_pcm(dev[:, a:b], fmt, route=route, dither=True, seed=seed, frame0=frame0 + a)
        parts.append(host(got.data))
        counts += got.clipped
    assert np.array_equal(np.concatenate(parts), ref) and counts.tolist() == clipped.tolist()
    other = encode_pcm(dev, fmt, route=route, dither=True, seed=seed + 1, frame0=frame0)
    assert not np.array_equal(host(other.data), ref)
    assert same(other.data, E.encode(x, fmt, route=route, dither_on=True, seed=seed + 1, frame0=frame0)[0], fmt)
    assert same(encode_pcm(np.array(x), fmt, route=route, dither=True, seed=seed, frame0=frame0, slab_bytes=1).data, ref, fmt)      # a tile per slab
    assert same(encode_pcm(dev, fmt, route=route, dither=True, seed=seed, frame0=frame0, to="host", slab_bytes=1).data, ref, fmt)


def test_dither_on_s32_and_a_seed_of_zero(hip):
    check(rows("s32", 2, 300, np.float64), "s32", dither=True)
    check(rows("s16", 2, 300, np.float32), "s16", dither=True, seed=0, frame0=(1 << 50) - 300)


# ---- round trips through the ingest ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt, dtype", ROUND_TRIPS, ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_encode_inverts_decode_on_the_device(hip, fmt, dtype):
    import torch
    C = 3
    T = 2 * tile_frames(fmt, C) + 3
    raw = H.random_raw(fmt, C, T, seed=11)
    H.place(raw, fmt, C, 0, H.edge_values(fmt, dtype == np.float32))
    raw_cuda = torch.from_numpy(raw).cuda()
    got = encode_pcm(decode_pcm(raw_cuda, fmt, C, dtype=dtype), fmt)
    assert torch.equal(got.data, raw_cuda) and got.clipped.tolist() == [0] * C


@pytest.mark.parametrize("fmt", ("s16", "s24", "f32"))
def test_save_wav_then_load_wav(hip, tmp_path, fmt):
    C, rate = 2, 44100
    T = tile_frames(fmt, C) + 11
    x = rows(fmt, C, T, np.float32)
    path = tmp_path / "take.wav"
    for samples in (cuda(x), np.array(x)):
        info = save_wav(path, samples, rate=rate, fmt=fmt, dither=False, slab_bytes=1 << 14)
        assert info == wav_info(path) and (info.fmt, info.channels, info.rate, info.n_frames, info.truncated) == (fmt, C, rate, T, False)
        ref = E.encode(x, fmt)[0]
        assert path.read_bytes() == E_header(fmt, C, rate, T) + ref.tobytes() + (b"\0" if len(ref) & 1 else b"")
        back = load_wav(path, rate=rate, dtype=np.float32)
        want = H.decode(ref, fmt, C, dtype=np.float32)
        assert back.rate_in == rate and np.array_equal(host(back.samples), want, equal_nan=True)
    if fmt == "s16":
        assert E.read_with_wave_module(path)[:4] == (C, 2, rate, T)
        save_wav(path, cuda(x), rate=rate)                                                  # dither=None: on for s16, seed 0
        assert np.fromfile(path, np.uint8)[44:].tobytes() == E.encode(x, "s16", dither_on=True, seed=0)[0].tobytes()
    if fmt == "s24":
        save_wav(path, cuda(x), rate=rate, fmt=fmt)                                         # dither=None: off for s24
        assert np.fromfile(path, np.uint8)[info.data_offset:].tobytes() == E.encode(x, fmt)[0].tobytes()


def E_header(fmt, channels, rate, n_frames):
    from friture_amd.recording import wav_header
    head = wav_header(fmt, channels, rate, n_frames)
    E.check_wav_header(head, fmt, channels, rate, n_frames)
    return head


def test_six_channel_s24_file_is_extensible_and_odd_data_is_padded(hip, tmp_path):
    x = rows("s24", 3, 101, np.float64)
    path = tmp_path / "six.wav"
    info = save_wav(path, cuda(x), rate=96000, fmt="s24", route=[0, 1, 2, -1, 2, 0])
    assert info == (("s24", 6, 96000, 101, 68, 24, False))
    raw = path.read_bytes()
    assert raw[20:22] == b"\xfe\xff" and raw[44:46] == b"\x01\x00" and raw[46:60] == H.GUID_TAIL and len(raw) == 68 + 101 * 18
    assert raw[68:] == E.encode(x, "s24", route=[0, 1, 2, -1, 2, 0])[0].tobytes()
    info = save_wav(path, np.array(x[:1, :5]), rate=8000, fmt="u8", dither=False)          # 5 bytes of data: one pad byte
    assert info == ("u8", 1, 8000, 5, 44, 8, False) and path.stat().st_size == 44 + 5 + 1 and path.read_bytes()[-1] == 0
    info = save_wav(path, np.array(x[:, :0]), fmt="s16")
    assert info.n_frames == 0 and path.stat().st_size == 68


# ---- player mode -----------------------------------------------------------------------------------------------------------------------

def test_player_mode_is_the_reference_block(hip):
    for S, outs, dtype in ((2, 2, np.float32), (1, 4, np.float64), (3, 2, np.float32), (2, 5, np.float64)):
        x = np.array(rows("s16", S, 1500, dtype))
        x[:, 100:108] = np.array([1.5, -1.5, 1.0, -1.0, np.nan, 0.99999, -0.99999, 1.0000001], dtype)
        route = player_route(S, outs)
        ref, clipped = check(x, "s16", route=route, mode="player")
        block = E.player_block(x, outs)
        assert block.shape == (1500, outs) and np.array_equal(ref, H.pack(block, "s16"))
        # the reference's three statements on the routed rows, NaN aside (the reference never meets one)
        routed = np.stack([x[r].astype(np.float64) if r >= 0 else np.zeros(1500) for r in route])
        info = np.iinfo(np.int16)
        res = min(abs(info.min), info.max) * np.clip(np.nan_to_num(routed, nan=0.0), -1.0, 1.0)
        assert np.array_equal(ref, H.pack(res.astype(np.int16).transpose(), "s16"))
        assert clipped.sum() > 0 and not clipped[[c for c, r in enumerate(route) if r < 0]].any()
        assert not np.array_equal(ref, E.encode(x, "s16", route=route)[0])                  # 32767 v truncated is not rint(32768 v)


# ---- stream discipline ----------------------------------------------------------------------------------------------------------------

def test_a_call_on_a_side_stream_is_ordered_behind_the_producer(hip):
    import torch
    T = 1 << 20
    seed = torch.from_numpy(np.array(rows("s16", 2, T, np.float32))).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = seed
        for _ in range(24):                                    # work for the stream to be busy with when the call arrives
            x = torch.sin(x) * 1.25
        got = encode_pcm(x, "s16")
        first = got.data[:64].clone()                          # read on the same stream, no synchronisation in between
        data, x_host = got.data.cpu(), x.cpu()
    side.synchronize()
    ref, clipped = E.encode(x_host.numpy(), "s16")
    assert np.array_equal(data.numpy(), ref) and np.array_equal(host(first), ref[:64]) and got.clipped.tolist() == clipped.tolist()
