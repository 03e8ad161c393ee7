"""PCM ingest on the GPU (pcm.hip, recording.py) against the numpy restatement of tests/recording_helpers.py, which
test_recording_cpu.py checks against hand-written values.  The output is defined to the bit, so every comparison is
np.array_equal (equal_nan where the input holds NaNs).  Shapes are a few tiles at most: F = tile_frames(fmt, C) frames is what one
workgroup decodes."""
import functools
import wave

import numpy as np
import pytest

import recording_helpers as H
from friture_amd import _batchio
from friture_amd.recording import FORMATS, decode_pcm, load_wav, tile_frames, wav_info
from friture_amd.resample import Resampler, to_48k

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)


def equal(got, ref):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True) and \
        np.array_equal(np.signbit(got), np.signbit(ref))


@functools.lru_cache(maxsize=None)
def buffer(fmt, channels, frames, seed=0):
    """Seeded bytes with the edge values at the start, across the first tile edge and at the end (read-only, shared)."""
    raw = H.random_raw(fmt, channels, frames, 1000 * seed + 7 * channels + frames)
    edges = np.concatenate([H.edge_values(fmt, True)] * 2)
    F = tile_frames(fmt, channels)
    per = -(-len(edges) // channels)
    for at in (0, F - per // 2, frames - per):
        if 0 <= at <= frames - 1:
            H.place(raw, fmt, channels, at, edges)
    raw.setflags(write=False)
    return raw


def cuda_bytes(raw, offset=0, pad=0):
    """`raw` on the device at byte `offset` of a fresh tensor with `pad` bytes behind it."""
    import torch
    t = torch.full((offset + len(raw) + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    t[offset:offset + len(raw)] = torch.from_numpy(np.array(raw))
    return t[offset:offset + len(raw)]


# ---- the main grid ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", (1, 2, 3, 8))
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_every_format_and_length_is_bit_exact(hip, fmt, channels):
    F = tile_frames(fmt, channels)
    for T in (0, 1, 63, F - 1, F, F + 1, 2 * F + 5):
        raw = buffer(fmt, channels, T)
        dev = cuda_bytes(raw)
        for dtype in DTYPES:
            got = decode_pcm(dev, fmt, channels, dtype=dtype)
            assert got.is_cuda and tuple(got.shape) == (channels, T)
            assert equal(got, H.decode(raw, fmt, channels, dtype=dtype)), (fmt, channels, T, dtype)
        assert np.array_equal(dev.cpu().numpy(), raw)


@pytest.mark.parametrize("channels", (32, 64))
@pytest.mark.parametrize("fmt", ("s32", "f64"))
def test_wide_frames(hip, fmt, channels):
    F = tile_frames(fmt, channels)
    raw = buffer(fmt, channels, F + 1)
    for dtype in DTYPES:
        assert equal(decode_pcm(cuda_bytes(raw), fmt, channels, dtype=dtype), H.decode(raw, fmt, channels, dtype=dtype))
        assert equal(decode_pcm(cuda_bytes(raw, 4), fmt, channels, dtype=dtype), H.decode(raw, fmt, channels, dtype=dtype))


@pytest.mark.parametrize("fmt,channels,select", (("s16", 8, [7, 6, 5, 4, 3, 2, 1, 0]), ("s24", 3, [1, 1, 0, 2, 1]), ("u8", 8, [5]), ("f32", 8, [5]),
                                                 ("s32", 64, [63, 17]), ("f64", 64, [0, 41])))
def test_select(hip, fmt, channels, select):
    F = tile_frames(fmt, channels)
    raw = buffer(fmt, channels, F + 70)
    for dtype in DTYPES:
        got = decode_pcm(cuda_bytes(raw), fmt, channels, select=select, dtype=dtype)
        assert equal(got, H.decode(raw, fmt, channels, select=select, dtype=dtype))
        assert equal(got, H.decode(raw, fmt, channels, dtype=dtype)[select])


@pytest.mark.parametrize("fmt,channels", (("s16", 2), ("s24", 3), ("f64", 2), ("u8", 1)))
def test_sub_ranges_equal_the_slice_of_the_whole(hip, fmt, channels):
    F = tile_frames(fmt, channels)
    T = 3 * F + 11
    raw = buffer(fmt, channels, T)
    dev = cuda_bytes(raw)
    whole = H.decode(raw, fmt, channels, dtype=np.float32)
    for start, count in ((5, 7), (F - 3, 6), (F + 9, F), (1, 2 * F + 1), (F, F), (T - 1, 1), (T, 0), (2 * F - 1, F + 12), (0, T)):
        assert equal(decode_pcm(dev, fmt, channels, start=start, count=count), whole[:, start:start + count]), (start, count)
        assert equal(decode_pcm(np.array(raw), fmt, channels, start=start, count=count, slab_bytes=1), whole[:, start:start + count])


@pytest.mark.parametrize("fmt", ("u8", "s24", "s16", "f64"))
def test_any_byte_alignment(hip, fmt):
    channels = 3 if fmt == "s24" else 2
    F = tile_frames(fmt, channels)
    raw = buffer(fmt, channels, F + 37)
    ref = {dtype: H.decode(raw, fmt, channels, dtype=dtype) for dtype in DTYPES}
    for offset in (1, 2, 3, 4, 7, 8, 15, 44):
        dev = cuda_bytes(raw, offset, 5)
        assert dev.data_ptr() % 16 == offset % 16
        for dtype in DTYPES:
            assert equal(decode_pcm(dev, fmt, channels, dtype=dtype), ref[dtype]), (fmt, offset, dtype)


OWN_BLOCK = 12 << 20        # above 10 MB the caching allocator asks the driver for the request rounded up to 2 MB: a block of its own


@pytest.mark.parametrize("fmt,channels", (("s16", 2), ("s24", 1), ("f32", 3)))
def test_buffer_at_the_start_and_at_the_end_of_its_allocation(hip, fmt, channels):
    """Only the caller's bytes are read.  The buffer is the first and then the last len(raw) bytes of a device allocation that
    is exactly one driver block: a 12 MB tensor taken with the allocator's cache empty, which the growth of the reserved
    memory by exactly its size confirms.  Then the bytes around a slice do not matter.  Results only are asserted."""
    import torch
    F = tile_frames(fmt, channels)
    raw = buffer(fmt, channels, F + 3)
    ref = H.decode(raw, fmt, channels)
    data = torch.from_numpy(np.array(raw)).cuda()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_reserved()
    block = torch.empty((OWN_BLOCK,), dtype=torch.uint8, device="cuda")
    assert torch.cuda.memory_reserved() - before == OWN_BLOCK, "the tensor is not a driver allocation of its own"
    block[:len(raw)] = data
    block[-len(raw):] = data
    first, last = block[:len(raw)], block[-len(raw):]
    assert first.data_ptr() == block.data_ptr() and last.data_ptr() + len(raw) == block.data_ptr() + OWN_BLOCK
    assert equal(decode_pcm(first, fmt, channels), ref)
    assert equal(decode_pcm(last, fmt, channels), ref)
    # and not tile-aligned within the block: the last frames alone, which end at the allocation's last byte
    frame = channels * FORMATS[fmt][1]
    assert equal(decode_pcm(block[-5 * frame:], fmt, channels), ref[:, -5:])
    assert equal(decode_pcm(block[:5 * frame], fmt, channels), ref[:, :5])
    for fill in (0x00, 0xFF):
        mid = torch.full((len(raw) + 64,), fill, dtype=torch.uint8, device="cuda")
        mid[21:21 + len(raw)] = data
        assert equal(decode_pcm(mid[21:21 + len(raw)], fmt, channels), ref)


def test_rows_of_a_wider_output_keep_what_lies_behind_them(hip):
    """ldy > T through the C ABI: the output is a view of a larger tensor whose other columns keep a sentinel."""
    import ctypes

    import torch
    from friture_amd import _lib
    fmt, channels = "s24", 2
    F = tile_frames(fmt, channels)
    T, ld = F + 9, F + 50
    raw = buffer(fmt, channels, T)
    dev = cuda_bytes(raw)
    sel = np.array([1, 0], np.int32)
    h = ctypes.c_void_p()
    _lib.check(hip.frt_pcm_create(ctypes.byref(h)))
    try:
        for dtype in DTYPES:
            out = torch.full((2, ld), -7.0, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
            host = np.full((2, ld), -7.0, dtype)
            for y in (out, host):
                _lib.check(hip.frt_pcm_decode(h, dev.data_ptr(), FORMATS[fmt][0], channels, T, 0, T, sel.ctypes.data, 2, _batchio.ptr(y),
                                              int(dtype == np.float64), ld, 0))
                y = y.cpu().numpy() if y is out else y
                assert np.array_equal(y[:, :T], H.decode(raw, fmt, channels, select=[1, 0], dtype=dtype))
                assert np.all(y[:, T:] == -7.0)
    finally:
        hip.frt_pcm_destroy(h)


# ---- host data ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,channels", (("s16", 2), ("s24", 8), ("f64", 1)))
def test_host_bytes_to_numpy_and_to_cuda(hip, fmt, channels):
    F = tile_frames(fmt, channels)
    raw = buffer(fmt, channels, F + 21)
    for dtype in DTYPES:
        ref = H.decode(raw, fmt, channels, dtype=dtype)
        got = decode_pcm(raw, fmt, channels, dtype=dtype)
        assert isinstance(got, np.ndarray) and equal(got, ref)
        dev = decode_pcm(raw, fmt, channels, dtype=dtype, to="cuda")
        assert dev.is_cuda and equal(dev, ref)
        assert equal(decode_pcm(bytes(raw), fmt, channels, dtype=dtype), ref)                # any buffer
        assert equal(decode_pcm(cuda_bytes(raw), fmt, channels, dtype=dtype, to="cuda"), ref)


def test_memmap_at_a_data_offset_of_44(hip, tmp_path):
    raw = buffer("s24", 2, 3000)
    path = tmp_path / "raw.bin"
    path.write_bytes(bytes(44) + raw.tobytes())
    mm = np.memmap(path, np.uint8, "r", offset=44)
    assert equal(decode_pcm(mm, "s24", 2, to="cuda"), H.decode(raw, "s24", 2))
    assert equal(decode_pcm(mm, "s24", 2, dtype=np.float64), H.decode(raw, "s24", 2, dtype=np.float64))


@pytest.mark.parametrize("fmt,channels", (("s16", 2), ("s24", 3), ("s32", 32)))
def test_slab_size_does_not_change_a_bit(hip, fmt, channels):
    """2F * 7 + 3 frames in slabs of one tile, of three tiles and in one slab: both page-locked blocks are reused several times."""
    F = tile_frames(fmt, channels)
    T = 2 * F * 7 + 3
    raw = buffer(fmt, channels, T)
    tile = F * channels * FORMATS[fmt][1]
    for dtype in DTYPES:
        ref = H.decode(raw, fmt, channels, select=[channels - 1, 0], dtype=dtype)
        for slab in (tile, 3 * tile, 3 * tile + 100, len(raw) + tile, None):
            assert equal(decode_pcm(raw, fmt, channels, select=[channels - 1, 0], dtype=dtype, slab_bytes=slab), ref), (dtype, slab)
            assert equal(decode_pcm(raw, fmt, channels, select=[channels - 1, 0], dtype=dtype, slab_bytes=slab, to="cuda"), ref), (dtype, slab)
        assert equal(decode_pcm(cuda_bytes(raw), fmt, channels, select=[channels - 1, 0], dtype=dtype, slab_bytes=tile), ref)


def test_calls_of_growing_and_shrinking_sizes_on_one_handle(hip):
    F = tile_frames("s16", 2)
    for T in (100, 5 * F + 1, 17, 9 * F, 3):
        raw = buffer("s16", 2, T, seed=T)
        assert equal(decode_pcm(raw, "s16", 2, dtype=np.float64), H.decode(raw, "s16", 2, dtype=np.float64))
        assert equal(decode_pcm(raw, "s16", 2, to="cuda", slab_bytes=2 * F * 4), H.decode(raw, "s16", 2))


# ---- load_wav -----------------------------------------------------------------------------------------------------------------------

def sine_file(path, rate, frames=5000, channels=2):
    t = np.arange(frames)
    x = np.stack([0.5 * np.sin(2 * np.pi * 1000.0 * t / rate + 0.3 * c) for c in range(channels)], axis=1)
    raw = H.pack(np.round(x * 32767).astype(np.int64), "s16")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(raw.tobytes())
    return raw


@pytest.mark.parametrize("dtype", DTYPES)
def test_load_wav_44100_is_the_resampler_on_the_helper(hip, tmp_path, dtype):
    raw = sine_file(tmp_path / "a.wav", 44100)
    rec = load_wav(tmp_path / "a.wav", dtype=dtype)
    assert rec.rate_in == 44100 and rec.info == wav_info(tmp_path / "a.wav") and rec.info.n_frames == 5000
    ref = Resampler(44100).run(H.decode(raw, "s16", 2, dtype=dtype)).y
    assert rec.samples.is_cuda and tuple(rec.samples.shape) == (2, -(-5000 * 160 // 147)) and equal(rec.samples, ref)
    host = load_wav(tmp_path / "a.wav", dtype=dtype, to=None)
    assert isinstance(host.samples, np.ndarray) and equal(host.samples, ref)
    one = load_wav(tmp_path / "a.wav", select=[1], dtype=dtype)
    assert tuple(one.samples.shape) == (1, ref.shape[1]) and equal(one.samples, ref[1:])


def test_load_wav_48000_comes_back_as_decoded(hip, tmp_path):
    raw = sine_file(tmp_path / "b.wav", 48000, frames=700)
    rec = load_wav(tmp_path / "b.wav")
    assert rec.rate_in == 48000 and equal(rec.samples, H.decode(raw, "s16", 2))
    assert equal(load_wav(tmp_path / "b.wav", dtype=np.float64, select=[1, 0], to=None).samples, H.decode(raw, "s16", 2, select=[1, 0], dtype=np.float64))


def test_load_wav_extensible_24_bit_6_channels(hip, tmp_path):
    raw = buffer("s24", 6, 1234)
    H.write_wav(tmp_path / "e.wav", raw, "s24", 6, 48000, extensible=True, before=[H.chunk(b"LIST", b"INFO\0")])
    rec = load_wav(tmp_path / "e.wav", dtype=np.float64)
    assert rec.info.fmt == "s24" and rec.info.channels == 6 and equal(rec.samples, H.decode(raw, "s24", 6, dtype=np.float64))
    pairs = rec.samples.reshape(3, 2, -1)                                 # the view a dual_channels chain takes
    assert pairs.data_ptr() == rec.samples.data_ptr() and equal(pairs[1, 1], H.decode(raw, "s24", 6, dtype=np.float64)[3])


def test_loaded_recording_goes_straight_into_a_chain(hip, tmp_path):
    """SpectrumBatch on load_wav's samples equals SpectrumBatch on the numpy-decoded, to_48k'd array: shape, dtype and device
    are what the chains take."""
    import torch
    from friture_amd.spectrum import SpectrumBatch
    raw = sine_file(tmp_path / "c.wav", 44100, frames=22050)
    rec = load_wav(tmp_path / "c.wav")
    ref_x = torch.from_numpy(to_48k(H.decode(raw, "s16", 2), 44100)).cuda()
    assert rec.samples.dtype == torch.float32 and tuple(rec.samples.shape) == tuple(ref_x.shape) == (2, 24000)
    a, b = SpectrumBatch().run(rec.samples), SpectrumBatch().run(ref_x)
    for name, u, v in zip(a._fields[:-1], _batchio.to_host(a)[:-1], _batchio.to_host(b)[:-1]):
        assert np.array_equal(u, v), name
    for u, v in zip(_batchio.to_host(a.state)[:2], _batchio.to_host(b.state)[:2]):
        assert np.array_equal(u, v)
    assert a.state.pending == b.state.pending and a.db.shape[1] > 10
