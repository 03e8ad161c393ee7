"""recording.py without a GPU: wav_info on files written by the stdlib `wave` module and on hand-built headers, its refusals,
decode_pcm's argument errors (raised before the library is loaded), frt_pcm_tile_frames (pure host), and the numpy restatement
of the definition (tests/recording_helpers.py) against hand-written expected values."""
import ctypes
import struct
import wave

import numpy as np
import pytest

import recording_helpers as H
from friture_amd.recording import FORMATS, Recording, WavInfo, decode_pcm, tile_frames, wav_info

LDS_BUDGET = 32768


def frames_of(fmt, channels, n, seed=1):
    return H.random_raw(fmt, channels, n, seed)


# ---- wav_info: files of the stdlib writer -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", (1, 2, 3))
@pytest.mark.parametrize("fmt", ("u8", "s16", "s24", "s32"))
def test_wav_info_reads_what_wave_writes(tmp_path, fmt, channels):
    raw = frames_of(fmt, channels, 37)
    path = tmp_path / "a.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(FORMATS[fmt][1])
        w.setframerate(44100)
        w.writeframes(raw.tobytes())
    info = wav_info(path)
    assert info == WavInfo(fmt, channels, 44100, 37, 44, 8 * FORMATS[fmt][1], False)
    assert np.array_equal(np.fromfile(path, np.uint8)[info.data_offset:info.data_offset + len(raw)], raw)


# ---- wav_info: hand-built headers -----------------------------------------------------------------------------------------------------

def test_float32_and_float64_tag_3(tmp_path):
    for fmt in ("f32", "f64"):
        raw = frames_of(fmt, 2, 10)
        info = wav_info(H.write_wav(tmp_path / f"{fmt}.wav", raw, fmt, 2, 96000))
        assert info == WavInfo(fmt, 2, 96000, 10, 44, 8 * FORMATS[fmt][1], False)


def test_extensible_pcm_24_bit_6_channels(tmp_path):
    raw = frames_of("s24", 6, 11)
    info = wav_info(H.write_wav(tmp_path / "e.wav", raw, "s24", 6, 48000, extensible=True))
    assert info == WavInfo("s24", 6, 48000, 11, 12 + 8 + 40 + 8, 24, False)


def test_extensible_float(tmp_path):
    raw = frames_of("f32", 4, 9)
    info = wav_info(H.write_wav(tmp_path / "e.wav", raw, "f32", 4, 48000, extensible=True))
    assert info == WavInfo("f32", 4, 48000, 9, 68, 32, False)


def test_list_chunk_before_data(tmp_path):
    raw = frames_of("s16", 2, 12)
    before = [H.chunk(b"LIST", b"INFOISFT" + struct.pack("<I", 4) + b"abc\0"), H.chunk(b"fact", struct.pack("<I", 12))]
    info = wav_info(H.write_wav(tmp_path / "l.wav", raw, "s16", 2, 44100, before=before))
    assert info == WavInfo("s16", 2, 44100, 12, 44 + 8 + 16 + 8 + 4, 16, False)
    assert np.array_equal(np.fromfile(tmp_path / "l.wav", np.uint8)[info.data_offset:], raw)


def test_odd_sized_chunk_before_data_is_padded(tmp_path):
    raw = frames_of("s16", 1, 12)
    info = wav_info(H.write_wav(tmp_path / "o.wav", raw, "s16", 1, 8000, before=[H.chunk(b"junk", b"12345")]))
    assert info == WavInfo("s16", 1, 8000, 12, 44 + 8 + 6, 16, False)
    assert np.array_equal(np.fromfile(tmp_path / "o.wav", np.uint8)[info.data_offset:], raw)


@pytest.mark.parametrize("size", (0, 0xFFFFFFFF))
def test_streamed_data_size_is_clamped_to_the_frames_present(tmp_path, size):
    raw = frames_of("s16", 2, 21)
    info = wav_info(H.write_wav(tmp_path / "s.wav", raw, "s16", 2, 44100, data_size=size))
    assert info == WavInfo("s16", 2, 44100, 21, 44, 16, True)


def test_data_past_the_end_of_the_file_ending_inside_a_frame(tmp_path):
    raw = frames_of("s24", 2, 10)
    info = wav_info(H.write_wav(tmp_path / "t.wav", raw[:-2], "s24", 2, 44100, data_size=len(raw) + 600))
    assert info == WavInfo("s24", 2, 44100, 9, 44, 24, True)


def test_valid_bits_20_in_a_24_bit_container(tmp_path):
    raw = frames_of("s24", 2, 10)
    assert wav_info(H.write_wav(tmp_path / "x.wav", raw, "s24", 2, 48000, extensible=True, valid_bits=20)) == \
        WavInfo("s24", 2, 48000, 10, 68, 20, False)
    assert wav_info(H.write_wav(tmp_path / "p.wav", raw, "s24", 2, 48000, valid_bits=20)) == WavInfo("s24", 2, 48000, 10, 44, 20, False)


# ---- wav_info: refusals ---------------------------------------------------------------------------------------------------------------

def data_chunk(n=8):
    return H.chunk(b"data", bytes(n))


def test_refusals_name_their_cause(tmp_path):
    def refuse(name, content, match):
        path = tmp_path / name
        path.write_bytes(content)
        with pytest.raises(ValueError, match=match):
            wav_info(path)

    good = H.fmt_chunk(1, 2, 44100, 2)
    refuse("a.wav", b"RIFX" + bytes(40), "not a RIFF/WAVE")
    refuse("b.wav", H.riff([good, data_chunk()], kind=b"AVI "), "not a RIFF/WAVE")
    refuse("c.wav", b"RIFF", "not a RIFF/WAVE")
    refuse("d.wav", H.riff([good, data_chunk()], form=b"RF64"), "RF64")
    refuse("e.wav", H.riff([good, data_chunk()], form=b"BW64"), "BW64")
    refuse("f.wav", H.riff([H.fmt_chunk(0x0055, 2, 44100, 2), data_chunk()]), "format tag 0x0055")               # MP3
    refuse("g.wav", H.riff([H.fmt_chunk(2, 2, 44100, 2), data_chunk()]), "compressed")                           # ADPCM
    refuse("h.wav", H.riff([H.fmt_chunk(1, 2, 44100, 2, extensible=True, sub_tail=bytes(14)), data_chunk()]), "sub-format")
    refuse("i.wav", H.riff([H.fmt_chunk(0x0161, 2, 44100, 2, extensible=True), data_chunk()]), "sub-format")      # WMA in extensible
    refuse("j.wav", H.riff([H.fmt_chunk(1, 2, 44100, 2, block_align=5), data_chunk()]), "block_align 5")
    refuse("k.wav", H.riff([H.fmt_chunk(1, 2, 44100, 2, bits=24), data_chunk()]), "block_align 4")              # 24 bits do not fit
    refuse("l.wav", H.riff([data_chunk(), good]), "no fmt chunk before")
    refuse("m.wav", H.riff([good, H.chunk(b"LIST", bytes(10))]), "no data chunk")
    refuse("n.wav", H.riff([H.fmt_chunk(1, 65, 44100, 2), data_chunk()]), "more than 64 channels")
    refuse("o.wav", H.riff([H.fmt_chunk(1, 2, 44100, 5), data_chunk()]), "5 bytes are not supported")
    refuse("p.wav", H.riff([H.fmt_chunk(3, 2, 44100, 2), data_chunk()]), "float samples of 2 bytes")
    refuse("q.wav", H.riff([H.chunk(b"fmt ", bytes(10)), data_chunk()]), "fmt chunk of 10 bytes")


# ---- decode_pcm: argument errors, no device --------------------------------------------------------------------------------------------

def test_decode_pcm_argument_errors_are_raised_on_the_host():
    raw = np.zeros(4 * 2 * 10, np.uint8)
    with pytest.raises(ValueError, match="format"):
        decode_pcm(raw, "s20", 2)
    with pytest.raises(ValueError, match="format"):
        decode_pcm(raw, 1, 2)
    for channels in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="channels"):
            decode_pcm(raw, "s16", channels)
    with pytest.raises(ValueError, match="whole number of frames"):
        decode_pcm(raw[:-1], "s16", 2)
    with pytest.raises(ValueError, match="whole number of frames"):
        decode_pcm(raw[:10], "s24", 1)
    for select in ([2], [-1], [0, 1, 5], [0.0], [1.5], ["0"], 1):
        with pytest.raises(ValueError, match="select"):
            decode_pcm(raw, "s16", 2, select=select)
    with pytest.raises(ValueError, match="selected channels"):
        decode_pcm(raw, "s16", 2, select=[])
    for start, count in ((-1, None), (21, None), (0, 21), (15, 6), (0, -1)):
        with pytest.raises(ValueError, match="frames"):
            decode_pcm(raw, "s16", 2, start=start, count=count)
    for dtype in (np.int16, np.float16, "complex64", object):
        with pytest.raises(TypeError, match="float32 or float64"):
            decode_pcm(raw, "s16", 2, dtype=dtype)
    with pytest.raises(ValueError, match="to="):
        decode_pcm(raw, "s16", 2, to="cpu")
    with pytest.raises(ValueError, match="slab_bytes"):
        decode_pcm(raw, "s16", 2, slab_bytes=-1)
    with pytest.raises(TypeError, match="uint8"):
        decode_pcm(raw.view(np.int16), "s16", 2)
    with pytest.raises(TypeError, match="uint8"):
        decode_pcm(raw.reshape(2, -1), "s16", 2)
    with pytest.raises(TypeError):
        decode_pcm(3.5, "s16", 2)


def test_formats_table():
    assert FORMATS == H.FORMATS == {"u8": (0, 1), "s16": (1, 2), "s24": (2, 3), "s32": (3, 4), "f32": (4, 4), "f64": (5, 8)}
    assert Recording._fields == ("samples", "rate_in", "info")
    assert WavInfo._fields == ("fmt", "channels", "rate", "n_frames", "data_offset", "valid_bits", "truncated")


# ---- the C entry points that need no device ---------------------------------------------------------------------------------------------

def test_tile_frames_without_a_gpu():
    from friture_amd import _lib
    lib = _lib.load()
    for fmt, (code, width) in FORMATS.items():
        for channels in (1, 2, 3, 8, 64):
            F = lib.frt_pcm_tile_frames(code, channels)
            assert F == tile_frames(fmt, channels) and F >= 64 and F % 64 == 0
            assert F * channels * width <= LDS_BUDGET < (F + 64) * channels * width, (fmt, channels, F)
    for fmt_code, channels in ((6, 2), (-1, 2), (1, 0), (1, 65)):
        assert lib.frt_pcm_tile_frames(fmt_code, channels) == -1
        assert b"frt_pcm_tile_frames" in lib.frt_last_error()
    with pytest.raises(ValueError):
        tile_frames("s16", 65)


def test_c_refusals_come_before_any_device_call():
    """frt_pcm_create allocates nothing on the device; every refusal of frt_pcm_decode is made on the arguments alone."""
    from friture_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.frt_pcm_create(ctypes.byref(h)) == 0 and h.value
    raw, y = np.zeros(2 * 2 * 10, np.uint8), np.zeros((2, 10), np.float32)
    sel = np.array([0, 1], np.int32)

    def run(fmt=1, channels=2, total=10, first=0, n=10, select=sel, n_select=2, y_dtype=0, ldy=10, slab=0):
        return lib.frt_pcm_decode(h, raw.ctypes.data, fmt, channels, total, first, n, select.ctypes.data, n_select, y.ctypes.data,
                                  y_dtype, ldy, slab)

    try:
        refusals(lib, run)
    finally:
        lib.frt_pcm_destroy(h)                 # a handle that never reached the device: no device call here either
    lib.frt_pcm_destroy(None)


def refusals(lib, run):
    for kw, word in (({"fmt": 6}, b"format 6"), ({"fmt": -1}, b"format -1"), ({"y_dtype": 2}, b"y_dtype 2"), ({"channels": 0}, b"0 channels"),
                     ({"channels": 65}, b"65 channels"), ({"n_select": 0}, b"0 selected"), ({"n_select": 65536}, b"65536 selected"),
                     ({"select": np.array([0, 2], np.int32)}, b"select[1] = 2"), ({"select": np.array([-1, 0], np.int32)}, b"select[0] = -1"),
                     ({"first": 11, "n": 0}, b"frames 11"), ({"first": 5, "n": 6}, b"frames 5 .. 11"), ({"first": -1}, b"frames -1"),
                     ({"n": -1}, b"frames"), ({"total": -1, "n": 0}, b"frames"), ({"ldy": 9}, b"ldy 9"), ({"slab": -1}, b"slab_bytes")):
        assert run(**kw) == -1, kw
        assert b"frt_pcm_decode" in lib.frt_last_error() and word in lib.frt_last_error(), (kw, lib.frt_last_error())
    assert run(n=0) == 0 and run(first=10, n=0) == 0                                   # nothing to do: no device call either
    assert lib.frt_pcm_decode(None, None, 0, 1, 0, 0, 0, None, 0, None, 0, 0, 0) == -1


# ---- the helper ---------------------------------------------------------------------------------------------------------------------

def test_helper_edge_values_per_format():
    def one(fmt, raw_bytes, dtype=np.float64):
        return H.decode(np.array(raw_bytes, np.uint8), fmt, 1, dtype=dtype)[0].tolist()

    assert one("u8", [0, 127, 128, 129, 255]) == [-1.0, -1 / 128, 0.0, 1 / 128, 127 / 128]
    assert one("s16", [0x00, 0x80, 0xFF, 0x7F, 0xFF, 0xFF, 0x00, 0x00, 0x01, 0x00]) == [-1.0, 32767 / 32768, -1 / 32768, 0.0, 1 / 32768]
    assert one("s24", [0x00, 0x00, 0x80, 0xFF, 0xFF, 0x7F, 0xFF, 0xFF, 0xFF, 0x01, 0x00, 0x00, 0x56, 0x34, 0x12]) == \
        [-1.0, (2 ** 23 - 1) / 2 ** 23, -(2.0 ** -23), 2.0 ** -23, 0x123456 / 2 ** 23]
    assert one("s32", [0, 0, 0, 0x80, 0xFF, 0xFF, 0xFF, 0x7F, 0xFF, 0xFF, 0xFF, 0xFF, 1, 0, 0, 0]) == \
        [-1.0, (2 ** 31 - 1) / 2 ** 31, -(2.0 ** -31), 2.0 ** -31]
    # float32 of s32: one rounding of the exact value.  2^24 + 1 and 2^24 + 3 are ties of the 24-bit grid (to even: down, up);
    # 2^31 - 65 rounds down to 1 - 2^-24, 2^31 - 64 is the tie that rounds up to 1.0; INT32_MIN is -1 exactly
    v = np.array([(1 << 24) + 1, (1 << 24) + 3, (1 << 31) - 65, (1 << 31) - 64, (1 << 31) - 1, -(1 << 31), -(1 << 24) - 1], np.int64)
    got = H.decode(H.pack(v, "s32"), "s32", 1, dtype=np.float32)[0]
    assert got.dtype == np.float32
    assert got.tolist() == [2.0 ** -7, 2.0 ** -7 + 2.0 ** -29, 1 - 2.0 ** -24, 1.0, 1.0, -1.0, -(2.0 ** -7)]
    # the same from exact rationals
    from fractions import Fraction
    for x, g in zip(v.tolist(), got.tolist()):
        exact = Fraction(x, 2 ** 31)
        lo, hi = np.nextafter(np.float32(g), np.float32(-2)), np.nextafter(np.float32(g), np.float32(2))
        assert abs(Fraction(g) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    # u8, s16, s24 are exact in float32
    for fmt in ("u8", "s16", "s24"):
        raw = H.random_raw(fmt, 1, 4096, 3)
        assert np.array_equal(H.decode(raw, fmt, 1, dtype=np.float32).astype(np.float64), H.decode(raw, fmt, 1, dtype=np.float64))
    # f64 -> float32: ties to even, the largest finite value, subnormals kept
    f = H.decode(H.pack(np.array([1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, float(np.finfo(np.float32).max), 2.0 ** -140, 3 * 2.0 ** -150, 2.0 ** -150]),
                        "f64"), "f64", 1, dtype=np.float32)[0]
    assert f.tolist() == [1.0, 1 + 2.0 ** -22, float(np.finfo(np.float32).max), 2.0 ** -140, 2.0 ** -148, 0.0]
    z = H.decode(H.pack(np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32), "f32"), "f32", 1, dtype=np.float64)[0]
    assert z[:4].tolist() == [0.0, 0.0, np.inf, -np.inf] and np.signbit(z[1]) and not np.signbit(z[0]) and np.isnan(z[4])


@pytest.mark.parametrize("fmt", sorted(H.FORMATS))
def test_pack_and_helper_round_trip(fmt):
    rng = np.random.default_rng(5)
    if fmt in H.INT_BITS:
        lo, hi = H.int_range(fmt)
        v = np.concatenate([rng.integers(lo, hi + 1, (50, 3)), [[lo, hi, -1], [0, 1, lo]]])
        raw = H.pack(v, fmt)
        assert raw.dtype == np.uint8 and raw.shape == (52 * 3 * H.FORMATS[fmt][1],)
        assert np.array_equal(H.raw_values(raw, fmt, 3), v)
        assert np.array_equal(H.decode(raw, fmt, 3, dtype=np.float64), v.T * 2.0 ** -(H.INT_BITS[fmt] - 1))
    else:
        v = rng.standard_normal((52, 3)).astype(np.float32 if fmt == "f32" else np.float64)
        raw = H.pack(v, fmt)
        assert np.array_equal(H.decode(raw, fmt, 3, dtype=v.dtype), v.T)
    assert np.array_equal(H.decode(raw, fmt, 3, select=[2, 0, 2], start=7, count=11, dtype=np.float64),
                          H.decode(raw, fmt, 3, dtype=np.float64)[[2, 0, 2], 7:18])
    assert H.decode(raw, fmt, 3, start=52, dtype=np.float32).shape == (3, 0)
    assert np.array_equal(H.raw_values(H.random_raw(fmt, 2, 9, 1), fmt, 2), H.raw_values(H.random_raw(fmt, 2, 9, 1), fmt, 2))
