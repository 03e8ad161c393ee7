"""PCM export without a GPU: the numpy restatement of the definition (tests/pcmenc_helpers.py) against known answers and
hand-written values, wav_header against wav_info and the stdlib `wave` module, player_route, encode_pcm's argument errors (raised
before the library is loaded) and the refusals of frt_pcmenc_encode (made on the arguments alone: no device call)."""
import ctypes

import numpy as np
import pytest

import pcmenc_helpers as E
import recording_helpers as H
from friture_amd.recording import FORMATS, EncodedPcm, encode_pcm, player_route, save_wav, wav_header, wav_info

# the seven combinations for which encode(decode(raw)) == raw is claimed (s32 through float32 is not)
ROUND_TRIPS = [(fmt, dtype) for fmt in ("u8", "s16", "s24", "s32") for dtype in (np.float32, np.float64) if (fmt, dtype) != ("s32", np.float32)]


# ---- the helper --------------------------------------------------------------------------------------------------------------------

def words(text):
    return [int(w, 16) for w in text.split()]


@pytest.mark.parametrize("counter, key, output", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, output):
    assert E.philox4x32_10(words(counter), words(key)).tolist() == words(output)


def test_philox_is_vectorised_as_it_is_scalar():
    counters = np.array([words("00000000 00000000 00000000 00000000"), words("243f6a88 85a308d3 13198a2e 03707344")], np.uint64)
    out = E.philox4x32_10(counters, words("a4093822 299f31d0"))
    assert out[1].tolist() == words("d16cfe09 94fdcceb 5001e420 24126ea1")
    assert out[0].tolist() == E.philox4x32_10(counters[0], words("a4093822 299f31d0")).tolist()


def test_dither_is_triangular_on_the_open_unit_interval():
    d = E.dither(np.arange(20000) + (1 << 33) - 10000, 3, 0x0123456789ABCDEF)           # frames on both sides of 2^32
    assert d.shape == (20000, 3) and d.dtype == np.float64
    assert d.min() > -1.0 and d.max() < 1.0
    assert np.array_equal(d * 2.0 ** 24, np.rint(d * 2.0 ** 24))
    assert abs(d.mean()) < 0.01 and abs(d.var() - 1 / 6) < 0.01                          # a triangle on (-1, 1): variance 1/6
    assert not np.array_equal(d, E.dither(np.arange(20000) + (1 << 33) - 10000, 3, 1))
    assert np.array_equal(d[5000:5010], E.dither(np.arange(10) + (1 << 33) - 5000, 3, 0x0123456789ABCDEF))
    assert not np.array_equal(d[:, 0], d[:, 1])


@pytest.mark.parametrize("fmt, dtype", ROUND_TRIPS, ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_encode_inverts_decode(fmt, dtype):
    channels = 3
    raw = H.random_raw(fmt, channels, 4001, seed=7)
    H.place(raw, fmt, channels, 5, H.edge_values(fmt, dtype == np.float32))
    got, clipped = E.encode(H.decode(raw, fmt, channels, dtype=dtype), fmt)
    assert np.array_equal(got, raw) and clipped.tolist() == [0] * channels


def test_s32_through_float32_does_not_round_trip():
    raw = H.pack(np.array([(1 << 24) + 1, (1 << 31) - 1], np.int64), "s32")
    got, clipped = E.encode(H.decode(raw, "s32", 1, dtype=np.float32), "s32")
    assert not np.array_equal(got, raw) and clipped.tolist() == [1]                      # 2^31 - 1 rounds to 1.0, which clips


def test_helper_values_by_hand():
    def one(fmt, values, **kw):
        b, c = E.encode(np.array([values], np.float64), fmt, **kw)
        return H.raw_values(b, fmt, 1)[:, 0].tolist(), int(c[0])

    # ties to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0, -1.5 -> -2; the clamp edges; inf and NaN
    lsb = 2.0 ** -15
    assert one("s16", [0.5 * lsb, 1.5 * lsb, 2.5 * lsb, -0.5 * lsb, -1.5 * lsb, -0.0]) == ([0, 2, 2, 0, -2, 0], 0)
    assert one("s16", [1.0, -1.0, 1 - lsb, -1 - lsb, 1 - 0.5 * lsb, -1 - 0.5 * lsb]) == ([32767, -32768, 32767, -32768, 32767, -32768], 3)
    assert one("s16", [np.inf, -np.inf, np.nan, 1e300, -1e300]) == ([32767, -32768, 0, 32767, -32768], 5)
    assert one("u8", [0.0, 1 / 128, -1.0, 127 / 128, 1.0]) == ([0, 1, -128, 127, 127], 1)
    assert E.encode(np.array([[0.0, -1.0, 127 / 128]]), "u8")[0].tolist() == [128, 0, 255]
    assert E.encode(np.array([[-(2.0 ** -23), 0x123456 / 2 ** 23]]), "s24")[0].tolist() == [0xFF, 0xFF, 0xFF, 0x56, 0x34, 0x12]
    assert one("s32", [1.0, -1.0, 1 - 2.0 ** -31, 0.5 * 2.0 ** -31, 1.5 * 2.0 ** -31]) == ([2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 0, 2], 1)
    # float formats: f32 of float64 is one rounding (ties to even, subnormals kept, overflow to infinity)
    b, c = E.encode(np.array([[1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 2.0 ** -149, 1e39, -0.0]]), "f32")
    assert b.view("<f4").tolist() == [1.0, 1 + 2.0 ** -22, 2.0 ** -149, np.inf, 0.0] and np.signbit(b.view("<f4")[4]) and c.tolist() == [0]
    # routing: silence, a repeat, the clip count per OUTPUT channel; silence is not dithered
    x = np.array([[2.0, 0.25], [0.5, -3.0]])
    b, c = E.encode(x, "s16", route=[1, -1, 0, 0])
    assert H.raw_values(b, "s16", 4).tolist() == [[16384, 0, 32767, 32767], [-32768, 0, 8192, 8192]] and c.tolist() == [1, 0, 1, 1]
    b, _ = E.encode(x, "u8", route=[-1, 0], dither_on=True, seed=5)
    assert b[0::2].tolist() == [128, 128]
    # player mode: trunc(32767 * clip(v)), not rint(32768 v)
    assert one("s16", [0.99999, -0.99999, 1.0, -1.0, 2.0, np.nan, 0.5, -0.5], mode="player") == \
        ([32766, -32766, 32767, -32767, 32767, 0, 16383, -16383], 2)


def test_player_block_is_the_reference_block():
    rows = np.array([[0.5, -2.0, 0.99999], [1.0, 0.25, -0.25], [0.1, 0.1, 0.1]])
    assert E.player_block(rows, 2).tolist() == [[16383, 32767], [-32767, 8191], [32766, -8191]]
    assert E.player_block(rows, 4)[:, 2:].tolist() == [[3276, 0]] * 3                     # outputs beyond the rows stay zero
    assert E.player_block(rows[:1], 3).tolist() == [[16383] * 3, [-32767] * 3, [32766] * 3]     # mono goes to every output
    assert E.player_block(rows, 2).dtype == np.int16
    for n_rows, outs in ((1, 3), (3, 2), (3, 4)):
        b, _ = E.encode(rows[:n_rows], "s16", route=player_route(n_rows, outs), mode="player")
        assert np.array_equal(b, H.pack(E.player_block(rows[:n_rows], outs), "s16"))


def test_player_route():
    assert player_route(1, 1) == [0] and player_route(1, 4) == [0, 0, 0, 0]
    assert player_route(2, 2) == [0, 1] and player_route(2, 4) == [0, 1, -1, -1] and player_route(5, 2) == [0, 1]
    for bad in ((0, 2), (2, 0), (-1, 1)):
        with pytest.raises(ValueError):
            player_route(*bad)
    with pytest.raises(TypeError):
        player_route(1.5, 2)


# ---- wav_header ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", (1, 2, 6))
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_wav_info_reads_what_wav_header_writes(tmp_path, fmt, channels):
    n = 37
    raw = H.random_raw(fmt, channels, n, seed=3)
    head = wav_header(fmt, channels, 44100, n)
    E.check_wav_header(head, fmt, channels, 44100, n)
    path = tmp_path / "a.wav"
    path.write_bytes(head + raw.tobytes() + (b"\0" if len(raw) & 1 else b""))
    info = wav_info(path)
    assert (info.fmt, info.channels, info.rate, info.n_frames, info.data_offset) == (fmt, channels, 44100, n, len(head))
    assert info.valid_bits == 8 * FORMATS[fmt][1] and not info.truncated
    assert path.stat().st_size == 8 + int.from_bytes(head[4:8], "little") and path.stat().st_size % 2 == 0
    plain = fmt in ("u8", "s16") and channels <= 2
    assert len(head) == (44 if plain else 68 + (12 if fmt in ("f32", "f64") else 0))
    if plain:
        assert E.read_with_wave_module(path) == (channels, FORMATS[fmt][1], 44100, n, raw.tobytes())


def test_wav_header_pads_odd_data_and_refuses_what_does_not_fit():
    for fmt, channels, n, odd in (("u8", 1, 3, True), ("u8", 1, 4, False), ("s24", 1, 5, True), ("s24", 3, 5, True), ("s16", 1, 5, False)):
        head = wav_header(fmt, channels, 8000, n)
        data = n * channels * FORMATS[fmt][1]
        assert int.from_bytes(head[-4:], "little") == data and data % 2 == int(odd)
        assert int.from_bytes(head[4:8], "little") == len(head) - 8 + data + int(odd)
    assert wav_header("s16", 2, 48000, 0)[-4:] == bytes(4)
    fits = (0xFFFFFFFF - 36) // 4
    assert len(wav_header("s16", 2, 48000, fits)) == 44
    with pytest.raises(ValueError, match="RF64"):
        wav_header("s16", 2, 48000, fits + 1)
    with pytest.raises(ValueError, match="RF64"):
        wav_header("f64", 64, 48000, 1 << 24)
    with pytest.raises(ValueError, match="format"):
        wav_header("s20", 2, 48000, 1)
    with pytest.raises(ValueError, match="channels"):
        wav_header("s16", 65, 48000, 1)
    with pytest.raises(ValueError, match="rate"):
        wav_header("s16", 2, 0, 1)
    with pytest.raises(ValueError, match="frames"):
        wav_header("s16", 2, 48000, -1)


# ---- encode_pcm: argument errors, no device ---------------------------------------------------------------------------------------

def test_encode_pcm_argument_errors_are_raised_on_the_host(tmp_path, monkeypatch):
    from friture_amd import recording

    def loaded():
        raise AssertionError("the library was asked for before the arguments were checked")

    monkeypatch.setattr(recording, "_encoder", loaded)              # on any machine: no check may come behind the load
    shared = recording._shared_encoder
    x = np.zeros((2, 10), np.float32)
    assert EncodedPcm._fields == ("data", "clipped")
    for fmt in ("s20", 1, None):
        with pytest.raises(ValueError, match="format"):
            encode_pcm(x, fmt)
    with pytest.raises(TypeError, match="numpy array or a CUDA tensor"):
        encode_pcm([[0.0, 1.0]], "s16")
    for bad in (x.astype(np.int16), x.astype(np.float16), x.astype(np.complex64)):
        with pytest.raises(TypeError, match="float32 or float64"):
            encode_pcm(bad, "s16")
    for bad in (np.zeros((2, 2, 2), np.float32), np.zeros((), np.float32)):
        with pytest.raises(ValueError, match="expected"):
            encode_pcm(bad, "s16")
    for route in ([2], [-2], [0, 1, 5], [0.0], ["0"], 1):
        with pytest.raises(ValueError, match="route"):
            encode_pcm(x, "s16", route=route)
    for route in ([], [0] * 65):
        with pytest.raises(ValueError, match="channels"):
            encode_pcm(x, "s16", route=route)
    with pytest.raises(ValueError, match="channels"):
        encode_pcm(np.zeros((65, 4), np.float32), "s16")
    for channels in (3, 2.0, True):
        with pytest.raises(ValueError, match="channels"):
            encode_pcm(x, "s16", route=[0, 1], channels=channels)
    for frame0 in (-1, (1 << 50) - 9):
        with pytest.raises(ValueError, match="frame0"):
            encode_pcm(x, "s16", frame0=frame0)
    with pytest.raises(TypeError):
        encode_pcm(x, "s16", frame0=1.5)
    with pytest.raises(ValueError, match="mode"):
        encode_pcm(x, "s16", mode="floor")
    for fmt in ("f32", "f64"):
        with pytest.raises(ValueError, match="dither"):
            encode_pcm(x, fmt, dither=True)
    with pytest.raises(TypeError, match="dither"):
        encode_pcm(x, "s16", dither=1)
    with pytest.raises(ValueError, match="player"):
        encode_pcm(x, "s24", mode="player")
    with pytest.raises(ValueError, match="player"):
        encode_pcm(x, "s16", mode="player", dither=True)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            encode_pcm(x, "s16", dither=True, seed=seed)
    with pytest.raises(ValueError, match="to="):
        encode_pcm(x, "s16", to="cpu")
    with pytest.raises(ValueError, match="slab_bytes"):
        encode_pcm(x, "s16", slab_bytes=-1)
    with pytest.raises(ValueError, match="holds 39 bytes"):
        encode_pcm(x, "s16", out=np.zeros(39, np.uint8))
    for out in (np.zeros(20, np.int16), np.zeros((4, 10), np.uint8), np.zeros(80, np.uint8)[::2], bytearray(40)):
        with pytest.raises(TypeError, match="out"):
            encode_pcm(x, "s16", out=out)
    frozen = np.zeros(40, np.uint8)
    frozen.flags.writeable = False
    with pytest.raises(TypeError, match="writable"):
        encode_pcm(x, "s16", out=frozen)
    with pytest.raises(ValueError, match="not both"):
        encode_pcm(x, "s16", out=np.zeros(40, np.uint8), to="host")
    with pytest.raises(ValueError, match="format"):
        save_wav(tmp_path / "a.wav", x, fmt="s20")
    with pytest.raises(ValueError, match="route"):
        save_wav(tmp_path / "a.wav", x, route=[2])
    assert not (tmp_path / "a.wav").exists()
    assert recording._shared_encoder is shared
    with pytest.raises(AssertionError, match="before the arguments"):      # and a call with nothing wrong does get that far
        encode_pcm(x, "s16")


def test_save_wav_leaves_no_file_when_the_encode_fails(tmp_path, monkeypatch):
    from friture_amd import recording

    def broken():
        raise RuntimeError("no device")

    monkeypatch.setattr(recording, "_encoder", broken)
    path = tmp_path / "take.wav"
    with pytest.raises(RuntimeError, match="no device"):
        save_wav(path, np.zeros((2, 10), np.float32), fmt="s24")
    assert not path.exists()
    info = save_wav(path, np.zeros((2, 0), np.float32), fmt="s24")           # nothing to encode: the header alone
    assert (info.fmt, info.channels, info.n_frames) == ("s24", 2, 0) and path.stat().st_size == 68


# ---- the C entry points that need no device ---------------------------------------------------------------------------------------

def test_c_refusals_come_before_any_device_call():
    """frt_pcmenc_create allocates nothing on the device; every refusal of frt_pcmenc_encode is made on the arguments alone."""
    from friture_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.frt_pcmenc_create(ctypes.byref(h)) == 0 and h.value
    x, dst = np.zeros((2, 10), np.float32), np.zeros(2 * 2 * 10, np.uint8)
    rt = np.array([0, 1], np.int32)
    clipped = np.full(2, 7, np.int64)

    def run(x_dtype=0, n_rows=2, ldx=10, n=10, frame0=0, route=rt, channels=2, fmt=1, mode=0, dither=0, seed=0, slab=0):
        return lib.frt_pcmenc_encode(h, x.ctypes.data, x_dtype, n_rows, ldx, n, frame0, route.ctypes.data, channels, fmt, mode, dither,
                                     seed, dst.ctypes.data, clipped.ctypes.data, slab)

    try:
        for kw, word in (({"fmt": 6}, b"format 6"), ({"fmt": -1}, b"format -1"), ({"x_dtype": 2}, b"x_dtype 2"), ({"mode": 2}, b"mode 2"),
                         ({"mode": -1}, b"mode -1"), ({"dither": 2}, b"dither 2"), ({"channels": 0}, b"0 channels"),
                         ({"channels": 65}, b"65 channels"), ({"n_rows": 0}, b"0 rows"), ({"n_rows": 65536}, b"65536 rows"),
                         ({"route": np.array([0, 2], np.int32)}, b"route[1] = 2"), ({"route": np.array([-2, 0], np.int32)}, b"route[0] = -2"),
                         ({"n": -1}, b"frames 0 .. -1"), ({"frame0": -1}, b"frames -1"), ({"frame0": (1 << 50) - 9}, b"frames 1125899906842615"),
                         ({"frame0": (1 << 50) + 1, "n": 0}, b"frames"), ({"ldx": 9}, b"ldx 9"), ({"slab": -1}, b"slab_bytes -1"),
                         ({"mode": 1, "fmt": 2}, b"mode 1"), ({"mode": 1, "dither": 1}, b"mode 1"), ({"mode": 1, "fmt": 4}, b"mode 1"),
                         ({"dither": 1, "fmt": 4}, b"dither with the float format 4"), ({"dither": 1, "fmt": 5}, b"dither with the float format 5")):
            assert run(**kw) == -1, kw
            assert b"frt_pcmenc_encode" in lib.frt_last_error() and word in lib.frt_last_error(), (kw, lib.frt_last_error())
        assert lib.frt_pcmenc_encode(h, x.ctypes.data, 0, 2, 10, 10, 0, None, 2, 1, 0, 0, 0, dst.ctypes.data, None, 0) == -1
        assert b"route" in lib.frt_last_error()
        assert run(n=0) == 0 and run(n=0, frame0=1 << 50) == 0 and run(n=0, ldx=0, dither=1, seed=(1 << 64) - 1) == 0      # nothing to do
        assert clipped.tolist() == [7, 7] and not dst.any()
    finally:
        lib.frt_pcmenc_destroy(h)              # a handle that never reached the device: no device call here either
    lib.frt_pcmenc_destroy(None)
    assert lib.frt_pcmenc_encode(None, None, 0, 1, 0, 0, 0, None, 1, 0, 0, 0, 0, None, None, 0) == -1
    assert b"null handle" in lib.frt_last_error()
    assert lib.frt_pcmenc_set_stream(None, None) == -1 and lib.frt_pcmenc_create(None) == -1
