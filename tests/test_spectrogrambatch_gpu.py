"""SpectrogramBatch on the GPU (specgrambatch.hip): the kernel on given frames against the numpy replay of the widget chain
(oracle.spectrogrambatch, pinned to the reference by test_spectrogrambatch_cpu), the whole route against the replay and against
SpectrogramStream fed chunk by chunk, and its invariances."""
import ctypes
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from conftest import synth
from oracle import spectrogrambatch as H
from oracle.cases import chunk_ends

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "spectrogrambatch"


@pytest.fixture(scope="module")
def gold():
    return H.load_golden(GOLDEN)


def scales():
    from friture_amd.plotting import frequency_scales as fscales
    return {"linear": fscales.Linear, "log": fscales.Logarithmic, "mel": fscales.Mel, "erb": fscales.Erb, "octave": fscales.Octave}


def batch_of(case):
    from friture_amd.spectrogram import SpectrogramBatch
    keys = ("fft_size", "overlap", "spec_min", "spec_max", "weighting", "minfreq", "maxfreq", "screen_width", "screen_height", "timerange_s")
    return SpectrogramBatch(scale=scales()[case.get("scale", "mel")], **{k: case[k] for k in keys if k in case})


def kernel(hip, norm, st, src, a, old_in):
    """frt_specgram_batch on host arrays: norm [S, F, B], src (local, -1 = filler) and a [P], old_in [S, H] -> (pixels [S, H, P], old_out)."""
    from friture_amd import _lib
    norm = np.ascontiguousarray(norm, np.float64)
    S, F, B = norm.shape
    Hh, P = st["height"], len(src)
    src, a = np.ascontiguousarray(src, np.int32), np.ascontiguousarray(a, np.float64)
    old_in = np.ascontiguousarray(old_in, np.float64)
    freq, targets = np.ascontiguousarray(st["freq"], np.float64), np.ascontiguousarray(st["targets"], np.float64)
    lut = np.ascontiguousarray(st["lut"], np.uint32)
    pixels, old_out = np.full((S, Hh, max(P, 1)), 0xdeadbeef, np.uint32), np.full((S, Hh), np.nan)
    _lib.check(hip.frt_specgram_batch(norm.ctypes.data, S, F, B, B, F * B, freq.ctypes.data, targets.ctypes.data, Hh,
                                      src.ctypes.data if P else None, a.ctypes.data if P else None, P, old_in.ctypes.data,
                                      old_out.ctypes.data, lut.ctypes.data, pixels.ctypes.data if P else None, 0, P))
    return pixels[:, :, :P], old_out


def check_kernel(hip, norm, frame_start, st, old_in):
    refs = [H.screen_replay(norm[s], frame_start, st, old=old_in[s]) for s in range(norm.shape[0])]
    src = np.where(refs[0]["filler"], -1, refs[0]["src"])
    pixels, old_out = kernel(hip, norm, st, src, refs[0]["a"], old_in)
    for s, ref in enumerate(refs):
        assert np.array_equal(pixels[s], ref["pixels"]), (s, int(np.sum(pixels[s] != ref["pixels"])))
        assert np.array_equal(old_out[s], ref["old_column"]), s
    return refs[0]


# ---- 1. the kernel on given frames ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(H.GOLDEN_CASES))
def test_kernel_on_the_recorded_frames_gives_the_recorded_pixels(hip, gold, name):
    case = H.GOLDEN_CASES[name]
    g = gold[name]
    st = H.settings(**case)
    pixels, _ = kernel(hip, g["norm"][None], st, np.where(g["filler"], -1, g["src"]), g["a"], np.zeros((1, st["height"])))
    assert np.array_equal(pixels[0], g["pixels"])
    check_kernel(hip, g["norm"][None], g["frame_start"], st, np.zeros((1, st["height"])))


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("height", [1, 48, 400, 1080])
@pytest.mark.parametrize("scale", ["linear", "log", "mel", "erb", "octave"])
@pytest.mark.parametrize("width", [125, 750])                       # 3 frames per column, half a frame per column
def test_kernel_equals_the_replay_on_random_frames(hip, S, height, scale, width):
    """Random frames reaching below 0 and above 1 (both clip branches), 75 frames (three tiles of the kernel, the last one short)
    in refreshes of 1..6 frames, a carried column that is not zero: with several columns per frame the slab's first column reads it."""
    st = H.settings(fft_size=256, overlap=Fraction(1, 2), scale=scale, minfreq=20., maxfreq=24000. if scale == "linear" else 20000.,
                    screen_width=width, screen_height=height, timerange_s=1.)
    rng = np.random.default_rng(1000 * S + height + width)
    F = 75
    norm = rng.uniform(-0.2, 1.2, (S, F, len(st["freq"])))
    steps = np.cumsum(rng.integers(1, 7, size=F))
    frame_start = np.concatenate([[0], steps[steps < F], [F]]).astype(np.int64)
    ref = check_kernel(hip, norm, frame_start, st, rng.uniform(-0.2, 1.2, (S, height)))
    assert ref["pixels"].shape[1] >= 15 and not ref["filler"].any()
    if width == 750:
        assert ref["src"][0] == 0 and ref["a"][0] != 0                # the first column mixes in old_in


def test_kernel_skips_unread_frames_and_carries_without_columns(hip):
    """NaN frames that no column reads leave no trace (24 frames per column: most are skipped); a slab without columns still
    leaves its last frame as the carried column."""
    st = H.settings(fft_size=256, overlap=Fraction(1, 2), screen_width=125, screen_height=48, timerange_s=8.)
    assert st["ratio"] == 24.
    rng = np.random.default_rng(5)
    F = 100
    norm = rng.uniform(0, 1, (2, F, len(st["freq"])))
    frame_start = np.arange(0, F + 1, 4)
    ref = H.screen_replay(norm[0], frame_start, st)
    used = np.unique(np.concatenate([ref["src"], ref["src"] - 1, [F - 1]]))
    poisoned = norm.copy()
    poisoned[:, np.setdiff1d(np.arange(F), used)] = np.nan
    assert np.isnan(poisoned).any()
    check_kernel(hip, norm, frame_start, st, np.zeros((2, 48)))
    pixels, old_out = kernel(hip, poisoned, st, ref["src"], ref["a"], np.zeros((2, 48)))
    assert np.array_equal(pixels[0], ref["pixels"]) and np.array_equal(old_out[0], ref["old_column"])
    _, carried = kernel(hip, norm[:, :7], st, [], [], np.zeros((2, 48)))
    assert np.array_equal(carried[0], H.screen_replay(norm[0, :7], np.array([0, 7]), st)["old_column"])


def test_kernel_argument_errors(hip):
    from friture_amd import _lib
    st = H.settings(fft_size=256, overlap=Fraction(1, 2), screen_height=8)
    norm = np.zeros((1, 4, len(st["freq"])))
    for src in ([4], [2, 1]):                                        # beyond the slab; not ascending
        with pytest.raises(_lib.FritureHipError, match="frt_specgram_batch"):
            kernel(hip, norm, st, src, [0.5] * len(src), np.zeros((1, 8)))


# ---- 2. end to end against the replay ---------------------------------------------------------------------------------------

E2E_CASES = {
    "defaults": dict(fft_size=4096, overlap=Fraction(3, 4), screen_width=800, screen_height=400, timerange_s=10., n=1 << 17, seed=21, chunk=512),
    "thirds": dict(H.GOLDEN_CASES["thirds_1000"], fft_size=1024, n=40000, seed=22),      # the device transform takes powers of two
    "up": dict(H.GOLDEN_CASES["up_512"], n=30000, seed=23, chunk=640),
}


@pytest.mark.parametrize("name", list(E2E_CASES))
def test_run_equals_the_replay_on_noise(hip, name):
    """Seeded noise: every bin lies far above the float64 transform's error floor.  A pixel may differ from the replay only where
    the replay's v * 255 lies within 1e-9 of an integer, and then by one LUT index; at most 1 pixel in 10^5 may be excused so.
    Counted on the CPU for these cases: no pixel of the replay has 0 < v * 255 < 255 within 1e-9 of an integer (`defaults` 87 200
    pixels, `thirds` 2 178, `up` 4 140).  The only pixels the rule names are those the clip sets to exactly 0 (802, 19 and 468: the
    all-zero first frame of a fresh widget and what it is mixed into; none clips at 255), which no last-bit difference of the
    frames moves; the replay alone therefore predicts no differing pixel at all."""
    case = E2E_CASES[name]
    st = H.settings(**case)
    x = synth("noise", case["n"], case["seed"])
    ends = chunk_ends(case["n"], case["chunk"])
    ref = H.replay(x, ends, st)
    res = batch_of(case).run(x, ends=ends)
    assert res.pixels.dtype == np.uint32 and res.pixels.shape == ref["pixels"].shape and ref["pixels"].size > 2000
    assert np.array_equal(res.column_refresh, ref["column_refresh"]) and np.array_equal(res.refresh_chunk, ref["refresh_chunk"])
    differs = res.pixels != ref["pixels"]
    edge = H.near_edge(ref["v255"])
    print(f"{name}: {ref['pixels'].size} pixels, {int(edge.sum())} near an edge, {int(differs.sum())} differ")
    assert not np.any(differs & ~edge)
    idx = ref["v255"].astype(np.intp)
    live = np.broadcast_to(~ref["filler"], differs.shape)
    assert not np.any(differs & ~live)
    one_off = (res.pixels == st["lut"][np.clip(idx - 1, 0, 255)]) | (res.pixels == st["lut"][np.clip(idx + 1, 0, 255)])
    assert np.all(one_off[differs])
    assert differs.sum() <= 1e-5 * differs.size
    assert np.array_equal(res.state.old_column.shape, (1, st["height"]))
    assert (res.state.orig_index, res.state.resampled_index) == (ref["orig_index"], ref["resampled_index"])
    np.testing.assert_allclose(res.state.old_column[0], ref["old_column"], rtol=0, atol=1e-12)


def test_silence_is_the_first_colour_everywhere(hip):
    from friture_amd.spectrogram import SpectrogramBatch
    sb = SpectrogramBatch(fft_size=1024, screen_height=48)
    res = sb.run(np.zeros((2, 30000), np.float32))
    assert res.pixels.shape[:2] == (2, 48) and res.pixels.shape[2] > 10 and np.all(res.pixels == sb.lut[0])


# ---- 3. equals the per-chunk object -----------------------------------------------------------------------------------------

def stream_pixels(x, chunk, **kw):
    from friture_amd.spectrogram import SpectrogramStream
    obj = SpectrogramStream(**kw)
    blocks = [obj.handle_new_data(x[None, a:a + chunk]) for a in range(0, len(x), chunk)]
    return np.concatenate([b for b in blocks if b is not None], axis=1)


@pytest.mark.parametrize("kind", ["tone", "chirp", "noise"])
@pytest.mark.parametrize("kw,T", [(dict(fft_size=1024, screen_height=48), 48000), (dict(), 1 << 16),
                                  (dict(fft_size=512, overlap=Fraction(1, 2), screen_width=1200, screen_height=33, timerange_s=2.), 20000)])
def test_run_equals_the_stream_object_fed_chunk_by_chunk(hip, kind, kw, T):
    from friture_amd.spectrogram import SpectrogramBatch
    x = synth(kind, T, 31)
    sb = SpectrogramBatch(**kw)
    assert not sb.columns(T).filler.any()                            # the stream object emits no filler columns
    res = sb.run(x, chunk=512)
    want = stream_pixels(x, 512, **kw)
    assert res.pixels.shape == want.shape and want.shape[1] > 30 and np.array_equal(res.pixels, want)


def test_streams_equal_as_many_stream_objects(hip):
    from friture_amd.spectrogram import SpectrogramBatch
    kw = dict(fft_size=1024, screen_height=48, weighting=1)
    x = np.stack([synth(kind, 40000, 40 + i) for i, kind in enumerate(["tone", "chirp", "noise", "noise", "tone"])])
    res = SpectrogramBatch(**kw).run(x, chunk=512)
    assert res.pixels.shape[0] == 5
    for s in range(5):
        assert np.array_equal(res.pixels[s], stream_pixels(x[s], 512, **kw)), s


# ---- 4. split, slab and keep invariance -------------------------------------------------------------------------------------

def test_split_slab_keep_and_tensor_input_give_the_same_bits(hip):
    import torch
    from friture_amd.spectrogram import SpectrogramBatch
    sb = SpectrogramBatch(fft_size=1024, screen_width=800, screen_height=100, timerange_s=2.)        # 0.47 frames per column
    T = 512 * 240
    x = np.stack([synth(kind, T, 50 + i) for i, kind in enumerate(["noise", "chirp", "tone"])])
    whole = sb.run(x)
    P = whole.pixels.shape[2]
    assert P > sb.screen_width and whole.pixels.shape == (3, 100, P) and len(whole.column_refresh) == P
    for cuts in ([512 * 37], [512, 512 * 239], [512 * 40, 512 * 41]):
        state, parts = None, []
        for a, b in zip([0] + cuts, cuts + [T]):
            r = sb.run(x[:, a:b], state=state)
            state = r.state
            parts.append(r.pixels)
        assert np.array_equal(np.concatenate(parts, axis=2), whole.pixels)
        assert np.array_equal(state.tail, whole.state.tail) and state.pending == whole.state.pending
        assert np.array_equal(state.old_column, whole.state.old_column)
        assert (state.orig_index, state.resampled_index) == (whole.state.orig_index, whole.state.resampled_index)
    one_refresh = 3 * sb.n_bins * 8
    for scratch in (one_refresh, 5 * one_refresh + 8, 40 * one_refresh, 1):
        r = sb.run(x, scratch_bytes=scratch)
        assert np.array_equal(r.pixels, whole.pixels) and np.array_equal(r.state.old_column, whole.state.old_column)
        k = sb.run(x, keep="screen", scratch_bytes=scratch)
        assert k.pixels.shape == (3, 100, sb.screen_width) and np.array_equal(k.pixels, whole.pixels[:, :, -sb.screen_width:])
        assert np.array_equal(k.column_refresh, whole.column_refresh[-sb.screen_width:])
        assert np.array_equal(k.state.old_column, whole.state.old_column) and np.array_equal(k.state.tail, whole.state.tail)
    short = sb.run(x[:, :512 * 20], keep="screen")                   # fewer columns than the screen is wide: all of them
    assert np.array_equal(short.pixels, sb.run(x[:, :512 * 20]).pixels) and short.pixels.shape[2] < sb.screen_width
    # ragged chunk ends and float64 input, a stream without its axis
    ends = np.array([100, 5000, 5001, 30000, T])
    r64 = sb.run(x.astype(np.float64), ends=ends)
    assert np.array_equal(r64.pixels, sb.run(x, ends=ends).pixels)
    single = sb.run(x[1])
    assert single.pixels.shape == (100, P) and np.array_equal(single.pixels, whole.pixels[1])
    # a CUDA tensor in, CUDA pixels out
    rt = sb.run(torch.from_numpy(x).cuda())
    assert rt.pixels.is_cuda and np.array_equal(rt.pixels.cpu().numpy().view(np.uint32), whole.pixels)
    assert np.array_equal(rt.state.old_column.cpu().numpy(), whole.state.old_column)
    rt2 = sb.run(torch.from_numpy(x[:, 512 * 37:]).cuda(), state=sb.run(torch.from_numpy(x[:, :512 * 37]).cuda()).state)
    assert np.array_equal(rt2.pixels.cpu().numpy().view(np.uint32), whole.pixels[:, :, P - rt2.pixels.shape[2]:])


def test_downsampling_route_with_screen_keep(hip):
    """The pixel rate below the STFT rate (4.7 frames per column): slabs and keep='screen' again, where most frames feed no column."""
    from friture_amd.spectrogram import SpectrogramBatch
    sb = SpectrogramBatch(fft_size=512, screen_width=40, screen_height=33, timerange_s=0.5)
    x = np.stack([synth("noise", 40000, 61), synth("chirp", 40000, 62)])
    whole = sb.run(x)
    assert whole.pixels.shape[2] > 40
    for scratch in (1, 1 << 16, 1 << 30):
        k = sb.run(x, keep="screen", scratch_bytes=scratch)
        assert np.array_equal(k.pixels, whole.pixels[:, :, -40:]) and np.array_equal(k.state.old_column, whole.state.old_column)
        assert np.array_equal(sb.run(x, scratch_bytes=scratch).pixels, whole.pixels)


# ---- 5. argument errors -------------------------------------------------------------------------------------------------------

def test_argument_errors_carry_a_message_and_leave_the_state_untouched(hip):
    from friture_amd.spectrogram import SpectrogramBatch
    sb = SpectrogramBatch(fft_size=1024, screen_height=48)
    x = synth("noise", 20000, 70)[None]
    state = sb.run(x).state
    kept = [np.array(state.tail, copy=True), np.array(state.old_column, copy=True)]
    with pytest.raises(ValueError, match="keep="):
        sb.run(x, keep="last", state=state)
    with pytest.raises(TypeError, match="float32 or float64"):
        sb.run(x.astype(np.int16), state=state)
    with pytest.raises(TypeError, match="numpy array or a CUDA tensor"):
        sb.run(x.tolist(), state=state)
    with pytest.raises(ValueError, match=r"expected \[S, T\]"):
        sb.run(x[None], state=state)
    with pytest.raises(ValueError, match="state of another shape"):
        sb.run(np.concatenate([x, x]), state=state)
    with pytest.raises(ValueError, match="ends must be sorted"):
        sb.run(x, ends=[300, 200], state=state)
    with pytest.raises(ValueError, match="chunk"):
        sb.run(x, chunk=0, state=state)
    c = H.OVER_EMISSION
    over = SpectrogramBatch(fft_size=c["fft_size"], overlap=c["overlap"], screen_width=c["screen_width"], screen_height=c["screen_height"],
                            timerange_s=c["timerange_s"])
    with pytest.raises(ValueError, match=f"refresh {c['refresh']}:"):
        over.run(synth("noise", c["n"], 71), chunk=c["chunk"])
    assert np.array_equal(state.tail, kept[0]) and np.array_equal(state.old_column, kept[1])
    again = sb.run(x, state=state)                                   # and a run with it does not modify it either
    assert np.array_equal(state.tail, kept[0]) and np.array_equal(state.old_column, kept[1]) and again.pixels.shape[2] > 0
