"""PitchBatch on the GPU against the numpy replay of the widget chain (oracle/pitchbatch.py, pinned to the reference's own
PitchTracker by tests/golden/pitchbatch.npz, which oracle/golden_pitchbatch.py records) and against PitchEngine.track.

Tolerances are those of tests/test_pitch_gpu.py: estimates and `pitch` 1e-9 relative, confidence 1e-11, level 1e-10 dB, the
voiced pattern identical; the raw estimate is not compared on `noise` (its arg-max sits among near-ties).  The curve is held to
1e-12 absolute of the numpy formula on the batch's own estimates (log2 rounding over a four-octave range) and to 1e-9 of the
replay's curve (the estimate tolerance over ln 2 * log2(max_freq / min_freq): about 3.6e-10).
"""
import functools

import numpy as np
import pytest

from oracle import pitchbatch as H
from friture_amd._batchio import chunk_ends

pytestmark = pytest.mark.gpu

CONFIGS = [(1024, 0.75), (2048, 0.5)]
NAMES = ["steady220", "jump", "noise"]                # S = 3
TOL_F0, TOL_CONF, TOL_DB = 1e-9, 1e-11, 1e-10
TOL_CURVE_FORMULA, TOL_CURVE_REPLAY = 1e-12, 1e-9
SHORT = 0.1                                            # seconds: M = 19 at step 256 ...
DURATIONS = {(1024, 0.75): 0.1, (2048, 0.5): 0.4}      # ... and at step 1024


@pytest.fixture(scope="module")
def pt(hip):
    from friture_amd import pitch_tracker
    return pitch_tracker


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(__file__.rsplit("/", 1)[0] + "/golden/pitch.npz", allow_pickle=False) as z:
        return {k: z[k] for k in z.files if k.endswith("_x")}


@functools.lru_cache(maxsize=None)
def mono(fft_size):
    """[3, T] float32: the recorded inputs of tests/golden/pitch.npz."""
    x = np.stack([_golden()[f"N{fft_size}_{n}_x"] for n in NAMES])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def dual(fft_size):
    """[3, 2, T] float64: the two inputs a row-0 level gets wrong, and a recorded input beside a seeded tone."""
    n = fft_size * 12
    d = H.dual_inputs(n)
    third = np.stack([_golden()[f"N{fft_size}_jump_x"].astype(np.float64), H.tone(n, 330.0, -30.0, 21)])
    x = np.stack([d[0], d[1], third])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def replays(fft_size, overlap, is_dual, duration, ends=None):
    """The replay of every stream, computed once per setting and shared."""
    x = (dual(fft_size) if is_dual else mono(fft_size)[:, None, :]).astype(np.float64)
    e = chunk_ends(x.shape[-1], 512) if ends is None else np.array(ends)
    return [H.replay(x[s], e, fft_size=fft_size, overlap=overlap, duration=duration) for s in range(x.shape[0])]


def host(a):
    return a if isinstance(a, np.ndarray) or a is None else a.cpu().numpy()


def check_against_replay(res, want, names=None):
    est, raw, pitch = host(res.estimates), host(res.raw), host(res.pitch)
    for s, w in enumerate(want):
        assert np.array_equal(res.frame_start, w["frame_start"]) and np.array_equal(res.refresh_chunk, w["refresh_chunk"])
        assert H.close(est[s], w["estimates"], TOL_F0), s
        assert H.close(pitch[s], w["pitch"], TOL_F0), s
        if raw is not None:
            if names is None or names[s] != "noise":
                assert H.close(raw[0, s], w["raw"][0], TOL_F0), s
            assert H.close(raw[1, s], w["raw"][1], TOL_CONF), s
            assert np.all(np.abs(raw[2, s] - w["raw"][2]) <= TOL_DB), s


@pytest.mark.parametrize("fft_size,overlap", CONFIGS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("on_device", [False, True])
def test_mono_equals_the_replay_and_the_engine(pt, fft_size, overlap, dtype, on_device):
    import torch
    x = mono(fft_size).astype(dtype)
    pb = pt.PitchBatch(fft_size, overlap)
    res = pb.run(torch.from_numpy(x).cuda() if on_device else x, with_raw=True)
    assert all(isinstance(v, np.ndarray) != on_device for v in (res.estimates, res.raw, res.pitch, res.curve, res.state.tail))
    assert isinstance(res.frame_start, np.ndarray) and isinstance(res.refresh_chunk, np.ndarray) and isinstance(res.times, np.ndarray)
    F, R = (x.shape[1] - fft_size) // pb.step + 1, len(res.refresh_chunk)
    assert res.estimates.shape == (3, F) and res.raw.shape == (3, 3, F) and res.pitch.shape == (3, R) and R > 1
    assert res.curve.shape == (3, pb.n_history) and np.array_equal(res.times, np.linspace(0, 1, pb.n_history))
    check_against_replay(res, replays(fft_size, overlap, False, 10), NAMES)
    eng = pt.PitchEngine(fft_size, pb.step, 3)
    assert np.array_equal(host(res.estimates), eng.track(x.astype(np.float64)), equal_nan=True)     # the same bits
    assert np.any(np.isnan(host(res.estimates)[1])) and not np.all(np.isnan(host(res.estimates)[1]))   # `jump` is gated somewhere


@pytest.mark.parametrize("fft_size,overlap", CONFIGS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dual_rows_pool_the_level_over_both_rows(pt, fft_size, overlap, dtype):
    """Stream 0: row 0 near -56 dBFS beside a row at -20 dBFS, voiced only by the pooled level; stream 1: row 0 near -48 dBFS
    beside silence, unvoiced only by it.  Both levels lie a decibel or more from min_db on opposite sides (checked on the CPU in
    tests/test_pitchbatch_cpu.py), so 1e-10 dB cannot flip a gate.  float32 rounds the samples first: the replay sees the same."""
    x = dual(fft_size).astype(dtype)
    pb = pt.PitchBatch(fft_size, overlap, dual_channels=True)
    res = pb.run(x, with_raw=True)
    want = [H.replay(x[s].astype(np.float64), chunk_ends(x.shape[-1], 512), fft_size=fft_size, overlap=overlap) for s in range(3)] \
        if dtype == np.float32 else replays(fft_size, overlap, True, 10)
    check_against_replay(res, want)
    assert not np.any(np.isnan(res.estimates[0])) and np.all(np.isnan(res.estimates[1]))
    row0 = pt.PitchBatch(fft_size, overlap).run(np.ascontiguousarray(x[:, 0]), with_raw=True)      # the level of row 0 alone
    assert np.all(np.isnan(row0.estimates[0])) and not np.any(np.isnan(row0.estimates[1]))
    assert np.array_equal(row0.raw[:2], res.raw[:2], equal_nan=True)                              # spectrum side: row 0 only
    import torch
    dev = pb.run(torch.from_numpy(x).cuda(), with_raw=True)
    assert np.array_equal(host(dev.estimates), res.estimates, equal_nan=True) and np.array_equal(host(dev.raw), res.raw, equal_nan=True)


@pytest.mark.parametrize("fft_size,overlap", CONFIGS)
@pytest.mark.parametrize("short", [True, False])
def test_curve(pt, fft_size, overlap, short):
    """M = 19 < F: the window slides; the default 10 s: M > F, the zeros before the first frame dominate."""
    duration = DURATIONS[(fft_size, overlap)] if short else 10
    x = mono(fft_size)
    pb = pt.PitchBatch(fft_size, overlap, duration=duration)
    M = pb.n_history
    every, last = pb.run(x, keep="all"), pb.run(x, keep="last")
    F, R = every.estimates.shape[1], len(every.refresh_chunk)
    assert (M == 19 and M < F) if short else (M in (469, 1876) and M > F)
    assert every.curve.shape == (3, R, M) and last.curve.shape == (3, M)
    assert not np.any(np.isnan(every.curve)) and np.all((every.curve >= 0) & (every.curve <= 1))
    assert np.array_equal(last.curve, every.curve[:, -1]) and np.array_equal(last.estimates, every.estimates, equal_nan=True)
    want = replays(fft_size, overlap, False, duration)
    for s in range(3):
        padded = np.concatenate([np.zeros(M), every.estimates[s]])
        for r in range(R):
            window = padded[every.frame_start[r + 1]:every.frame_start[r + 1] + M]
            assert np.max(np.abs(every.curve[s, r] - H.axis_curve(window))) <= TOL_CURVE_FORMULA, (s, r)
            assert np.array_equal(every.curve[s, r] == 1.0, ~(window > 65.0)), (s, r)       # NaN and 0 sit at 1
        assert every.curve[s].shape == want[s]["curves"].shape
        assert np.max(np.abs(every.curve[s] - want[s]["curves"])) <= TOL_CURVE_REPLAY, s
        assert np.max(np.abs(last.curve[s] - want[s]["last_curve"])) <= TOL_CURVE_REPLAY, s
        assert np.array_equal(every.state.history[s], padded[-M:], equal_nan=True)
    assert np.any(every.curve < 1.0)


def joined(first, second, n_chunks_first):
    """The fields of two consecutive runs as one run would give them (curve: keep="all")."""
    cat = lambda a, b, axis: np.concatenate([a, b], axis=axis)
    return {"estimates": cat(first.estimates, second.estimates, -1), "raw": cat(first.raw, second.raw, -1),
            "frame_start": cat(first.frame_start, second.frame_start[1:] + first.frame_start[-1], 0),
            "refresh_chunk": cat(first.refresh_chunk, second.refresh_chunk + n_chunks_first, 0),
            "pitch": cat(first.pitch, second.pitch, -1), "curve": cat(first.curve, second.curve, -2)}


def assert_same_state(a, b):
    assert a.pending == b.pending
    for name in ("tail", "previous", "history"):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name


@pytest.mark.parametrize("fft_size,overlap", CONFIGS)
@pytest.mark.parametrize("is_dual", [False, True])
def test_a_recording_in_two_pieces_equals_the_recording(pt, fft_size, overlap, is_dual):
    x = dual(fft_size) if is_dual else mono(fft_size)
    T = x.shape[-1]
    pb = pt.PitchBatch(fft_size, overlap, duration=DURATIONS[(fft_size, overlap)], dual_channels=is_dual)
    # a chunk boundary, a sample that is neither a chunk nor a step multiple, and a first piece without a frame
    for a, base in ((512 * 17, chunk_ends(T, 512)), (5001, chunk_ends(T, 512)), (fft_size - 325, chunk_ends(T, 512)),
                    (5001, H.ragged(T, 7)), (512 * 17, H.ragged(T, 8))):
        ends = np.unique(np.concatenate([base, [a]]))
        e1, e2 = ends[ends <= a], ends[ends > a] - a
        whole = pb.run(x, ends=ends, keep="all", with_raw=True)
        first = pb.run(x[..., :a], ends=e1, keep="all", with_raw=True)
        second = pb.run(x[..., a:], ends=e2, state=first.state, keep="all", with_raw=True)
        assert first.state.pending == a - first.estimates.shape[-1] * pb.step and first.state.tail.dtype == np.float64
        for name, value in joined(first, second, len(e1)).items():
            assert np.array_equal(value, getattr(whole, name), equal_nan=True), (a, name)
        assert_same_state(second.state, whole.state)
        last = pb.run(x[..., a:], ends=e2, state=first.state, keep="last")
        assert np.array_equal(last.curve, whole.curve[:, -1])
    # the default chunking cut at a chunk boundary needs no ends
    a = 512 * 17
    whole, first = pb.run(x, keep="all", with_raw=True), pb.run(x[..., :a], keep="all", with_raw=True)
    second = pb.run(x[..., a:], state=first.state, keep="all", with_raw=True)
    for name, value in joined(first, second, 17).items():
        assert np.array_equal(value, getattr(whole, name), equal_nan=True), name
    assert_same_state(second.state, whole.state)


def test_four_scratch_slabs_give_the_same_bits(pt):
    """16392 bytes of scratch per frame at N = 1024 and slabs of whole 32-frame blocks per stream: 120 frames of 3 streams
    under 32 * 16392 * 3 bytes go through as 32 + 32 + 32 + 24."""
    g = _golden()
    order = [("steady220", "jump", "glide"), ("glide", "steady220", "jump"), ("jump", "high900", "quiet")]
    T = 1024 + 256 * 119
    x = np.stack([np.concatenate([g[f"N1024_{n}_x"] for n in names])[:T] for names in order])
    x2 = np.stack([x, x[::-1]], axis=1)
    for pb, data in ((pt.PitchBatch(1024, 0.75, duration=SHORT), x), (pt.PitchBatch(1024, 0.75, duration=SHORT, dual_channels=True), x2)):
        whole = pb.run(data, keep="all", with_raw=True)
        slabs = pb.run(data, keep="all", with_raw=True, scratch_bytes=32 * 16392 * 3)
        assert whole.estimates.shape == (3, 120) and np.any(~np.isnan(whole.estimates))
        for name in ("estimates", "raw", "pitch", "curve", "frame_start", "refresh_chunk"):
            assert np.array_equal(getattr(slabs, name), getattr(whole, name), equal_nan=True), name
        assert_same_state(slabs.state, whole.state)
        first = pb.run(data[..., :512 * 17], with_raw=True, scratch_bytes=32 * 16392 * 3)
        second = pb.run(data[..., 512 * 17:], state=first.state, keep="all", with_raw=True, scratch_bytes=32 * 16392 * 3)
        assert np.array_equal(np.concatenate([first.estimates, second.estimates], -1), whole.estimates, equal_nan=True)
        assert_same_state(second.state, whole.state)


def test_a_hop_that_does_not_divide_the_frame(pt):
    """overlap 0.3: step 716 — the level comes from one wavefront per frame instead of the shared hop blocks."""
    x = dual(1024)
    pb = pt.PitchBatch(1024, 0.3, dual_channels=True)
    assert pb.step == 716 and 1024 % pb.step
    res = pb.run(x, with_raw=True)
    want = [H.replay(x[s], chunk_ends(x.shape[-1], 512), fft_size=1024, overlap=0.3) for s in range(3)]
    check_against_replay(res, want)
    first = pb.run(x[..., :5001].astype(np.float32))
    second = pb.run(x[..., 5001:].astype(np.float32), state=first.state)
    both = pb.run(x.astype(np.float32))
    assert np.array_equal(np.concatenate([first.estimates, second.estimates], -1), both.estimates, equal_nan=True)


def test_small_things(pt):
    import torch
    x = mono(1024).astype(np.float64)
    pb = pt.PitchBatch(1024, 0.75, duration=SHORT)
    whole = pb.run(x, keep="all", with_raw=True)
    # a stream without its axis
    one = pb.run(x[1], keep="all", with_raw=True)
    assert one.estimates.shape == whole.estimates.shape[1:] and one.raw.shape == (3,) + whole.raw.shape[2:]
    assert np.array_equal(one.estimates, whole.estimates[1], equal_nan=True) and np.array_equal(one.curve, whole.curve[1])
    assert np.array_equal(one.pitch, whole.pitch[1], equal_nan=True) and np.array_equal(one.raw, whole.raw[:, 1], equal_nan=True)
    # a strided CUDA tensor on a stream of its own
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big = torch.zeros((6, x.shape[1] + 5), dtype=torch.float64, device="cuda")
        big[::2, 3:-2] = torch.from_numpy(x).cuda()
        view = big[::2, 3:-2]
        assert not view.is_contiguous()
        got = pb.run(view, keep="all", with_raw=True)
        late = got.estimates.clone()                              # the caller's stream may use the results at once
    side.synchronize()
    assert got.estimates.is_cuda and np.array_equal(late.cpu().numpy(), whole.estimates, equal_nan=True)
    assert np.array_equal(got.curve.cpu().numpy(), whole.curve) and np.array_equal(got.raw.cpu().numpy(), whole.raw, equal_nan=True)
    # shorter than a frame: nothing to show yet, and a state that a later call completes
    none = pb.run(x[:, :700], keep="all", with_raw=True)
    assert none.estimates.shape == (3, 0) and none.raw.shape == (3, 3, 0) and none.pitch.shape == (3, 0) and none.curve.shape == (3, 0, 19)
    assert none.frame_start.tolist() == [0] and none.refresh_chunk.size == 0
    assert none.state.pending == 700 and np.array_equal(none.state.tail, x[:, None, :700]) and np.all(np.isnan(none.state.previous))
    assert np.array_equal(none.state.history, np.zeros((3, 19)))
    assert np.array_equal(pb.run(x[:, :700]).curve, np.ones((3, 19)))            # the widget's first curve: the ring's zeros
    rest = pb.run(x[:, 700:], state=none.state)
    assert np.array_equal(rest.estimates, whole.estimates, equal_nan=True) and np.array_equal(rest.curve, whole.curve[:, -1])
    # what run refuses
    for bad, err in ((np.zeros((3, 2, 4096)), ValueError), (np.zeros((3, 4096), np.int16), TypeError), ([0.0] * 4096, TypeError),
                     (torch.zeros(4096), TypeError)):
        with pytest.raises(err):
            pb.run(bad)
    with pytest.raises(ValueError):
        pb.run(x, keep="first")
    with pytest.raises(ValueError):
        pt.PitchBatch(1024, 0.75, duration=SHORT, dual_channels=True).run(np.zeros((3, 3, 4096)))
    with pytest.raises(ValueError):
        pt.PitchBatch(1024, 0.75, duration=SHORT, dual_channels=True).run(x, state=whole.state)       # one row carried into two
    with pytest.raises(ValueError):
        pt.PitchBatch(1024, 0.75).run(x, state=whole.state)                                            # another history length
    with pytest.raises(ValueError):
        pb.run(x[:2], state=whole.state)                                                               # another number of streams
