"""PitchTrackerStream on the GPU: a RingBuffer fed in chunks, update() after every push, against the numpy replay of the widget
chain (oracle/pitchbatch.py), against PitchBatch on the same samples and chunk ends bit for bit, and against PitchTracker.

Inputs: the recorded inputs of tests/golden/pitch.npz (steady220, jump, noise at N = 1024 / overlap 0.75 and N = 2048 / 0.5,
12 N samples each) and oracle.pitchbatch's dual_inputs, ragged and tone.  Tolerances are those of tests/test_pitchbatch_gpu.py:
estimates and `pitch` 1e-9 relative with the voiced pattern identical, the curve 1e-12 absolute of the numpy formula on the
stream's own estimates and 1e-9 of the replay's curve; the raw estimate of `noise` is not compared (its arg-max sits among
near-ties), its gated estimates are (all unvoiced or equal).
"""
import functools
import math

import numpy as np
import pytest

from oracle import pitchbatch as H
from friture_amd._batchio import chunk_ends
from friture_amd.ringbuffer import RingBuffer

pytestmark = pytest.mark.gpu

CONFIGS = [(1024, 0.75), (2048, 0.5)]
NAMES = ["steady220", "jump", "noise"]
TOL_F0 = 1e-9
TOL_CURVE_FORMULA, TOL_CURVE_REPLAY = 1e-12, 1e-9
DURATIONS = {(1024, 0.75): 0.1, (2048, 0.5): 0.4}      # M = 19: the window slides within 12 N samples
CROSSOVER = 16                                         # frames per update up to which the few-frames product kernel runs


@pytest.fixture(scope="module")
def pt(hip):
    from friture_amd import pitch_tracker
    return pitch_tracker


@functools.lru_cache(maxsize=None)
def golden(key):
    with np.load(__file__.rsplit("/", 1)[0] + "/golden/pitch.npz", allow_pickle=False) as z:
        x = z[key]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def dual(fft_size):
    """[3, 2, T] float64: the two inputs a row-0 level gets wrong, and a recorded input beside a seeded tone."""
    n = fft_size * 12
    d = H.dual_inputs(n)
    x = np.stack([d[0], d[1], np.stack([golden(f"N{fft_size}_jump_x").astype(np.float64), H.tone(n, 330.0, -30.0, 21)])])
    x.setflags(write=False)
    return x


def feed(tracker_class, x, ends, fft_size, overlap, before_chunk=None, state=None, **settings):
    """x [T] or [rows, T] through a RingBuffer as the chunks that end at `ends`, update() after every push.  Returns the tracker
    and what each call left: estimates [F], frames per refresh, refresh_chunk, pitch [R], curves [R, M]."""
    x = np.atleast_2d(x)
    ring = RingBuffer()
    ring.grow_if_needed(x.shape[1] + fft_size)         # the true samples, however long an update stalls (ringbuffer.py:34)
    ring.push(x[:, :0])
    trk = tracker_class(ring, fft_size, overlap, **settings)
    if state is not None:
        trk.set_state(state)
    est, counts, chunks, pitch, curves = [], [], [], [], []
    start = 0
    for c, e in enumerate(np.asarray(ends).tolist()):
        if before_chunk is not None:
            before_chunk(trk, c)
        ring.push(x[:, start:e])
        start = e
        had, curve = trk.out_offset, getattr(trk, "curve", None)
        fresh = trk.update()
        n = trk.out_offset - had
        assert fresh is (n > 0)
        if not fresh:
            assert getattr(trk, "curve", None) is curve                  # no refresh: nothing moves
            continue
        est += trk.out_buf.data_indexed(trk.out_offset, n)[0].tolist()
        counts.append(n)
        chunks.append(c)
        assert np.array_equal(trk.get_latest_estimate(), est[-1], equal_nan=True)
        if hasattr(trk, "curve"):
            assert np.array_equal(trk.pitch, est[-1], equal_nan=True)
            pitch.append(trk.pitch)
            curves.append(trk.curve.copy())
    M = getattr(trk, "n_history", 0)
    return trk, {"estimates": np.array(est), "counts": counts, "refresh_chunk": np.array(chunks, np.int64),
                 "pitch": np.array(pitch), "curve": np.array(curves).reshape(len(curves), M)}


def assert_bits_of_the_batch(got, res):
    """res: PitchBatch.run(..., keep="all") of ONE stream on the same samples and ends."""
    assert np.array_equal(np.diff(res.frame_start), got["counts"]) and np.array_equal(res.refresh_chunk, got["refresh_chunk"])
    for name in ("estimates", "pitch", "curve"):
        assert got[name].shape == getattr(res, name).shape, name
        assert np.array_equal(got[name], getattr(res, name), equal_nan=True), name


def assert_close_to_replay(got, want):
    assert np.array_equal(np.diff(want["frame_start"]), got["counts"]) and np.array_equal(want["refresh_chunk"], got["refresh_chunk"])
    assert H.close(got["estimates"], want["estimates"], TOL_F0)
    assert H.close(got["pitch"], want["pitch"], TOL_F0)
    assert got["curve"].shape == want["curves"].shape
    assert np.max(np.abs(got["curve"] - want["curves"])) <= TOL_CURVE_REPLAY
    M = got["curve"].shape[1]
    padded, done = np.concatenate([np.zeros(M), got["estimates"]]), np.cumsum(got["counts"])
    for r in range(len(done)):                                            # the numpy formula on the stream's own estimates
        assert np.max(np.abs(got["curve"][r] - H.axis_curve(padded[done[r]:done[r] + M]))) <= TOL_CURVE_FORMULA, r


@pytest.mark.parametrize("fft_size,overlap", CONFIGS)
@pytest.mark.parametrize("name", NAMES)
def test_mono_chunks_of_512(pt, fft_size, overlap, name):
    x = golden(f"N{fft_size}_{name}_x")
    ends, duration = chunk_ends(x.size, 512), DURATIONS[(fft_size, overlap)]
    trk, got = feed(pt.PitchTrackerStream, x, ends, fft_size, overlap, duration=duration)
    assert trk.n_history == 19 and max(got["counts"]) <= 2 and len(got["counts"]) > 19
    assert_close_to_replay(got, H.replay(x.astype(np.float64), ends, fft_size=fft_size, overlap=overlap, duration=duration))
    assert_bits_of_the_batch(got, pt.PitchBatch(fft_size, overlap, duration=duration).run(x, keep="all"))
    voiced = ~np.isnan(got["estimates"])
    assert voiced.all() if name == "steady220" else voiced.any() and not voiced.all() if name == "jump" else True
    assert np.array_equal(trk.get_estimates(duration)[-5:], got["estimates"][-5:], equal_nan=True)


@pytest.mark.parametrize("fft_size,overlap", CONFIGS)
def test_two_rows_pool_the_level(pt, fft_size, overlap):
    """dual_inputs: stream 0 is voiced and stream 1 unvoiced only because the gate's level is the RMS over both rows."""
    x = dual(fft_size)
    ends = chunk_ends(x.shape[-1], 512)
    res = pt.PitchBatch(fft_size, overlap, dual_channels=True).run(x, keep="all")
    for s in range(3):
        trk, got = feed(pt.PitchTrackerStream, x[s], ends, fft_size, overlap)
        one = type(res)(*(v[s] if name in ("estimates", "pitch", "curve") else v for name, v in zip(res._fields, res)))
        assert_bits_of_the_batch(got, one)
        _, host_gate = feed(pt.PitchTracker, x[s], ends, fft_size, overlap)       # the gate as a host loop over frames
        assert np.array_equal(np.isnan(got["estimates"]), np.isnan(host_gate["estimates"]))
        assert H.close(got["estimates"], host_gate["estimates"], TOL_F0)
        if s < 2:
            assert np.isnan(got["estimates"]).all() == (s == 1) and np.isnan(got["estimates"]).any() == (s == 1)
            _, row0 = feed(pt.PitchTrackerStream, x[s, 0], ends, fft_size, overlap)      # the level of row 0 alone says otherwise
            assert np.isnan(row0["estimates"]).all() == (s == 0) and np.isnan(row0["estimates"]).any() == (s == 0)
    want = H.replay(x[2], ends, fft_size=fft_size, overlap=overlap)
    assert_close_to_replay(got, want)


def stalled(T, seed, fft_size, step, frames):
    """ragged(T, seed) with every chunk given twice (an empty chunk after each), a run of chunks shorter than a step, and
    one stall that completes at least `frames` frames in one update."""
    ends = H.ragged(T, seed)
    lo = ends[1]
    hi = lo + fft_size + frames * step
    assert hi < T
    short = np.arange(lo - 5 * (step // 3), lo, step // 3)
    ends = np.concatenate([ends[(ends <= lo - 5 * (step // 3)) | (ends >= hi)], short])
    return np.sort(np.repeat(ends, 2))


@pytest.mark.parametrize("is_dual", [False, True])
def test_ragged_chunks_and_a_stall(pt, is_dual):
    fft_size, overlap, duration = 1024, 0.75, 0.1
    x = dual(fft_size)[2] if is_dual else golden("N1024_jump_x")
    ends = stalled(x.shape[-1], 7, fft_size, 256, CROSSOVER + 3)
    assert np.any(np.diff(ends) == 0) and np.any((np.diff(ends) > 0) & (np.diff(ends) < 256))
    trk, got = feed(pt.PitchTrackerStream, x, ends, fft_size, overlap, duration=duration)
    assert trk.crossover == CROSSOVER and max(got["counts"]) > CROSSOVER and min(got["counts"]) == 1
    assert len(got["counts"]) < len(ends) // 2                     # chunks that complete no frame: update() False, curve unchanged
    assert_bits_of_the_batch(got, pt.PitchBatch(fft_size, overlap, duration=duration, dual_channels=is_dual).run(x, ends=ends, keep="all"))
    assert_close_to_replay(got, H.replay(np.asarray(x, np.float64), ends, fft_size=fft_size, overlap=overlap, duration=duration))


def test_both_sides_of_the_crossover_give_the_same_bits(pt):
    """The same recording fed so that every update completes 1, crossover, crossover + 1 and 40 frames: the few-frames kernel on
    one side, the tiled kernel of PitchEngine on the other; and with the threshold moved."""
    fft_size, overlap, step = 1024, 0.75, 256
    x = golden("N1024_jump_x")
    T = x.size
    whole = pt.PitchBatch(fft_size, overlap, duration=0.1).run(x, ends=[T], keep="last")
    F = whole.estimates.size

    def every(k):
        return np.append(fft_size + step * (np.arange(k, F, k) - 1), T)

    runs = {}
    for k, crossover in ((1, None), (CROSSOVER, None), (CROSSOVER + 1, None), (40, None), (5, 4), (5, 5), (40, 64), (1, 0)):
        def move(trk, c):
            if crossover is not None and c == 0:
                trk.crossover = crossover
        trk, got = feed(pt.PitchTrackerStream, x, every(k), fft_size, overlap, before_chunk=move, duration=0.1)
        assert trk.crossover == (CROSSOVER if crossover is None else crossover)
        assert got["counts"][0] == k and set(got["counts"][:-1]) == {k} and sum(got["counts"]) == F
        runs[(k, crossover)] = got
        assert np.array_equal(got["estimates"], whole.estimates, equal_nan=True), (k, crossover)
        assert np.array_equal(got["curve"][-1], whole.curve), (k, crossover)
    assert np.any(~np.isnan(whole.estimates)) and np.any(np.isnan(whole.estimates))
    assert np.array_equal(runs[(5, 4)]["curve"], runs[(5, 5)]["curve"])


@pytest.mark.parametrize("overlap,step", [(0.7, 307), (0.3, 716)])
@pytest.mark.parametrize("is_dual", [False, True])
def test_awkward_steps(pt, overlap, step, is_dual):
    """An odd step, and a step that does not divide the frame: the level is one sum per frame, not per shared block."""
    x = dual(1024)[2] if is_dual else golden("N1024_jump_x")
    for ends in (chunk_ends(x.shape[-1], 512), H.ragged(x.shape[-1], 9)):
        trk, got = feed(pt.PitchTrackerStream, x, ends, 1024, overlap, duration=0.2)
        assert trk.step == step and 1024 % step
        assert_bits_of_the_batch(got, pt.PitchBatch(1024, overlap, duration=0.2, dual_channels=is_dual).run(x, ends=ends, keep="all"))
    assert_close_to_replay(got, H.replay(np.asarray(x, np.float64), ends, fft_size=1024, overlap=overlap, duration=0.2))


def test_thresholds_changed_between_chunks_act_from_the_next_frame(pt):
    x = golden("N1024_steady220_x")
    ends = chunk_ends(x.size, 512)

    def change(trk, c):
        if c == 8:
            trk.min_db = 0.0                   # nothing is that loud
        if c == 14:
            trk.min_db, trk.conf = -50.0, 0.999            # loud enough again, never that sure
        if c == 19:
            trk.conf = 0.5

    _, got = feed(pt.PitchTrackerStream, x, ends, 1024, 0.75, before_chunk=change)
    _, want = feed(pt.PitchTracker, x, ends, 1024, 0.75, before_chunk=change)
    assert got["counts"] == want["counts"] and np.array_equal(got["refresh_chunk"], want["refresh_chunk"])
    assert H.close(got["estimates"], want["estimates"], TOL_F0)
    done = dict(zip(got["refresh_chunk"].tolist(), np.cumsum(got["counts"]).tolist()))       # frames complete after a chunk
    voiced = ~np.isnan(got["estimates"])
    assert voiced[:done[7]].all() and not voiced[done[7]:done[18]].any() and voiced[done[18]:].all()
    _, plain = feed(pt.PitchTrackerStream, x, ends, 1024, 0.75)
    assert np.array_equal(plain["estimates"][voiced], got["estimates"][voiced])


@pytest.mark.parametrize("fft_size,overlap,is_dual", [(2048, 0.5, False), (1024, 0.75, True)])
def test_state_hand_over_between_batch_and_stream(pt, fft_size, overlap, is_dual):
    x = dual(fft_size)[2] if is_dual else golden(f"N{fft_size}_jump_x")
    T, a, duration = x.shape[-1], 5001, DURATIONS[(fft_size, overlap)]
    pb = pt.PitchBatch(fft_size, overlap, duration=duration, dual_channels=is_dual)
    ends = np.unique(np.append(chunk_ends(T, 512), a))
    e1, e2 = ends[ends <= a], ends[ends > a] - a
    whole = pb.run(x, ends=ends, keep="all")
    first = pb.run(x[..., :a], ends=e1, keep="all")
    F1, R1 = first.estimates.shape[-1], len(first.refresh_chunk)
    assert first.state.pending % 2 == 1 and 0 < F1 < whole.estimates.size
    # the batch on the first piece, the stream on the rest
    trk, got = feed(pt.PitchTrackerStream, x[..., a:], e2, fft_size, overlap, state=first.state, duration=duration)
    assert np.array_equal(got["estimates"], whole.estimates[F1:], equal_nan=True)
    assert np.array_equal(got["pitch"], whole.pitch[R1:], equal_nan=True) and np.array_equal(got["curve"], whole.curve[R1:])
    last = trk.get_state()
    assert last.pending == whole.state.pending
    for field in ("tail", "previous", "history"):
        assert np.array_equal(getattr(last, field), getattr(whole.state, field), equal_nan=True), field
    # the stream on the first piece, the batch on the rest
    trk, got = feed(pt.PitchTrackerStream, x[..., :a], e1, fft_size, overlap, duration=duration)
    assert np.array_equal(got["estimates"], first.estimates, equal_nan=True)
    handed = trk.get_state()
    for field in ("tail", "previous", "history"):
        assert np.array_equal(getattr(handed, field), getattr(first.state, field), equal_nan=True), field
    second = pb.run(x[..., a:], ends=e2, state=handed, keep="all")
    assert np.array_equal(second.estimates, whole.estimates[F1:], equal_nan=True)
    assert np.array_equal(second.pitch, whole.pitch[R1:], equal_nan=True) and np.array_equal(second.curve, whole.curve[R1:])
    # and from stream to stream
    _, rest = feed(pt.PitchTrackerStream, x[..., a:], e2, fft_size, overlap, state=handed, duration=duration)
    assert np.array_equal(rest["estimates"], whole.estimates[F1:], equal_nan=True) and np.array_equal(rest["curve"], whole.curve[R1:])


def test_the_defaults(pt):
    """N = 4096, overlap 0.75, 10 s: M = 469, one frame every second chunk."""
    x = golden("N4096_jump_x")
    ends = chunk_ends(x.size, 512)
    trk, got = feed(pt.PitchTrackerStream, x, ends, 4096, 0.75)
    assert trk.n_history == 469 and trk.times.shape == (469,) and set(got["counts"]) == {1} and len(got["counts"]) == 45
    assert_bits_of_the_batch(got, pt.PitchBatch().run(x, keep="all"))
    assert_close_to_replay(got, H.replay(x.astype(np.float64), ends))
    assert np.any(got["curve"][-1] < 1.0) and np.all(got["curve"][:, :469 - 45] == 1.0)


def test_estimate_pitch_and_what_the_stream_refuses(pt):
    import ctypes
    from friture_amd import _lib
    x = golden("N1024_steady220_x").astype(np.float64)
    trk, got = feed(pt.PitchTrackerStream, x[:4096], chunk_ends(4096, 512), 1024, 0.75, duration=0.1)
    state, curve = trk.get_state(), trk.curve
    f0 = trk.estimate_pitch(x[None, 4096:5120])                    # moves the gate's previous estimate, nothing else
    assert abs(f0 - 220.0) < 1.0 and trk.prev_f0 == f0 and trk.curve is curve
    assert np.array_equal(trk.get_state().history, state.history, equal_nan=True)
    with pytest.raises(ValueError):
        trk.estimate_pitch(x[None, :1000])
    with pytest.raises(ValueError):                                # a span of another frame size
        trk._push(x[None, :1024 + 100])
    est, curve, latest = np.empty(4), np.empty(19), ctypes.c_double()
    lib = _lib.load()
    args = (x.ctypes.data, 1, 1, 1024 + 100, 1024 + 100, -50.0, 0.5, 2.0, est.ctypes.data, ctypes.byref(latest), curve.ctypes.data, None)
    with pytest.raises(_lib.FritureHipError, match="span"):
        _lib.check(lib.frt_pitch_live_push(trk._live, *args))
    with pytest.raises(_lib.FritureHipError, match="rows"):
        _lib.check(lib.frt_pitch_live_push(trk._live, x.ctypes.data, 1, 3, 1024, 1024, *args[5:]))
    with pytest.raises(ValueError):                                # three rows in the ring
        feed(pt.PitchTrackerStream, np.zeros((3, 2048)), [2048], 1024, 0.75)
    M = trk.n_history
    for bad in (state._replace(history=np.zeros((1, M + 1))), state._replace(tail=np.zeros((1, 2, state.pending + 1))),
                state._replace(previous=np.zeros(3)), state._replace(pending=1024, tail=np.zeros((1, 1, 1024)))):
        with pytest.raises(ValueError):
            trk.set_state(bad)
    with pytest.raises(_lib.FritureHipError, match="channels"):   # the C object wants a one-channel plan
        eng = pt.PitchEngine(1024, 256, 2)
        h = ctypes.c_void_p()
        _lib.check(lib.frt_pitch_live_create(ctypes.byref(h), eng._h, 19, 65.0, 1047.0))
    trk.set_state(state)                                           # and the good one still goes in
    assert math.isclose(trk.prev_f0, state.previous[0])
