"""SpectrumBatch on the GPU: frt_spectrum_batch alone on given PSD frames, the whole chain from samples against the oracle
replay and against the per-chunk SpectrumAnalyzerStream, split and slab invariance bit for bit, the hand-over to CurveBatch,
silence, argument errors.  Tolerances are those of tests/test_widgets_gpu.py for the same stages (smoothed 1e-13 relative, dB
1e-9 on given PSD frames and 1e-8 from samples); index equality is asserted only where oracle.spectrumbatch.assert_decisive
holds on the oracle's own values."""
import ctypes

import numpy as np
import pytest

from oracle import plotcurves as PH
from oracle import spectrumbatch as H
from conftest import rel_max
from oracle import dsp

pytestmark = pytest.mark.gpu

I64P = ctypes.POINTER(ctypes.c_int64)


def _kernel_call(hip, psd, frame_start, kern, alpha, weight, state, keep_last=False):
    """frt_spectrum_batch on host arrays: psd [S, rows, F, B] float32 / float64.  Returns (db, peak, pitch, state)."""
    from friture_amd import _lib
    S, rows, F, B = psd.shape
    psd = np.ascontiguousarray(psd)
    fs = np.ascontiguousarray(frame_start, np.int64)
    R = len(fs) - 1
    Ro = 1 if keep_last else R
    st = np.array(state, np.float64, copy=True)
    db, pk, pt = np.empty((S, Ro, B)), np.empty((S, Ro), np.int32), np.empty((S, Ro), np.int32)
    w = None if weight is None else np.ascontiguousarray(weight, np.float64)
    _lib.check(hip.frt_spectrum_batch(psd.ctypes.data, int(psd.dtype == np.float64), S, rows, F, B, B, F * B, fs.ctypes.data_as(I64P),
                                      R, kern.ctypes.data, len(kern), alpha, None if w is None else w.ctypes.data, st.ctypes.data,
                                      int(keep_last), db.ctypes.data, 0, pk.ctypes.data, pt.ctypes.data))
    return db, pk, pt, st


def _compare_kernel(got, ref, last_only=False):
    db, pk, pt, st = got
    H.assert_decisive(ref)
    sl = slice(-1, None) if last_only else slice(None)
    print("smoothed rel_max", rel_max(st, ref["state"]), "dB max", float(np.max(np.abs(db - ref["db"][:, sl]))))
    assert rel_max(st, ref["state"]) < 1e-13
    assert np.max(np.abs(db - ref["db"][:, sl])) < 1e-9
    assert np.array_equal(pk, ref["peak_index"][:, sl]) and np.array_equal(pt, ref["pitch_index"][:, sl])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("weighting", [0, 1])
def test_kernel_on_given_psd_frames(hip, dtype, rows, weighting):
    """Refreshes of 1, 3 and 64 frames, mixed, three streams, a bin count that fills neither a wavefront nor a workgroup."""
    B, S = 333, 3
    rng = np.random.default_rng(7 + rows + 2 * weighting)
    counts = [1, 3, 64, 1, 1, 3, 64, 3, 1]
    fs = np.concatenate([[0], np.cumsum(counts)])
    psd = (rng.random((S, rows, fs[-1], B)) ** 4 * 1e-3 + 1e-12).astype(dtype)
    _, _, alpha, kern, weight, freq = H.settings(2 * (B - 1), 0.75, weighting, 0.025)
    prev = rng.random((S, rows, B)) * 1e-4
    ref = H.readout_loop(psd, fs, kern, alpha, prev, weight, freq)
    _compare_kernel(_kernel_call(hip, psd, fs, kern, alpha, None if rows == 2 else weight, prev), ref)
    _compare_kernel(_kernel_call(hip, psd, fs, kern, alpha, None if rows == 2 else weight, prev, keep_last=True), ref, last_only=True)


def test_kernel_refresh_longer_than_the_smoothing_kernel(hip):
    """n > nk = 8192 frames in one refresh: data[:, :nk], the refresh's first nk frames, count and the previous value is forgotten
    (exp_smoothing.py:94-105, as dsp.exp_smoothed_value_2d and frt_spectrum_post have it)."""
    B = 12
    rng = np.random.default_rng(11)
    fs = np.array([0, 2, 2 + 8200, 2 + 8200 + 5])
    psd = rng.random((2, 1, fs[-1], B)) + 1e-6
    _, _, alpha, kern, weight, freq = H.settings(2 * (B - 1), 0.75, 1, 0.025)
    prev = rng.random((2, 1, B))
    ref = H.readout_loop(psd, fs, kern, alpha, prev, weight, freq)
    _compare_kernel(_kernel_call(hip, psd, fs, kern, alpha, weight, prev), ref)


def test_kernel_reproduces_the_golden_refresh(hip, golden):
    g = golden("spectrum")
    psd = np.ascontiguousarray(g["spn"].T)[None, None]              # [1, 1, frames, 513]
    alpha = float(g["kern_alpha"])
    kern = dsp.smoothing_kernel(alpha, 8192)
    db, pk, pt, st = _kernel_call(hip, psd, [0, psd.shape[2]], kern, alpha, g["weight"], np.zeros((1, 1, 513)))
    assert rel_max(st[0, 0], g["smoothed"]) < 1e-13 and np.max(np.abs(db[0, 0] - g["db"])) < 1e-9
    assert pk[0, 0] == int(g["peak_index"]) and pt[0, 0] == int(g["pitch_index"])


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _assert_equals_replay(res, ref, tol=1e-8):
    db = _np(res.db)
    assert db.shape == ref["db"].shape and np.array_equal(res.refresh_chunk, ref["refresh_chunk"])
    if db.size:
        print("dB max per stream", np.max(np.abs(db - ref["db"]), axis=(1, 2)))
        assert np.max(np.abs(db - ref["db"])) < tol
    assert np.array_equal(_np(res.fmax), ref["fmax"]) and np.array_equal(_np(res.fpitch), ref["fpitch"])
    assert np.array_equal(_np(res.peak_index), ref["peak_index"]) and np.array_equal(_np(res.pitch_index), ref["pitch_index"])


@pytest.mark.parametrize("fft_size,T", [(1024, 512 * 40), (8192, 512 * 128), (32, 512 * 12)])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("dual", [False, True])
def test_end_to_end_against_the_oracle_replay(hip, fft_size, T, S, dual):
    """fft_size 1024 fed 512 samples per chunk (two frames per refresh), the defaults (a refresh every fourth chunk), 32 (64 frames
    per refresh); numpy and CUDA input; keep="last" is the last row of keep="all"."""
    import torch
    from friture_amd.spectrum import SpectrumBatch
    rows = 2 if dual else 1
    x = H.streams(S, rows, T, seed=fft_size + S)
    ref = H.replay(x, fft_size=fft_size, weighting=1)
    H.assert_decisive(ref)
    sb = SpectrumBatch(fft_size, weighting=1, dual_channels=dual)
    xin = x if dual else x[:, 0]
    res = sb.run(xin)
    assert isinstance(res.db, np.ndarray) and res.db.dtype == np.float64 and res.peak_index.dtype == np.int32
    _assert_equals_replay(res, ref)
    dev = sb.run(torch.from_numpy(xin).cuda())
    assert dev.db.is_cuda and dev.fmax.is_cuda and dev.state.smoothed.is_cuda
    for a, b in zip(res[:5], dev[:5]):
        assert np.array_equal(a, _np(b))
    assert np.array_equal(res.state.smoothed, _np(dev.state.smoothed)) and np.array_equal(res.state.tail, _np(dev.state.tail))
    last = sb.run(xin, keep="last")
    for a, b in zip(res[:5], last[:5]):
        assert b.shape[1] == 1 and np.array_equal(a[:, -1:], b)
    assert np.array_equal(last.state.smoothed, res.state.smoothed)
    if S == 1:                                                       # one stream given without its axis
        one = sb.run(xin[0].astype(np.float64))
        assert one.db.shape == res.db.shape[1:] and np.array_equal(one.db, res.db[0]) and np.array_equal(one.fmax, res.fmax[0])


def test_end_to_end_ragged_ends_and_other_settings(hip):
    from friture_amd.spectrum import SpectrumBatch
    T = 60000
    x = H.streams(3, 1, T, seed=77)
    rng = np.random.default_rng(5)
    ends = np.cumsum(rng.choice([1, 100, 512, 512, 700, 5000], size=200))
    ends = ends[ends <= T]
    for kw in (dict(fft_size=1024, overlap=0.5, weighting=2, response_time=0.1), dict(fft_size=2048, overlap=0.0, weighting=3)):
        ref = H.replay(x[..., :ends[-1]], ends=ends, **kw)
        H.assert_decisive(ref)
        _assert_equals_replay(SpectrumBatch(**kw).run(x[:, 0], ends=ends), ref)


def test_largest_case_in_slabs(hip):
    """8 streams x 2^20 samples at the defaults under a 64 MiB scratch bound (several slabs)."""
    from friture_amd.spectrum import SpectrumBatch
    x = H.streams(8, 1, 1 << 20, seed=9)
    ref = H.replay(x)
    H.assert_decisive(ref)
    _assert_equals_replay(SpectrumBatch().run(x[:, 0], scratch_bytes=64 << 20), ref)


@pytest.mark.parametrize("dual", [False, True])
def test_equals_the_per_chunk_object(hip, dual):
    """SpectrumAnalyzerStream fed chunk by chunk: the same dB rows to 1e-9 (two GPU paths that sum at different sites) and the
    same fmax / fpitch."""
    from friture_amd.spectrum import SpectrumAnalyzerStream, SpectrumBatch
    kw = dict(fft_size=2048, overlap=0.75, weighting=2, response_time=0.05, dual_channels=dual)
    rows = 2 if dual else 1
    T = 512 * 60
    x = H.streams(1, rows, T, seed=21)
    H.assert_decisive(H.replay(x, fft_size=2048, weighting=2, response_time=0.05))
    res = SpectrumBatch(**kw).run(x if dual else x[:, 0])
    sa, r = SpectrumAnalyzerStream(**kw), 0
    for c in range(T // 512):
        got = sa.handle_new_data(x[0, :, c * 512:(c + 1) * 512].astype(np.float64))
        if got is None:
            continue
        assert res.refresh_chunk[r] == c
        assert np.max(np.abs(got[1] - res.db[0, r])) < 1e-9, (r, float(np.max(np.abs(got[1] - res.db[0, r]))))
        assert got[2] == res.fmax[0, r] and got[3] == res.fpitch[0, r]
        r += 1
    assert r == len(res.refresh_chunk) and r > 10


def _same(a, b):
    assert np.array_equal(_np(a.db), _np(b.db)) and np.array_equal(_np(a.peak_index), _np(b.peak_index))
    assert np.array_equal(_np(a.pitch_index), _np(b.pitch_index)) and np.array_equal(a.refresh_chunk, b.refresh_chunk)
    assert np.array_equal(_np(a.state.smoothed), _np(b.state.smoothed)) and np.array_equal(_np(a.state.tail), _np(b.state.tail))
    assert a.state.pending == b.state.pending


@pytest.mark.parametrize("dual", [False, True])
def test_split_and_slab_invariance_bit_for_bit(hip, dual):
    """run(x) == run(x[:c]) then run(x[c:], state): c before the first refresh (1024 < hop), inside a frame's span, on a hop, one
    chunk before the end; and the same bits under scratch bounds that make 1, 2 and many slabs."""
    import torch
    from friture_amd.spectrum import SpectrumBatch, SpectrumResult
    rows = 2 if dual else 1
    T = 512 * 140
    x = H.streams(3, rows, T, seed=31)
    xin = x if dual else x[:, 0]
    sb = SpectrumBatch(dual_channels=dual)
    whole = sb.run(xin)
    F = int(sb.schedule(T)[0][-1])
    per_frame = 3 * rows * sb.n_bins * 8
    for bound in (per_frame * (F // 2 + 1), per_frame * 3, 1):
        _same(sb.run(xin, scratch_bytes=bound), whole)
    for c in (1024, 2048 * 3 + 512, 2048 * 10, T - 512):
        a = sb.run(xin[..., :c])
        kept = (a.state.smoothed.copy(), a.state.tail.copy(), a.state.pending)
        b = sb.run(xin[..., c:], state=a.state, scratch_bytes=per_frame * 5)
        assert np.array_equal(kept[0], a.state.smoothed) and np.array_equal(kept[1], a.state.tail)     # not modified
        joined = SpectrumResult(np.concatenate([a.db, b.db], axis=1), np.concatenate([a.peak_index, b.peak_index], axis=1),
                                np.concatenate([a.pitch_index, b.pitch_index], axis=1), None, None,
                                np.concatenate([a.refresh_chunk, b.refresh_chunk + c // 512]), b.state)
        _same(joined, whole)
        assert np.array_equal(np.concatenate([a.fmax, b.fmax], axis=1), whole.fmax)
    xd = torch.from_numpy(xin).cuda()                                # the state carried on the device
    a = sb.run(xd[..., :2048 * 3 + 512])
    b = sb.run(xd[..., 2048 * 3 + 512:], state=a.state)
    assert np.array_equal(np.concatenate([_np(a.db), _np(b.db)], axis=1), whole.db) and np.array_equal(_np(b.state.tail), whole.state.tail)


def test_db_rows_go_into_curve_batch_in_place(hip):
    import torch
    from friture_amd.plotcurves import CurveBatch, initial_state
    from friture_amd.spectrum import SpectrumBatch
    x = H.streams(4, 1, 512 * 64, seed=41)[:, 0]
    res = SpectrumBatch(1024).run(torch.from_numpy(x).cuda())
    assert res.db.is_cuda and res.db.dtype == torch.float64 and res.db.is_contiguous()
    cb = CurveBatch(-140., 0.)
    got = cb.run(res.db)
    rows = res.db.cpu().numpy()
    want = PH.batch_np(rows, initial_state(rows.shape[2], 4), -140., 0.)
    for u, v in zip(got, want):
        assert np.array_equal(u.cpu().numpy(), v, equal_nan=True)


@pytest.mark.parametrize("weighting", [0, 1])
def test_silence(hip, weighting):
    from friture_amd.spectrum import SpectrumBatch
    res = SpectrumBatch(weighting=weighting).run(np.zeros((2, 512 * 64), np.float32))
    w = H.settings(8192, 0.75, weighting, 0.025)[4]
    assert res.db.shape == (2, 16, 4097) and np.max(np.abs(res.db - (-300.0 + w))) < 1e-9
    ref = dict(db=np.broadcast_to(-300.0 + w, res.db.shape), smoothed=np.zeros((2, 16, 1, 4097)), pitch_index=np.zeros((2, 16), int))
    H.assert_decisive(ref)
    assert np.all(res.pitch_index == 0) and np.all(res.peak_index == (0 if weighting == 0 else np.argmax(w)))
    assert not np.any(res.state.smoothed)


def test_argument_errors_carry_a_message_and_leave_the_state(hip):
    from friture_amd import _lib
    from friture_amd.spectrum import SpectrumBatch, SpectrumState
    sb = SpectrumBatch(1024)
    x = H.streams(2, 1, 4096, seed=1)[:, 0]
    good = sb.run(x)
    kept = (good.state.smoothed.copy(), good.state.tail.copy())
    with pytest.raises(ValueError, match="expected"):
        sb.run(np.zeros((2, 2, 2, 100), np.float32), state=good.state)                       # wrong rank
    with pytest.raises(TypeError, match="float32 or float64"):
        sb.run(x.astype(np.int16), state=good.state)                                           # wrong dtype
    with pytest.raises(ValueError, match="another shape"):
        sb.run(x[:1], state=good.state)                                                        # a state of two streams
    with pytest.raises(ValueError, match="another shape"):
        sb.run(x, state=SpectrumState(good.state.smoothed[..., :-1], good.state.tail, good.state.pending))
    with pytest.raises(ValueError, match="two rows"):
        SpectrumBatch(1024, dual_channels=True).run(np.zeros((2, 3, 4096), np.float32))
    assert np.array_equal(kept[0], good.state.smoothed) and np.array_equal(kept[1], good.state.tail)
    # the C entry: rows other than 1 or 2, a bad dtype, an unsorted or overlong refresh table — rejected before anything runs
    psd, st = np.ones((1, 1, 4, 8)), np.full((1, 1, 8), 0.5)
    kern = dsp.smoothing_kernel(0.1, 16)
    db, pk, pt = np.empty((1, 1, 8)), np.zeros(1, np.int32), np.zeros(1, np.int32)

    def call(rows=1, dtype=1, fs=(0, 4), bins=8):
        fs = np.asarray(fs, np.int64)
        return hip.frt_spectrum_batch(psd.ctypes.data, dtype, 1, rows, 4, bins, 8, 32, fs.ctypes.data_as(I64P), len(fs) - 1,
                                      kern.ctypes.data, 16, 0.1, None, st.ctypes.data, 1, db.ctypes.data, 0, pk.ctypes.data,
                                      pt.ctypes.data)
    for kwargs, msg in [({"rows": 3}, b"rows"), ({"rows": 0}, b"rows"), ({"dtype": 2}, b"dtype"), ({"fs": (0, 3, 2)}, b"not sorted"),
                        ({"fs": (0, 5)}, b"outside"), ({"bins": 2}, b"bins")]:
        assert call(**kwargs) == -1, kwargs
        assert msg in hip.frt_last_error(), (kwargs, hip.frt_last_error())
    assert np.all(st == 0.5)
    assert call() == 0 and not np.all(st == 0.5)
