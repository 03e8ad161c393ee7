"""TransferBatch without a GPU: the restatement of X1 (tests/transfer_helpers.py) against scipy.signal, the frame count, the
delay convention, the bookkeeping of `average`, and the host side of friture_amd/transfer.py: arguments, the state's layout
and its rejections, the bound symbols and the argument checks of the C entry points that precede any device call."""
import ctypes

import numpy as np
import pytest

import transfer_helpers as th
from friture_amd import transfer as tf


# ---- the restatement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N, hop", [(64, 16), (512, 256), (1024, 385)])
def test_restatement_equals_scipy(N, hop):
    """h1 and coherence of the restatement against scipy.signal.csd / welch / coherence within 1e-13 (measured: 2e-15);
    hop <= N, which is all that scipy's noverlap can say."""
    signal = pytest.importorskip("scipy.signal")
    x, y = th.standard_case(N, hop)[0]
    w = th.window_of("hann", N)
    ref = th.restate(x, y, N, hop)
    kw = dict(window=w, nperseg=N, noverlap=N - hop, detrend=False)
    _, pxy = signal.csd(x, y, **kw)
    _, pxx = signal.welch(x, **kw)
    _, coh = signal.coherence(x, y, **kw)
    h1 = pxy / pxx
    d_h1 = np.max(np.abs(ref["h1"][0] - h1)) / np.max(np.abs(h1))
    d_coh = np.max(np.abs(ref["coherence"][0] - coh))
    print(f"N {N} hop {hop}: h1 {d_h1:.2e}, coherence {d_coh:.2e}")
    assert d_h1 <= 1e-13 and d_coh <= 1e-13


def test_sxx_is_the_packages_psd_scale():
    """A full-scale sine at a bin centre through a rectangular window: |X|^2 = 1/4 at that bin."""
    N = 64
    x = np.cos(2 * np.pi * 8 * np.arange(N) / N)
    ref = th.restate(x, x, N, N, window=np.ones(N))
    assert abs(ref["sxx"][0, 8] - 0.25) < 1e-15 and abs(ref["h1"][0, 8] - 1) < 1e-15


@pytest.mark.parametrize("N, hop, d", [(64, 32, 0), (64, 32, 5), (64, 32, -5), (64, 100, 0), (128, 1, 7)])
def test_frame_count(N, hop, d):
    b = tf.TransferBatch(N, hop, delay=d)
    for n in (0, N - 1, N + abs(d) - 1, N + abs(d), N + abs(d) + hop - 1, N + abs(d) + hop, N + abs(d) + 7 * hop + 3):
        want = sum(1 for f in range(n) if max(0, -d) + f * hop + N <= n and max(0, d) + f * hop + N <= n)
        assert b.frames_after(n) == th.frames_after(n, N, hop, d) == want


def test_delay_convention_positive_means_the_measured_row_lags():
    rng = np.random.default_rng(3)
    N, hop, d = 64, 32, 9
    x = rng.standard_normal(N + 10 * hop + d)
    y = np.concatenate([np.zeros(d), x[:-d]])                    # y[t] = x[t - d]
    ref = th.restate(x, y, N, hop, delay=d)
    assert np.max(np.abs(ref["h1"] - 1)) < 1e-12 and np.max(np.abs(ref["coherence"] - 1)) < 1e-12
    assert np.max(np.abs(th.restate(x, y, N, hop, delay=0)["h1"] - 1)) > 0.1
    ref = th.restate(y, x, N, hop, delay=-d)                     # the reference row lags: a negative delay
    assert np.max(np.abs(ref["h1"] - 1)) < 1e-12
    assert np.max(np.abs(th.restate(y, x, N, hop, delay=d)["h1"] - 1)) > 0.1


def test_average_bookkeeping():
    N, hop = 64, 32
    b = tf.TransferBatch(N, hop, average=3)
    n7 = N + 6 * hop                                             # 7 frames
    assert b.frames_after(n7) == 7 and b.estimates_after(n7) == 2
    assert b.emitted(0, N - 1) == 0 and b.emitted(0, N + 2 * hop - 1) == 0 and b.emitted(0, N + 2 * hop) == 1
    assert b.emitted(N + 2 * hop, n7) == 1 and b.emitted(n7, n7 + 1) == 0
    running = tf.TransferBatch(N, hop)
    assert running.emitted(0, N - 1) == 0 and running.emitted(0, N) == 1 and running.emitted(n7, n7) == 1
    x, y = th.standard_case(N, hop)[0]
    ref = th.restate(x, y, N, hop, average=3)
    assert ref["sxx"].shape == (13, 33) and np.all(ref["frames"] == 3)
    X, Y = th.frame_spectra(x, y, N, hop)
    assert np.allclose(ref["sxy"][4], np.mean(np.conj(X[12:15]) * Y[12:15], 0), rtol=0, atol=1e-18)
    assert th.restate(x, y, N, hop)["frames"].tolist() == [40]


def test_silence_and_a_single_frame_in_the_restatement():
    x = np.random.default_rng(1).standard_normal(64)
    ref = th.restate(x, np.zeros(64), 64, 32)
    assert np.all(ref["h1"] == 0) and np.all(ref["coherence"] == 0)
    ref = th.restate(x, x[::-1].copy(), 64, 32)
    assert np.max(np.abs(ref["coherence"] - 1)) < 1e-9


# ---- the host side of TransferBatch ---------------------------------------------------------------------------------------------

def test_defaults():
    b = tf.TransferBatch()
    assert (b.fft_size, b.hop, b.average, b.delay, b.bins) == (8192, 4096, None, 0, 4097)
    assert np.array_equal(b.window, th.window_of("hann", 8192)) and b.freq.shape == (4097,) and b.freq[-1] == 24000.0
    assert tf.RUN == th.RUN == 16


@pytest.mark.parametrize("kwargs", [dict(fft_size=32), dict(fft_size=96), dict(fft_size=16384), dict(fft_size=64.0), dict(hop=0),
                                    dict(hop=1.5), dict(average=0), dict(average=2.0), dict(delay=96001), dict(delay=-96001),
                                    dict(delay=0.5), dict(window="hamming"), dict(window=np.ones(63)),
                                    dict(window=np.full(64, np.nan))])
def test_argument_errors(kwargs):
    with pytest.raises(ValueError):
        tf.TransferBatch(**{"fft_size": 64, **kwargs})


def test_input_errors_precede_the_device():
    b = tf.TransferBatch(64)
    with pytest.raises(TypeError):
        b.run([[0.0] * 64] * 2)
    with pytest.raises(TypeError):
        b.run(np.zeros((2, 64), np.int16))
    with pytest.raises(ValueError):
        b.run(np.zeros((1, 3, 64)))
    with pytest.raises(ValueError):
        b.run(np.zeros(64))
    with pytest.raises(ValueError):
        b.run(np.zeros((2, 64)), scratch_bytes=-1)


def state_of(b, S, n):
    layout, length = tf.state_layout(S, b.fft_size, b.hop, b.delay, n)
    return tf.TransferState(np.zeros(length), S, n, layout["row0"][1][1], b.settings)


def test_state_layout():
    b = tf.TransferBatch(64, 48, delay=5)
    for n, row0, row1 in ((0, 0, 0), (3, 3, 0), (68, 68, 63), (69, 21, 16), (116, 68, 63), (117, 21, 16)):
        layout, length = tf.state_layout(2, 64, 48, 5, n)
        assert layout["row0"][1] == (2, row0) and layout["row1"][1] == (2, row1), n
        assert length == 2 * (2 * 33 * 4 + row0 + row1)
        parts = b.state_parts(state_of(b, 2, n))
        assert parts["sum"].shape == parts["open_run"].shape == (2, 33, 4) and parts["row1"].shape == (2, row1)
    far = tf.state_layout(1, 64, 1000, 0, 64)[0]                 # a hop beyond the samples seen: nothing to carry
    assert far["row0"][1] == (1, 0)


def test_state_errors_precede_the_device():
    b = tf.TransferBatch(64, 32, average=4, delay=3)
    good = state_of(b, 2, 100)
    x = np.zeros((2, 2, 10))
    for other in (tf.TransferBatch(128, 32, average=4, delay=3), tf.TransferBatch(64, 16, average=4, delay=3),
                  tf.TransferBatch(64, 32, average=None, delay=3), tf.TransferBatch(64, 32, average=4, delay=-3),
                  tf.TransferBatch(64, 32, np.ones(64), average=4, delay=3)):
        with pytest.raises(ValueError, match="other settings"):
            other.run(x, good)
    with pytest.raises(ValueError, match="another shape"):
        b.run(np.zeros((3, 2, 10)), good)
    with pytest.raises(ValueError, match="another shape"):
        b.run(x, good._replace(data=good.data[:-1]))
    with pytest.raises(ValueError, match="another stream"):
        b.run(x, good._replace(pending=good.pending + 1))
    with pytest.raises(ValueError, match="another stream"):
        b.run(x, good._replace(n_in=-1))


# ---- the C entry points ---------------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_reject_bad_arguments_before_any_device_call():
    from friture_amd import _lib
    lib = _lib.load()
    for name in ("frt_transfer_create", "frt_transfer_set_stream", "frt_transfer_run", "frt_transfer_destroy"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    w = np.ones(16384)
    wp = w.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for args, status, word in (((16384, 64, wp, 0, 0), -4, b"not supported"), ((100, 64, wp, 0, 0), -1, b"fft_size"),
                               ((32, 64, wp, 0, 0), -1, b"fft_size"), ((64, 0, wp, 0, 0), -1, b"hop"), ((64, 32, wp, -1, 0), -1, b"average"),
                               ((64, 32, wp, 0, 96001), -1, b"delay"), ((64, 32, None, 0, 0), -1, b"window")):
        h = ctypes.c_void_p()
        assert lib.frt_transfer_create(ctypes.byref(h), *args) == status and h.value is None
        assert b"frt_transfer_create" in lib.frt_last_error() and word in lib.frt_last_error()
    assert lib.frt_transfer_run(None, None, 0, 1, 0, 0, 0, None, None, 0, 0, None, None) == -1
    assert b"frt_transfer_run" in lib.frt_last_error()
    assert lib.frt_transfer_set_stream(None, None) == -1
    lib.frt_transfer_destroy(None)
