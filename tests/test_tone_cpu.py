"""X9 without a GPU: the numpy restatement against closed forms, the settings' validation on both sides of the C boundary, the
state layout and the lobe-ownership rule."""
import ctypes
import math

import numpy as np
import pytest

import tone_helpers as th
from friture_amd import distortion
from friture_amd.distortion import ToneBatch, frames_after, kaiser_lobe, state_layout

FS = th.FS


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1024, 8192])
@pytest.mark.parametrize("f1", [997.0, 1000.0, 3141.59])
def test_restatement_meets_the_closed_forms(N, f1):
    """A unit sine with harmonics 2, 3, 5 at 1e-3, 1e-5, 1e-4 and white noise at 1e-8 under Kaiser 20, L = 8.  Measured with a
    prototype: harmonic levels within 9e-4 dB of their amplitudes, freq within 2.5e-8 Hz, P1 within 1.5e-9 of 0.5, the residual
    within 0.8 dB of the noise power; the bars are 0.01 dB, 1e-6 Hz, 1e-8 and 1.5 dB (the last for the variance of a noise
    estimate over about N/2 bins).  The noise power is that of the residual's own bins: white noise of variance v puts
    c_k v / N into bin k, and the lobes of the present orders take their bins out of the residual."""
    L, H, hop = 8, 10, N // 2
    kappa = f1 * N / FS
    x = th.tone(kappa, N, N + 3 * hop, seed=N + int(f1))
    ka, kb, klo, khi = th.settings_bins(N, L)
    r = th.restate(x, N, hop, np.kaiser(N, 20.0), L, H, ka, kb, klo, khi)
    assert r["valid"].all() and r["n_valid"][0] == 4
    freq = r["kappa"] * FS / N
    print("freq distance", np.abs(freq - f1).max(), "P1 distance", np.abs(r["fund"] - 0.5).max())
    assert np.abs(freq - f1).max() <= 1e-6
    assert np.abs(r["fund"] - 0.5).max() <= 1e-8
    for h, a in th.AMPLITUDES.items():
        level = 10 * np.log10(r["harmonics"][0, :, h - 2] / r["fund"][0])
        print("order", h, "level distance dB", np.abs(level - 20 * math.log10(a)).max())
        assert np.abs(level - 20 * math.log10(a)).max() <= 0.01
    weight = np.full(N // 2 + 1, 2.0)
    weight[0] = weight[-1] = 1.0
    weight[:ka] = 0
    for c in r["centres"][0, 0]:
        if c >= 0:
            weight[c - L:c + L + 1] = 0
    noise = th.NOISE ** 2 * weight.sum() / N
    mean = r["totals"][0, 2] / r["n_valid"][0]
    print("residual against the noise power dB", 10 * math.log10(mean / noise))
    assert abs(10 * math.log10(mean / noise)) <= 1.5


def test_float64_and_longdouble_restatements_agree_on_the_standard_case():
    x, settings, r64, rld = th.standard_case(1024, 512, 3, 2)
    d = th.distances(r64, rld)
    print(d)
    assert d["fund"] <= 1e-15 and d["kappa"] <= 1e-11
    assert np.array_equal(np.isnan(r64["harmonics"]), np.isnan(rld["harmonics"]))


# ---- the lobe-ownership rule ------------------------------------------------------------------------------------------------------

def test_a_bin_counts_once_for_the_lowest_order_that_holds_it():
    """kappa below 2 L + 1 with L = 2: c1 = 5, lobe 1 = [3, 7]; c2 = rint(2 * 4.714) = 9, lobe 2 = [max(7, 8), 11] = [8, 11]."""
    L, H, M = 2, 4, 32
    Q = np.zeros(M + 1)
    Q[3], Q[5], Q[7] = 0.25, 0.5, 0.125          # P1 = 0.875, kappa = 4.125 / 0.875 = 4.714..
    Q[8], Q[9], Q[12] = 2.0, 4.0, 8.0
    P1, kappa, c, spans = th.lobes(Q, 5, L, H, M)
    assert P1 == 0.875 and kappa == 4.125 / 0.875
    assert c == [5, 9, 14, 19] and spans == [(3, 7), (8, 11), (12, 16), (17, 21)]
    P = th.lobe_sums(Q, spans)
    assert P[0] == 6.0                           # bins 8 .. 11; bin 7 went to the fundamental
    assert P[1] == 8.0 and P[2] == 0.0
    # everything is inside a lobe or zero: no residual; a loud bin 22 is the residual, unless the band ends before it
    assert th.residual(Q, spans, L + 1, M) == 0.0
    Q[22] = 3.0
    assert th.residual(Q, spans, L + 1, M) == 3.0
    assert th.residual(Q, spans, L + 1, 21) == 0.0


def test_an_order_is_present_up_to_the_band_edge_and_absent_one_bin_later():
    L, H, M = 2, 3, 32
    Q = np.zeros(M + 1)
    Q[10] = 1.0                                  # kappa = 10: c2 = 20, c3 = 30
    for kb, present in ((32, True), (31, False)):
        _, _, c, spans = th.lobes(Q, 10, L, H, kb)
        assert (c[2] == 30) == present and (spans[2] is not None) == present
        assert np.isnan(th.lobe_sums(Q, spans)[1]) != present


# ---- settings ---------------------------------------------------------------------------------------------------------------------

def test_defaults():
    tb = ToneBatch()
    assert (tb.fft_size, tb.hop, tb.lobe, tb.harmonics, tb.ka, tb.kb) == (8192, 4096, 8, 10, 9, 4096)
    assert tb.klo.tolist() == [17] and tb.khi.tolist() == [4088] and tb.gate == 0.0
    assert kaiser_lobe(20.0) == 8 and kaiser_lobe(9.0) == 5
    assert np.array_equal(tb.window, np.kaiser(8192, 20.0))


def test_band_and_f0_give_the_documented_bins():
    tb = ToneBatch(fft_size=1024, band=(500.0, 10000.0), f0=[1000.0, 3000.0])
    ka, kb, klo, khi = th.settings_bins(1024, 8, (500.0, 10000.0), [1000.0, 3000.0])
    assert (tb.ka, tb.kb) == (ka, kb) == (11, 213)
    assert tb.klo.tolist() == klo.tolist() == [19, 56] and tb.khi.tolist() == khi.tolist() == [29, 72]


@pytest.mark.parametrize("bad", [
    dict(fft_size=256), dict(fft_size=32768), dict(fft_size=1000), dict(fft_size=1024.0), dict(hop=0), dict(hop=(1 << 30) + 1),
    dict(hop=1.5), dict(window="hann"), dict(window=("kaiser", -1.0)), dict(window=("hann", 1.0)), dict(window=np.ones(100), lobe=3),
    dict(window=np.ones(8192)), dict(window=np.zeros(8192), lobe=3), dict(window=np.full(8192, np.nan), lobe=3), dict(lobe=0),
    dict(lobe=17), dict(lobe=2.0), dict(harmonics=1), dict(harmonics=33), dict(band=(100.0,)), dict(band=(2000.0, 1000.0)),
    dict(band=(-1.0, 1000.0)), dict(band=(1000.0, 1010.0)), dict(f0=-5.0), dict(f0=float("nan")), dict(f0=10.0),
    dict(band=(1000.0, 5000.0), f0=8000.0), dict(gate_db=float("nan")), dict(gate_db="loud"), dict(fs=0), dict(fs=float("inf")),
])
def test_bad_settings_raise_before_any_device_call(bad):
    with pytest.raises(ValueError):
        ToneBatch(**bad)


def test_bad_input_raises_before_any_device_call():
    tb = ToneBatch(fft_size=1024, f0=[1000.0, 2000.0])
    with pytest.raises(ValueError, match="f0 has 2 values for 3 streams"):
        tb.run(np.zeros((3, 4096)))
    with pytest.raises(TypeError):
        tb.run(np.zeros((2, 4096), np.int16))
    with pytest.raises(ValueError):
        tb.run(np.zeros((2, 2, 4096)))
    with pytest.raises(ValueError):
        ToneBatch(fft_size=1024).run(np.zeros(4096), scratch_bytes=-1)


def _create(lib, fft_size=1024, hop=512, window=True, lobe=8, harmonics=10, ka=9, kb=512, klo=17, khi=504, n_search=1, gate=0.0):
    w = np.kaiser(max(int(fft_size), 1), 20.0) if window is True else window
    wp = None if w is None else w.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    lo, hi = (ctypes.c_int * 1)(klo), (ctypes.c_int * 1)(khi)
    h = ctypes.c_void_p()
    rc = lib.frt_tone_create(ctypes.byref(h), fft_size, hop, wp, lobe, harmonics, ka, kb, lo, hi, n_search, gate)
    return rc, h, lib.frt_last_error().decode()


@pytest.mark.parametrize("bad, word", [
    (dict(fft_size=256), "fft_size 256"), (dict(fft_size=32768), "fft_size 32768"), (dict(fft_size=1000), "fft_size 1000"),
    (dict(hop=0), "hop 0"), (dict(hop=(1 << 30) + 1), "hop"), (dict(lobe=0), "lobe 0"), (dict(lobe=17), "lobe 17"),
    (dict(harmonics=1), "harmonics 1"), (dict(harmonics=33), "harmonics 33"), (dict(ka=8), "ka 8"), (dict(kb=513), "kb 513"),
    (dict(ka=300, kb=200, klo=208, khi=208), "ka 300"), (dict(klo=16), "klo 16"), (dict(khi=505), "khi 505"),
    (dict(klo=100, khi=99), "klo 100"), (dict(n_search=0), "n_search 0"), (dict(gate=-1.0), "gate"),
    (dict(gate=float("nan")), "gate"), (dict(window=None), "window"), (dict(window=np.full(1024, np.inf)), "window[0]"),
    (dict(window=np.zeros(1024)), "window"),
])
def test_the_c_entry_point_names_the_bad_argument(bad, word):
    from friture_amd import _lib
    lib = _lib.load()
    rc, h, message = _create(lib, **bad)
    assert rc == -1 and h.value is None
    assert "frt_tone_create" in message and word in message, message


def test_the_c_run_entry_point_rejects_a_null_handle():
    from friture_amd import _lib
    lib = _lib.load()
    rc = lib.frt_tone_run(None, None, 0, 1, 0, 0, None, None, 0, 0, None, None)
    assert rc == -1 and "frt_tone_run: null handle" in lib.frt_last_error().decode()
    assert lib.frt_tone_set_stream(None, None) == -1
    lib.frt_tone_destroy(None)


# ---- frames and state -------------------------------------------------------------------------------------------------------------

def test_frames_after():
    assert [frames_after(n, 1024, 512) for n in (0, 1023, 1024, 1535, 1536, 2048)] == [0, 0, 1, 1, 2, 3]
    assert [frames_after(n, 512, 643) for n in (511, 512, 1154, 1155, 1798)] == [0, 1, 1, 2, 3]
    assert ToneBatch(fft_size=512, hop=7).frames_after(512 + 70) == 11


@pytest.mark.parametrize("N, hop, n_in, pending", [(1024, 512, 0, 0), (1024, 512, 1000, 1000), (1024, 512, 1024, 512),
                                                   (1024, 512, 1700, 676), (512, 643, 600, 0), (512, 643, 650, 7),
                                                   (512, 643, 1155, 0), (512, 1, 4000, 511)])
def test_state_layout(N, hop, n_in, pending):
    """totals [S, 3 + H] | row [S, pending]: the samples from min(n, F(n) hop) on, at most N - 1 of them."""
    S, H = 3, 7
    layout, length = state_layout(S, N, hop, H, n_in)
    assert layout["totals"] == (0, (S, 3 + H)) and layout["row"] == (S * (3 + H), (S, pending))
    assert length == S * (3 + H + pending) and pending <= N - 1


def test_a_state_of_other_settings_is_refused():
    tb, other = ToneBatch(fft_size=1024), ToneBatch(fft_size=1024, harmonics=5)
    _, n = state_layout(1, 1024, 512, 10, 100)
    state = distortion.ToneState(np.zeros(n), 1, 100, 100, tb.settings)
    assert tb._check_state(state, 1)[1] == 100
    with pytest.raises(ValueError, match="other settings"):
        other._check_state(state, 1)
    with pytest.raises(ValueError, match="another shape"):
        tb._check_state(state, 2)
    with pytest.raises(ValueError, match="another stream"):
        tb._check_state(state._replace(pending=99), 1)
