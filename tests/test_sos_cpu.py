"""SosBatch (X6) without a GPU: the Butterworth design, the host's cell transition, the cell form's own accuracy, the refusals,
and that the default band front of room_acoustics / speech_transmission is still the FIR one."""
import numpy as np
import pytest

import sos_helpers as sh
from friture_amd import decay, sosfilter, sti


def response(sos, f, fs):
    """H(exp(2 pi i f / fs)) in long double: the evaluation adds nothing to what is measured."""
    th = 2 * np.pi * np.asarray(f, np.longdouble) / fs
    z = np.cos(th).astype(np.clongdouble) - 1j * np.sin(th)
    H = np.ones(len(z), np.clongdouble)
    for b0, b1, b2, a0, a1, a2 in np.asarray(sos).astype(np.longdouble):
        H *= (b0 + b1 * z + b2 * z * z) / (a0 + a1 * z + a2 * z * z)
    return H


OCTAVES_48K = [(lo, hi, 48000, 3) for lo, hi in decay.band_edges("octave")[1]]


@pytest.mark.parametrize("f_lo,f_hi,fs,order", OCTAVES_48K + [(89.1, 112.2, 48000, 3), (17.8, 22.4, 48000, 4), (707.0, 1414.0, 44100, 5),
                                                              (2828.0, 5657.0, 96000, 8), (500.0, 2000.0, 48000, 1)])
def test_butterworth_matches_its_closed_form(f_lo, f_hi, fs, order):
    """|H|^2 = 1 / (1 + W^(2 order)) across the band, at the edges and two octaves either side.  The edges are 1/2 to 1e-12 for
    every octave band; a float64 section cannot hold that for a narrow band low down: a1 and a2 are rounded to 2^-53 of 2 and 1,
    and |1 + a1 z + a2 z^2| at the edge of the 100 Hz third-octave is 1.6e-5 (20 Hz, order 4: 4.9e-7), so the rounding of the
    coefficients alone moves |H|^2 by up to 2 sum_k 1.5 * 2^-52 / |A_k|; those bands are held to that bound."""
    sos = sosfilter.butter_band_sos(f_lo, f_hi, fs, order)
    assert sos.shape == (order, 6) and np.all(sos[:, 3] == 1)
    w = lambda f: np.tan(np.pi * np.asarray(f, np.longdouble) / fs)
    f0 = np.sqrt(f_lo * f_hi)
    grid = np.concatenate([np.geomspace(f_lo, f_hi, 41), np.geomspace(f0 / 4, min(f0 * 4, 0.49 * fs), 41), [f_lo, f_hi]])
    W = (w(grid) ** 2 - w(f_lo) * w(f_hi)) / (w(grid) * (w(f_hi) - w(f_lo)))
    want = 1 / (1 + W ** (2 * order))
    got = np.abs(response(sos, grid, fs)) ** 2
    z = np.exp(-2j * np.pi * grid[:, None] / fs)
    rounding = np.sum(3.0 * 2.0 ** -52 / np.abs(1 + sos[:, 4] * z + sos[:, 5] * z * z), axis=1)
    narrow = f_hi / f_lo < 1.9
    assert np.all(np.abs(got - want) <= np.maximum(1e-12, rounding))
    assert np.allclose(np.asarray(want[-2:], np.float64), 0.5, rtol=0, atol=1e-15)
    assert np.all(np.abs(got[-2:] - 0.5) <= (np.maximum(1e-12, rounding[-2:]) if narrow else 1e-12))


def test_butterworth_matches_scipy():
    signal = pytest.importorskip("scipy.signal")
    for f_lo, f_hi, fs, order in [(88.4, 176.8, 48000, 3), (1122.0, 1413.0, 44100, 4), (2828.0, 5657.0, 96000, 6)]:
        ours = sosfilter.butter_band_sos(f_lo, f_hi, fs, order)
        theirs = signal.butter(order, [f_lo, f_hi], "band", fs=fs, output="sos")
        grid = np.geomspace(f_lo / 4, min(f_hi * 4, 0.49 * fs), 200)
        assert np.max(np.abs(response(ours, grid, fs) - response(theirs, grid, fs))) < 1e-9


@pytest.mark.parametrize("fs", [44100, 48000, 96000])
@pytest.mark.parametrize("bands", ["octave", "third"])
def test_poles_lie_inside_the_unit_circle(bands, fs):
    centres, sos = sosfilter.band_sos(bands, fs, 3)
    assert sos.shape == (len(centres), 3, 6)
    for a1, a2 in sos[..., 4:].reshape(-1, 2):
        assert np.max(np.abs(np.roots([1.0, a1, a2]))) < 1
    sosfilter.SosBatch(sos)                                      # and the host's own check agrees


@pytest.mark.parametrize("cell", [32, 256])
def test_host_transition_matches_explicit_steps(cell):
    _, sos = sosfilter.band_sos("octave", 48000, 3)
    batch = sosfilter.SosBatch(sos, cell=cell)
    coef, M, M64 = batch.tables()
    assert np.array_equal(coef, sh.normalise(sos)[..., [0, 1, 2, 4, 5]])
    assert np.array_equal(M, sh.transition(sh.normalise(sos), cell))
    assert np.array_equal(M64, sh.transition(sh.normalise(sos), 64 * cell))
    # and against float64 steps of a random state: the two differ by rounding only
    rng = np.random.default_rng(3)
    z = rng.standard_normal((6, 6))
    want = z.copy()
    sh._steps(np.zeros((6, cell)), sh.normalise(sos), want, np.float64)
    got = np.einsum("fij,fj->fi", M, z)
    assert np.max(np.abs(got - want)) < 1e-12 * np.max(np.abs(want))


def cell_form_within_bar(name, args, cell):
    x, sos, fan, yld, y64 = sh.cached(name, *args)
    d, b = sh.distance(sh.cell_form(x, sos, cell, fan), yld), sh.bar(y64, yld)
    print(f"{name} {args}: e_seq {sh.distance(y64, yld).max():.2e}, cell form {d.max():.2e}, largest ratio to e_seq "
          f"{(d / np.maximum(sh.distance(y64, yld), 1e-300)).max():.1f}")
    assert np.all(d <= b)


@pytest.mark.parametrize("kind", sh.SEAM_KINDS)
@pytest.mark.parametrize("T", sh.SEAM_LENGTHS)
def test_cell_form_stays_within_the_bar_on_the_seam_inputs(T, kind):
    cell_form_within_bar("seam", (T, kind), sh.SEAM_CELL)


def test_cell_form_stays_within_the_bar_on_the_long_row():
    cell_form_within_bar("seam", (sh.LONG_LENGTH, "bank6"), sh.SEAM_CELL)


@pytest.mark.parametrize("bands", ["octave", "third"])
def test_cell_form_stays_within_the_bar_on_the_banks(bands):
    cell_form_within_bar("bank", (bands,), sosfilter.SosBatch(sh.cached("bank", bands)[1]).cell)


def test_closed_form_impulse_response_is_the_sequential_one():
    sos = sosfilter.band_sos("octave", 48000, 3)[1][0]
    x = np.zeros((1, 4096))
    x[0, 0] = 1
    yld = sh.sequential(x, sos, dtype=np.longdouble)[0]
    h = sh.impulse_response(sos, 4096)
    assert np.max(np.abs(h - yld)) < 1e-15 * np.max(np.abs(yld))


def test_refusals():
    good = sosfilter.butter_band_sos(500.0, 1000.0, 48000, 3)
    with pytest.raises(ValueError, match="sections"):
        sosfilter.SosBatch(np.tile(good, (3, 1)))                # K = 9
    with pytest.raises(ValueError, match="filters"):
        sosfilter.SosBatch(np.tile(good, (65, 1, 1)))
    bad = good.copy()
    bad[1, 5] = 1.0                                              # a pole on the unit circle
    with pytest.raises(ValueError, match="pole"):
        sosfilter.SosBatch(bad)
    bad = good.copy()
    bad[0, 4] = 2.5
    with pytest.raises(ValueError, match="pole"):
        sosfilter.SosBatch(bad)
    bad = good.copy()
    bad[2, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        sosfilter.SosBatch(bad)
    for cell in (16, 48, 2048, 64.0, True):
        with pytest.raises(ValueError, match="cell"):
            sosfilter.SosBatch(good, cell=cell)
    batch = sosfilter.SosBatch(good, cell=64)
    x = np.zeros((2, 100))
    state = sosfilter.SosState(np.zeros((2, batch.state_length)), 2, 10, batch.settings)
    with pytest.raises(ValueError, match="reverse"):
        batch.run(x, reverse=True, state=state)
    with pytest.raises(ValueError, match="shape"):
        batch.run(x, state=sosfilter.SosState(np.zeros((2, batch.state_length - 1)), 2, 10, batch.settings))
    with pytest.raises(ValueError, match="shape"):
        batch.run(x, fan=True, state=sosfilter.SosState(np.zeros((3, batch.state_length)), 3, 10, batch.settings))
    with pytest.raises(ValueError, match="settings"):
        batch.run(x, state=state._replace(settings=sosfilter.SosBatch(good, cell=32).settings))
    # a0 != 1 is normalised, not refused
    scaled = good * 2.0
    assert np.array_equal(sosfilter.SosBatch(scaled).sos, sosfilter.SosBatch(good).sos)


def test_library_refuses_what_the_class_refuses():
    import ctypes

    from friture_amd import _lib
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    good = sosfilter.butter_band_sos(500.0, 1000.0, 48000, 3)
    bad = good.copy()
    bad[1, 5] = 1.0
    for sos, F, K, cell, word in [(good, 1, 9, 0, b"sections"), (good, 65, 3, 0, b"filters"), (good, 1, 3, 48, b"cell"), (bad, 1, 3, 0, b"pole")]:
        assert lib.frt_sos_tables(sos.ctypes.data_as(dp), F, K, cell, None, None, None) == -1
        assert b"frt_sos_tables" in lib.frt_last_error() and word in lib.frt_last_error()
    assert lib.frt_sos_state_length(3) == 30 == sosfilter.SosBatch(good).state_length
    assert sosfilter.SosBatch(good).cell == lib.frt_sos_default_cell()


class Stop(Exception):
    pass


@pytest.mark.parametrize("front", ["room", "speech"])
def test_the_default_band_front_is_the_fir_one(front, monkeypatch):
    """With the keyword left out (and with filters="fir") ConvolveBatch is constructed and SosBatch is not.  No GPU: the
    broadband DecayBatch.run is stubbed and the first ConvolveBatch ends the call."""
    made = []

    def convolve_batch(h, *a, **k):
        made.append("convolve")
        raise Stop

    def sos_batch(*a, **k):
        made.append("sos")
        raise Stop

    fake = decay.DecayResult(*[np.zeros(1, np.int64)] * len(decay.DecayResult._fields))
    monkeypatch.setattr(decay.DecayBatch, "run", lambda self, ir, **k: fake)
    monkeypatch.setattr(decay.convolve, "ConvolveBatch", convolve_batch)
    monkeypatch.setattr(sosfilter, "SosBatch", sos_batch)
    ir = np.zeros((1, 4800))
    call = decay.room_acoustics if front == "room" else sti.speech_transmission
    for kw in ({}, {"filters": "fir"}):
        made.clear()
        with pytest.raises(Stop):
            call(ir, **kw)
        assert made == ["convolve"]
    made.clear()
    with pytest.raises(Stop):
        call(ir, filters="butterworth")
    assert made == ["sos"]
    with pytest.raises(ValueError, match="filters"):
        call(ir, filters="chebyshev")
