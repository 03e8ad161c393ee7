"""The host side of SoundLevelBatch (X7): the A and C weighting designs against the analogue formula, the library's tables
against the helper's long double ones, the float64 restatement of the cell form against the long double recurrence on the inputs
that tests/test_soundlevel_gpu.py shares, percentile levels, and the refusals.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

import soundlevel_helpers as sl
from friture_amd import _lib, soundlevel

FS = 48000


def analogue_db(kind, f):
    """The analogue weighting in dB, unnormalised, in long double."""
    f2 = np.asarray(f, np.longdouble) ** 2
    f1, fa, fb, f4 = (np.longdouble(v) ** 2 for v in (soundlevel.F1, soundlevel.F2, soundlevel.F3, soundlevel.F4))
    if kind == "A":
        h = f4 * f2 * f2 / ((f2 + f1) * np.sqrt((f2 + fa) * (f2 + fb)) * (f2 + f4))
    else:
        h = f4 * f2 / ((f2 + f1) * (f2 + f4))
    return 20 * np.log10(h)


def sections_db(sos, f, fs):
    """The sections' response in dB, straight from the coefficients, in long double."""
    zi = np.exp(-2j * np.longdouble(np.pi) * np.asarray(f, np.longdouble) / np.longdouble(fs)).astype(np.clongdouble)
    h = np.ones(zi.shape, np.clongdouble)
    for b0, b1, b2, a0, a1, a2 in sos.astype(np.longdouble):
        h = h * (b0 + b1 * zi + b2 * zi * zi) / (a0 + a1 * zi + a2 * zi * zi)
    return 20 * np.log10(np.abs(h))


@pytest.mark.parametrize("fs", [44100, 48000, 96000])
@pytest.mark.parametrize("kind", ["A", "C"])
def test_weighting_is_the_analogue_curve_at_the_warped_frequency(kind, fs):
    sos = soundlevel.weighting_sos(kind, fs)
    assert sos.shape == ((3, 6) if kind == "A" else (2, 6)) and sos.dtype == np.float64 and np.all(sos[:, 3] == 1.0)
    f = np.geomspace(10.0, 20000.0, 60)
    warp = lambda v: np.longdouble(fs) / np.pi * np.tan(np.pi * np.asarray(v, np.longdouble) / fs)
    want = analogue_db(kind, warp(f)) - analogue_db(kind, warp(1000.0))
    got = sections_db(sos, f, fs)
    print(f"{kind} at {fs}: largest deviation {float(np.abs(got - want).max()):.2e} dB")
    assert np.abs(got - want).max() < 1e-9
    assert abs(float(sections_db(sos, 1000.0, fs))) < 1e-12
    for a1, a2 in sos[:, 4:]:
        assert np.max(np.abs(np.roots([1.0, a1, a2]))) < 1


def test_bilinear_deviation_table_at_48k():
    """The docstring's table: the digital response minus the analogue curve at the same frequency, the same for A and C."""
    table = {4000.0: -0.04, 8000.0: -0.54, 10000.0: -1.22, 12500.0: -2.67, 16000.0: -6.4, 20000.0: -15.8}
    for kind in ("A", "C"):
        sos = soundlevel.weighting_sos(kind, FS)
        for f, dev in table.items():
            got = float(sections_db(sos, f, FS) - (analogue_db(kind, f) - analogue_db(kind, 1000.0)))
            assert abs(got - dev) < (0.1 if abs(dev) > 5 else 0.01), (kind, f, got)      # one unit of the last printed digit
        low = np.geomspace(10.0, 500.0, 40)
        assert np.abs(sections_db(sos, low, FS) - (analogue_db(kind, low) - analogue_db(kind, 1000.0))).max() < 0.0045       # 0.004 rounded


def test_z_and_unknown_kinds():
    assert soundlevel.weighting_sos("Z") is None
    for kind in ("B", "a", None):
        with pytest.raises(ValueError, match="weighting"):
            soundlevel.weighting_sos(kind)


@pytest.mark.parametrize("fs,taus,interval,cell", [(48000, (0.125, 1.0), 4800, None), (48000, (0.002, 0.02), 480, 32),
                                                   (44100, (0.035, 0.125, 1.0, 10.0), 1024, 1024), (96000, (0.125,), 16, 16)])
def test_tables_are_the_long_double_values(fs, taus, interval, cell):
    batch = soundlevel.SoundLevelBatch("Z", interval=interval, taus=taus, fs=fs, cell=cell)
    got, want = batch.tables(), sl.tables(fs, taus, batch.cell)
    for name, g, w in zip("a g A A64".split(), got, want):
        assert g.tobytes() == w.tobytes(), name
    a, g = got[:2]
    assert np.all((0 < a) & (a < 1)) and np.allclose(a + g, 1.0, rtol=0, atol=1e-15)


def test_default_cell_and_state_length():
    lib = _lib.load()
    for interval in (16, 480, 4800, 48000, 1 << 20, 4816):
        cell = lib.frt_spl_default_cell(interval)
        assert cell % 16 == 0 and 16 <= cell <= 1024 and interval % cell == 0
        assert all(interval % c for c in range(cell + 16, 401, 16))      # the largest admissible one up to 400
    assert lib.frt_spl_default_cell(4800) == 400 and lib.frt_spl_default_cell(480) == 240
    assert lib.frt_spl_default_cell(100) == 0 and lib.frt_spl_default_cell((1 << 20) + 16) == 0
    assert [lib.frt_spl_state_length(n) for n in range(6)] == [0, 14, 23, 32, 41, 0]
    assert lib.frt_spl_intervals_for(480, 0, 481, 0) == 1 and lib.frt_spl_intervals_for(480, 0, 481, 1) == 2
    assert lib.frt_spl_intervals_for(480, 470, 10, 1) == 1 and lib.frt_spl_intervals_for(480, 470, 9, 0) == 0


def cell_form_within_bar(kind, T):
    w, ref, seq, bar, peak = sl.cached(kind, T, **sl.SEAM)
    got = sl.cell_form(w, sl.SEAM["fs"], sl.SEAM["taus"], sl.SEAM["cell"], sl.SEAM["interval"])
    for name in ("last", "max", "min"):
        print(f"{kind} {T} {name}: cell form {sl.distance(getattr(got, name), getattr(ref, name), peak).max():.2e}, "
              f"sequential {sl.distance(getattr(seq, name), getattr(ref, name), peak).max():.2e}, bar {bar.min():.2e}")
    sl.check_fields(got, ref, bar, peak, w, sl.SEAM["interval"])
    if T <= sl.SEAM["cell"]:
        for name in sl.FIELD_NAMES:
            assert getattr(got, name).tobytes() == getattr(seq, name).tobytes(), name


@pytest.mark.parametrize("kind", sl.SEAM_KINDS)
@pytest.mark.parametrize("T", sl.SEAM_LENGTHS)
def test_cell_form_stays_within_the_bar_on_the_seam_inputs(T, kind):
    cell_form_within_bar(kind, T)


def test_cell_form_stays_within_the_bar_on_the_long_row():
    cell_form_within_bar("long", sl.LONG_LENGTH)


def sorted_percentiles(row, percents):
    v = sorted(row)
    return [v[int(math.floor((len(v) - 1) * (1 - p / 100) + 0.5))] for p in percents] if v else [math.nan] * len(percents)


def test_percentile_levels():
    import torch
    rng = np.random.default_rng(5)
    levels = np.round(rng.normal(60.0, 8.0, (7, 101)))            # rounded: many ties
    levels[3, :40] = -np.inf                                     # silence
    for pct in ((10, 50, 90), (0, 1, 99, 100), (5,)):
        want = np.array([sorted_percentiles(r.tolist(), pct) for r in levels])
        got = soundlevel.percentile_levels(levels, pct)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, want)
        t = soundlevel.percentile_levels(torch.from_numpy(levels), pct)
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and np.array_equal(t.numpy(), want)
        assert np.array_equal(soundlevel.percentile_levels(levels[2], pct), want[2])
    got = soundlevel.percentile_levels(levels[:, :10])
    assert np.all(got[:, 0] >= got[:, 1]) and np.all(got[:, 1] >= got[:, 2])      # L10 >= L50 >= L90
    assert np.array_equal(soundlevel.percentile_levels(np.array([3.0, 1.0, 2.0])), [3.0, 2.0, 1.0])
    for empty in (np.zeros((3, 0)), torch.zeros((3, 0), dtype=torch.float64)):
        got = soundlevel.percentile_levels(empty)
        assert tuple(got.shape) == (3, 3) and bool(np.isnan(np.asarray(got)).all())
    assert np.isnan(soundlevel.percentile_levels(np.zeros(0))).all()
    with pytest.raises(ValueError, match="percents"):
        soundlevel.percentile_levels(levels, (101,))


def test_refusals():
    B = soundlevel.SoundLevelBatch
    for interval in (100, 8, 4808, (1 << 20) + 16, 480.0, True):
        with pytest.raises(ValueError, match="interval"):
            B("Z", interval=interval)
    for cell in (128, 1600, 24, 0, 32.0):                        # 128 does not divide 4800, 1600 is too large
        with pytest.raises(ValueError, match="cell"):
            B("Z", interval=4800, cell=cell)
    for taus in ((), (0.1, 0.2, 0.3, 0.4, 0.5), (0.0,), (-1.0, 1.0), (math.nan,), (1e-9,)):
        with pytest.raises(ValueError, match="time constant"):
            B("Z", taus=taus)
    with pytest.raises(ValueError, match="weighting"):
        B("D")
    with pytest.raises(ValueError, match="fs"):
        B("A", fs=0)
    batch = B("Z", interval=480, cell=32)
    other = B("Z", interval=480, cell=16)
    x = np.zeros((2, 100))
    det = soundlevel.DetectorState(np.zeros((2, batch.state_length)), 2, 10, False, batch.settings)
    state = soundlevel.SoundLevelState((), det)
    with pytest.raises(ValueError, match="settings"):
        batch.run(x, state=state._replace(detector=det._replace(settings=other.settings)))
    with pytest.raises(ValueError, match="final"):
        batch.run(x, state=state._replace(detector=det._replace(final=True)))
    with pytest.raises(ValueError, match="shape"):
        batch.run(x, state=state._replace(detector=det._replace(data=np.zeros((2, batch.state_length + 1)))))
    with pytest.raises(ValueError, match="shape"):
        batch.run(np.zeros((3, 100)), state=state)
    with pytest.raises(ValueError, match="samples"):
        batch.run(np.zeros((2, 0)))
    with pytest.raises(TypeError):
        batch.run(np.zeros((2, 100), np.int16))


def test_library_refuses_what_the_class_refuses():
    lib = _lib.load()
    taus = (ctypes.c_double * 5)(0.125, 1.0, 2.0, 3.0, 4.0)
    zero = (ctypes.c_double * 1)(0.0)
    for fs, t, n, interval, cell, word in [(48000.0, taus, 2, 100, 0, b"interval"), (48000.0, taus, 2, 4800, 128, b"cell"),
                                           (48000.0, taus, 0, 4800, 0, b"time constants"), (48000.0, taus, 5, 4800, 0, b"time constants"),
                                           (48000.0, zero, 1, 4800, 0, b"time constant"), (1.0, taus, 2, 4800, 0, b"fs")]:
        assert lib.frt_spl_tables(fs, t, n, interval, cell, None, None, None, None) == -1
        assert b"frt_spl_tables" in lib.frt_last_error() and word in lib.frt_last_error()
    h = ctypes.c_void_p()
    assert lib.frt_spl_create(ctypes.byref(h), 48000.0, taus, 2, 4800, 128) == -1 and not h.value
