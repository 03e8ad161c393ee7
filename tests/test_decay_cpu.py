"""DecayBatch without a GPU: the numpy restatement (tests/decay_helpers.py) against a closed form, the band front's host
design (band_edges, band_filter), the argument checks of run() that come before the library, and the binding table."""
import math

import numpy as np
import pytest

import decay_helpers as dh
from friture_amd import _lib, convolve, decay

FS = 48000


@pytest.mark.parametrize("real", [np.float64, np.longdouble])
def test_restatement_gives_the_closed_form_of_an_exponential(real):
    """x[t] = A r^t with alternating signs, truncate=None: L[t] = -60 t / (rt fs) up to r^(2 (T - t)), so every decay time is
    rt, C50 = 10 log10((1 - r^(2 n50)) / r^(2 n50)) and Ts = r^2 / (1 - r^2) / fs.  The crossings are checked to lie off the
    sample grid, all but one: with rt = 0.0517 s the -25 dB crossing is sample 25 rt fs / 60 = 1034 exactly, so rounding decides
    whether T20's range ends at 1034 or 1035; on a straight line the slope is the same either way, and this test asserts no
    index there."""
    rt = 0.0517
    x, r = dh.closed_form_row(8192, rt, FS)
    ref = dh.restate(x, truncate=None, real=real)
    assert sorted(ref["gap_at"]) == [-35.0, -25.0, -15.0, -10.0, -5.0]
    assert all(gap >= 1e-6 for level, gap in ref["gap_at"].items() if level != -25.0), ref["gap_at"]
    assert 25 * rt * FS / 60 == 1034.0
    assert (ref["peak"], ref["onset"], ref["truncation"]) == (0, 0, 8192)
    for name in ("edt", "t10", "t20", "t30"):
        print(name, float(ref[name]) - rt)
        assert abs(float(ref[name]) - rt) <= 1e-9
    assert np.all(np.abs(ref["r2"] - 1) <= 1e-12)
    n50 = 2400
    assert abs(float(ref["c50"]) - 10 * math.log10((1 - r ** (2 * n50)) / r ** (2 * n50))) <= 1e-9
    assert abs(float(ref["ts"]) - r * r / (1 - r * r) / FS) <= 1e-9 * r * r / (1 - r * r) / FS
    assert abs(float(ref["d50"]) - (1 - r ** (2 * n50))) <= 1e-12


def test_restatement_float64_against_longdouble_and_its_edges():
    x = dh.response(1 << 14, 0.08, 3, lead=100)
    a, b = dh.restate(x, curve_step=48), dh.restate(x, curve_step=48, real=np.longdouble)
    dh.check_gaps([b])
    for f in dh.INDICES:
        assert a[f] == b[f]
    assert max(dh.db_distance(a[f], b[f]) for f in dh.DB_FIELDS) <= 1e-11
    assert max(dh.rel_distance(a[f], b[f]) for f in dh.REL_FIELDS) <= 1e-11
    assert dh.db_distance(a["curve"], b["curve"]) <= 1e-11 and np.isnan(a["curve"][-1]) and a["curve"][0] == 0
    dead = dh.restate(np.zeros(100))
    assert dead["peak"] == -1 and math.isnan(dead["edt"])
    short = dh.restate(dh.response(2000, 0.01, 5))                   # shorter than n50
    assert short["c50"] == math.inf and short["c80"] == math.inf and short["d50"] == 1
    tiny = dh.restate(dh.response(300, 0.01, 5))                     # T < W
    assert math.isnan(tiny["dynamic_range"]) and tiny["noise_db"] == -math.inf and tiny["truncation"] == 300


def test_band_edges_are_the_base_ten_series():
    fm, edges = decay.band_edges("octave")
    assert fm.shape == (6,) and edges.shape == (6, 2) and fm[3] == 1000.0
    assert np.allclose(fm, [125.89254, 251.18864, 501.18723, 1000.0, 1995.26231, 3981.07171], rtol=1e-7)
    assert np.allclose(edges[0], [10 ** 1.95, 10 ** 2.25], rtol=1e-12)          # the 125 Hz octave: 89.125 .. 177.83 Hz
    fm3, edges3 = decay.band_edges("third")
    assert fm3.shape == (18,) and fm3[10] == 1000.0
    assert np.allclose(fm3[0], 100.0, rtol=1e-12) and np.allclose(fm3[-1], 10 ** 3.7, rtol=1e-12)
    assert np.allclose(edges3[0], [10 ** 1.95, 10 ** 2.05], rtol=1e-12)         # the 100 Hz third octave: 89.125 .. 112.20 Hz
    fmp, edgesp = decay.band_edges([(100.0, 400.0)])
    assert fmp[0] == 200.0 and edgesp.tolist() == [[100.0, 400.0]]
    for bad in ("fifth", [(400.0, 100.0)], [1.0, 2.0]):
        with pytest.raises(ValueError):
            decay.band_edges(bad)


@pytest.mark.parametrize("f_lo,f_hi,att", [(10 ** 3.15, 10 ** 3.45, 60.0), (10 ** 1.95, 10 ** 2.25, 60.0), (10 ** 2.95, 10 ** 3.05, 80.0)])
def test_band_filter_meets_its_design(f_lo, f_hi, att):
    h = decay.band_filter(f_lo, f_hi, FS, attenuation_db=att)
    assert h.dtype == np.float64 and len(h) % 2 == 1 and np.array_equal(h, h[::-1])
    n = 1 << (len(h) * 8).bit_length()
    H = 20 * np.log10(np.maximum(np.abs(np.fft.rfft(h, n)), 1e-300))
    f = np.arange(n // 2 + 1) * FS / n
    tw = 0.25 * (f_hi - f_lo)
    stop = (f <= f_lo - tw / 2) | (f >= f_hi + tw / 2)
    centre = np.argmin(np.abs(f - math.sqrt(f_lo * f_hi)))
    print(f"{f_lo:.1f} .. {f_hi:.1f} Hz: {len(h)} taps, stop band {H[stop].max():.2f} dB, centre {H[centre]:.5f} dB")
    assert H[stop].max() <= -att
    assert abs(H[centre]) <= 0.1


def test_band_filter_refuses_what_convolve_cannot_take():
    with pytest.raises(ValueError, match="taps"):
        decay.band_filter(20.0, 20.5, FS)
    assert len(decay.band_filter(10 ** 1.95, 10 ** 2.05, FS)) <= convolve.MAX_TAPS       # the narrowest third octave fits
    for bad in ((0.0, 100.0), (200.0, 100.0), (1000.0, 24000.0)):
        with pytest.raises(ValueError):
            decay.band_filter(*bad, FS)


def test_arguments_are_checked_before_the_library():
    for bad in (7, 65537, True, 480.0):
        with pytest.raises(ValueError, match="block"):
            decay.DecayBatch(block=bad)
    for kw in ({"fs": 0}, {"onset_db": 3.0}, {"noise_tail": 0.0}, {"noise_tail": 1.5}, {"margin_db": -1.0}, {"fs": math.nan}):
        with pytest.raises(ValueError):
            decay.DecayBatch(**kw)
    db = decay.DecayBatch()
    x = np.zeros((3, 1000), np.float32)
    with pytest.raises(TypeError):
        db.run([[0.0] * 10])
    with pytest.raises(TypeError):
        db.run(x.astype(np.int32))
    with pytest.raises(ValueError):
        db.run(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="samples"):
        db.run(np.zeros((2, 0)))
    with pytest.raises(ValueError, match="samples"):
        db.run(np.broadcast_to(np.float32(0), (decay.MAX_SAMPLES + 1,)))
    for onset in ([0, 1], [0, 1, 1000], [0, -1, 2], [0.0, 1.0, 2.0]):
        with pytest.raises(ValueError, match="onset"):
            db.run(x, onset=onset)
    for truncate in ("lundeby", [1, 2], [1, 2, 1001], [0, 5, 5], [1.5, 2.0, 3.0]):
        with pytest.raises(ValueError, match="truncate"):
            db.run(x, truncate=truncate)
    with pytest.raises(ValueError, match="truncate"):
        db.run(x, onset=[5, 5, 5], truncate=[6, 5, 6])
    for keep in (("curve",), "params", ("params", "lines")):
        with pytest.raises(ValueError, match="keep"):
            db.run(x, keep=keep)
    for step in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="curve_step"):
            db.run(x, keep=("params", "curve"), curve_step=step)
    with pytest.raises(ValueError, match="scratch_bytes"):
        db.run(x, scratch_bytes=-1)


def test_row_integers_of_the_row_chains():
    """_batchio.row_integers, which DecayBatch (onset, truncate) and MtfBatch (start, stop) share, at R = 3."""
    from friture_amd import _batchio
    v = _batchio.row_integers("onset", [0, 5, 999], 3, 0, 999)
    assert v.dtype == np.int64 and v.shape == (3,) and v.flags.c_contiguous and v.tolist() == [0, 5, 999]
    assert _batchio.row_integers("stop", np.int32(7), 3, 1, 1000, device=True).tolist() == [7, 7, 7]       # shape (): every row
    for bad in ([0.0, 1.0, 2.0], np.float32(1), [0, 1], [[0, 1, 2]]):
        with pytest.raises(ValueError, match=r"onset must be integers \[3\], got "):
            _batchio.row_integers("onset", bad, 3, 0, 999)
    with pytest.raises(ValueError, match=r"onset must lie in 0 \.\. 999, got -1 \.\. 2"):
        _batchio.row_integers("onset", [0, -1, 2], 3, 0, 999)
    with pytest.raises(ValueError, match=r"truncate must lie in 1 \.\. 1000, got 1 \.\. 1001"):
        _batchio.row_integers("truncate", [1, 2, 1001], 3, 1, 1000)


@pytest.mark.parametrize("filters", decay.FILTERS)
def test_band_axis_is_the_way_back_from_the_band_front(filters):
    """Numpy stand-ins for what a consumer made of band_front's pairs, S = 2, B = 3: one result [S, ..] per band of "fir", one
    [S B, ..] of the bank, response-major.  Entry (s, b) comes back at [s, b]."""
    S, B = 2, 3
    flat, r2 = np.arange(S * B, dtype=np.float64), np.arange(S * B * 4, dtype=np.float64).reshape(S * B, 4)
    if filters == "fir":
        made = lambda v, lead: [v.reshape(lead + (B,) + v.shape[1:]).take(b, len(lead)) for b in range(B)]
    else:
        made = lambda v, lead: [v]
    ir = np.zeros((S, 100))
    got, got_r2 = decay.band_axis(ir, B, filters, made(flat, (S,))), decay.band_axis(ir, B, filters, made(r2, (S,)))
    assert got.shape == (2, 3) and np.array_equal(got, flat.reshape(2, 3))
    assert got_r2.shape == (2, 3, 4) and np.array_equal(got_r2, r2.reshape(2, 3, 4))
    one = decay.band_axis(ir[0], B, filters, made(flat[:B], ()))
    assert one.shape == (3,) and np.array_equal(one, flat[:B])


def test_binding_table_lists_the_entry_points():
    names = {n for n in _lib.SIGNATURES if n.startswith("frt_decay_")}
    assert names == {"frt_decay_tile", "frt_decay_create", "frt_decay_destroy", "frt_decay_set_stream", "frt_decay_run"}
    assert _lib.load().frt_decay_tile() == decay.TILE
