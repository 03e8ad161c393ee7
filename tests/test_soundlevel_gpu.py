"""SoundLevelBatch on the GPU: the detector against the sequential recurrence in np.longdouble (tests/soundlevel_helpers.py), against
itself for everything X7 says does not matter (how a stream is cut into calls, the other rows, the slab size, a row stride, the
input's dtype and kind), on dead data, against expectations derived from IEC 61672-1's formulas, and the chain against its parts.

The accuracy bar is measured, not fixed: per (row, time constant) e_seq is the distance of the float64 sequential recurrence from
the long double one relative to the row's largest average, and the device must lie within max(64 e_seq, 1e-13) of the long
double one; the energy within 1e-10 interval max w^2; count and peak exactly.  tests/test_soundlevel_cpu.py shows that the float64
numpy restatement of the cell form meets the same bars on the same inputs.  Inputs and references are made once and shared."""
import math

import numpy as np
import pytest

import soundlevel_helpers as sl
from sos_helpers import decaying_noise
from soundlevel_helpers import (DETECTOR_FIELDS, RESULT_FIELDS, as_fields, host, in_pieces, joined, led, pieces_equal_whole, same_bits,
                                same_detector_state, same_result)

pytestmark = pytest.mark.gpu

FS = 48000
SEAM = dict(sl.SEAM)


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import soundlevel
    return soundlevel


@pytest.fixture(scope="module")
def seam(mod):
    return mod.SoundLevelBatch("Z", **SEAM)


# ---- seams --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sl.SEAM_KINDS)
@pytest.mark.parametrize("T", sl.SEAM_LENGTHS)
def test_parity_on_the_seams(seam, T, kind):
    """interval 480, cell 32, taus 2 ms and 20 ms: 3 float64 rows and 65 float32 rows; the lead-ins 0, 1 and 63 in turn."""
    w, ref, seq, bar, peak = sl.cached(kind, T, **SEAM)
    lead = (0, 1, 63)[(sl.SEAM_LENGTHS.index(T) + sl.SEAM_KINDS.index(kind)) % 3]
    d = seam.detect(led(w, lead))
    got = as_fields(d)
    for name in ("last", "max", "min"):
        print(f"{kind} {T} {name}: device {sl.distance(getattr(got, name), getattr(ref, name), peak).max():.2e}, "
              f"sequential {sl.distance(getattr(seq, name), getattr(ref, name), peak).max():.2e}, bar {bar.min():.2e}")
    assert got.energy.dtype == np.float64 and got.count.dtype == np.int64 and got.last.shape == (w.shape[0], -(-T // 480), 2)
    sl.check_fields(got, ref, bar, peak, w, SEAM["interval"])
    assert d.total_count == T and d.state.final and d.state.n == T
    if T <= SEAM["cell"]:                                        # one cell is the sequential recurrence
        for name in sl.FIELD_NAMES:
            same_bits(getattr(got, name), getattr(seq, name))
    # and the restatement of the cell form in float64 is the device, bit for bit
    want = sl.cell_form(w, SEAM["fs"], SEAM["taus"], SEAM["cell"], SEAM["interval"])
    for name in sl.FIELD_NAMES:
        same_bits(getattr(got, name), getattr(want, name))


@pytest.mark.parametrize("flush", [True, False])
def test_parity_on_the_long_row(seam, flush):
    """64 * 64 * 32 + 3 samples at cell 32: 65 runs, so level two of the scan walks; two float64 rows."""
    w, ref, seq, bar, peak = sl.cached("long", sl.LONG_LENGTH, **SEAM)
    d = seam.detect(w, flush=flush)
    got = as_fields(d)
    J = sl.LONG_LENGTH // 480 + int(flush)
    assert got.energy.shape == (2, J) and d.total_count == (sl.LONG_LENGTH if flush else J * 480) and d.state.final == flush
    cut = sl.Fields(*(getattr(ref, n)[:, :J] for n in sl.FIELD_NAMES), ref.count[:J])
    sl.check_fields(got, cut, bar, peak, w, SEAM["interval"])
    if not flush:                                                # the open interval arrives with the next call
        rest = seam.detect(np.zeros((2, 13)), state=d.state)
        assert host(rest.count).tolist() == [sl.LONG_LENGTH % 480 + 13] and rest.total_count == sl.LONG_LENGTH + 13
    else:                                                        # the restatement of the cell form in float64 is the device
        want = sl.cell_form(w, SEAM["fs"], SEAM["taus"], SEAM["cell"], SEAM["interval"])
        for name in sl.FIELD_NAMES:
            same_bits(getattr(got, name), getattr(want, name))


def test_default_settings(mod):
    """interval 4800, the default cell, Fast and Slow: 2 rows of 20000 samples."""
    batch = mod.SoundLevelBatch("Z")
    assert (batch.interval, batch.ntau) == (4800, 2) and batch.cell == mod._lib.load().frt_spl_default_cell(4800)
    w = decaying_noise(2, 20000, 31, rt=1.0)
    a, g, _, _ = batch.tables()
    eld, e64 = sl.sequential(w, a, g, np.longdouble), sl.sequential(w, a, g, np.float64)
    bar, peak = sl.bar(e64, eld)
    got = as_fields(batch.detect(w))
    assert got.count.tolist() == [4800] * 4 + [800]
    sl.check_fields(got, sl.fields(w, eld, 4800), bar, peak, w, 4800)
    want = sl.cell_form(w, FS, (0.125, 1.0), batch.cell, 4800)
    for name in sl.FIELD_NAMES:
        same_bits(getattr(got, name), getattr(want, name))


# ---- bit-identity ---------------------------------------------------------------------------------------------------------------

def test_pieces_give_the_bits_of_the_whole(seam):
    w = sl.cached("f64x3", 2049, **SEAM)[0]
    whole, state = pieces_equal_whole(seam, w, (1, 31, 32, 33, 480, 1000))
    same_detector_state(state, whole.state)
    pieces_equal_whole(seam, w[:, :100], range(1, 100))           # one-sample pieces
    long = sl.cached("long", sl.LONG_LENGTH, **SEAM)[0]                   # and cut inside the second level's runs
    pieces_equal_whole(seam, long, (64 * 32 * 3 + 5, 2049 * 50, 64 * 32 * 64, 64 * 32 * 64 + 1))


def test_what_does_not_matter(seam, mod):
    import torch
    w = sl.cached("f32x65", 2049, **SEAM)[0]
    whole = seam.detect(w)
    per_row = 8 * (2 * (2 * 66 + 2 * 3) + 8 * 66)                 # a little more than one row's scratch: one row per launch
    same_result(seam.detect(w, scratch_bytes=per_row), whole)
    same_result(seam.detect(w, scratch_bytes=0), whole)
    same_result(seam.detect(w, scratch_bytes=3 * per_row), whole)
    alone = seam.detect(w[7:8])
    for name in DETECTOR_FIELDS:
        if name != "count":
            same_bits(getattr(alone, name), getattr(whole, name)[7:8])
    flat = seam.detect(w[7])                                      # [T]: no row axis
    for name in DETECTOR_FIELDS:
        if name != "count":
            same_bits(getattr(flat, name), getattr(whole, name)[7])
    wide = np.zeros((65, 2049 + 77), np.float32)
    wide[:, 5:5 + 2049] = w
    same_result(seam.detect(wide[:, 5:5 + 2049]), whole)          # a strided view, read in place
    same_result(seam.detect(w.astype(np.float64)), whole)         # float32 widens exactly
    dev = seam.detect(torch.from_numpy(w).cuda())
    assert dev.energy.is_cuda and dev.count.is_cuda and dev.state.data.is_cuda
    same_result(dev, whole)
    same_detector_state(dev.state._replace(data=host(dev.state.data)), whole.state)
    dwide = torch.from_numpy(wide).cuda()
    same_result(seam.detect(dwide[:, 5:5 + 2049]), whole)
    parts, state = in_pieces(seam, torch.from_numpy(w).cuda(), (33, 1000))
    same_bits(joined(parts, "max"), whole.max)
    same_bits(state.data, whole.state.data)
    same_result(mod.SoundLevelBatch("Z", **SEAM).detect(w), whole)        # another handle


def test_z_run_is_the_detector_in_decibels(seam, mod):
    w = sl.cached("f64x3", 2049, **SEAM)[0]
    d, r = seam.detect(w), seam.run(w)
    with np.errstate(divide="ignore"):
        same_bits(r.leq, 10 * np.log10(d.energy / d.count))
        same_bits(r.level, 10 * np.log10(d.last))
        same_bits(r.lmax, 10 * np.log10(d.max))
        same_bits(r.lmin, 10 * np.log10(d.min))
        same_bits(r.peak_db, 20 * np.log10(d.peak))
        same_bits(r.total_leq, 10 * np.log10(d.total_energy / 2049))
        same_bits(r.sel, 10 * np.log10(d.total_energy / FS))
        same_bits(r.total_lmax, 10 * np.log10(d.max.max(axis=1)))
        same_bits(r.total_lmin, 10 * np.log10(d.min.min(axis=1)))
        same_bits(r.total_peak_db, 20 * np.log10(d.peak.max(axis=1)))
    same_bits(r.energy, d.energy)
    total = np.zeros(3)
    for j in range(d.energy.shape[1]):                           # the intervals' energies in ascending order
        total = total + d.energy[:, j]
    same_bits(d.total_energy, total)
    cal = mod.SoundLevelBatch("Z", cal_db=94.0, **SEAM).run(w)
    same_bits(cal.leq, r.leq + 94.0)
    same_bits(cal.sel, r.sel + 94.0)
    one = mod.sound_levels(w, "Z", **SEAM)
    same_result(one, r)


# ---- dead data --------------------------------------------------------------------------------------------------------------------

def test_zero_rows_and_a_nan(seam):
    w = sl.cached("f64x3", 2049, **SEAM)[0]
    clean = seam.detect(w)
    bad = w.copy()
    bad[0] = 0.0
    bad[1, 700] = np.nan
    d = seam.detect(bad)
    for name in ("energy", "peak", "last", "max", "min", "total_energy", "total_peak", "total_max", "total_min"):
        assert not host(getattr(d, name))[0].any(), name          # exact zeros
        same_bits(getattr(d, name)[2], getattr(clean, name)[2])   # the neighbour keeps its bits
    r = seam.run(bad)
    for name in ("leq", "lmax", "lmin", "level", "peak_db", "total_leq", "sel", "total_lmax", "total_lmin", "total_peak_db"):
        assert np.all(host(getattr(r, name))[0] == -np.inf), name
    for name in ("energy", "peak", "last", "max", "min"):
        same_bits(getattr(d, name)[1, :1], getattr(clean, name)[1, :1])      # the interval before the NaN
    for name in ("last", "max", "min"):
        assert np.isnan(getattr(d, name)[1, 1:]).all(), name
    for name in ("energy", "peak"):
        assert np.isnan(getattr(d, name)[1, 1]), name
        same_bits(getattr(d, name)[1, 2:], getattr(clean, name)[1, 2:])
    assert np.isnan(d.total_energy[1]) and np.isnan(d.total_peak[1]) and np.isnan(d.total_max[1]).all()
    # and in pieces, the NaN's cell cut in two
    parts, _ = in_pieces(seam, bad, (690, 701, 1000))
    for name in ("energy", "peak", "last", "max", "min"):
        same_bits(joined(parts, name), getattr(d, name))


# ---- the instrument ---------------------------------------------------------------------------------------------------------------

def test_a_weighted_sine_at_1_khz(mod):
    """Amplitude 1 for 2 s: every interval from 1 s on has leq = 10 log10(0.5) within 1e-6 dB (100 whole cycles per interval; the
    20.6 Hz poles' transient is below e^-100 by then), and the Fast level within 0.01 dB of it (its ripple at 2 kHz is 1 / (4 pi
    1000 0.125) relative, 0.003 dB)."""
    x = np.sin(2 * np.pi * 1000.0 * np.arange(2 * FS) / FS)
    r = mod.SoundLevelBatch("A").run(x)
    want = 10 * math.log10(0.5)
    assert r.leq.shape == (20,) and r.level.shape == (20, 2)
    print("leq - want:", np.abs(r.leq[10:] - want).max(), "fast - want:", np.abs(r.level[10:, 0] - want).max())
    assert np.abs(r.leq[10:] - want).max() < 1e-6
    assert np.abs(r.level[10:, 0] - want).max() < 0.01


def test_tone_burst_responses(mod):
    """A 4 kHz burst of 200 ms in silence, Z: the maximum of the Fast and Slow levels is the reference tone-burst response
    10 log10(0.5 (1 - exp(-0.2 / tau))) of IEC 61672-1 within 0.01 dB (the ripple term is below 0.002 dB), the sound exposure
    level is 10 log10(0.5 0.2) within 1e-9 dB."""
    x = np.zeros(FS)
    n = np.arange(9600)
    x[4800 * 3:4800 * 3 + 9600] = np.sin(2 * np.pi * 4000.0 * n / FS)
    r = mod.SoundLevelBatch("Z").run(x.astype(np.float64))
    fast, slow = (10 * math.log10(0.5 * (1 - math.exp(-0.2 / tau))) for tau in (0.125, 1.0))
    print("fast", r.total_lmax[0] - fast, "slow", r.total_lmax[1] - slow, "sel", r.sel - 10 * math.log10(0.1))
    assert abs(r.total_lmax[0] - fast) < 0.01
    assert abs(r.total_lmax[1] - slow) < 0.01
    assert abs(r.sel - 10 * math.log10(0.5 * 0.2)) < 1e-9
    assert r.total_peak_db <= 0.0 and r.total_lmin[0] == -np.inf


# ---- the chain ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain_input():
    return decaying_noise(2, 6000, 41, rt=1.0, dtype=np.float32)


def test_a_chain_is_its_parts(mod, chain_input):
    """weighting="A": SosBatch(weighting_sos("A")).run in float64, then the Z-weighted batch on its output."""
    from friture_amd import sosfilter
    x = chain_input
    kw = dict(interval=480, taus=(0.002, 0.125))
    r = mod.SoundLevelBatch("A", **kw).run(x)
    y = sosfilter.SosBatch(mod.weighting_sos("A")).run(x, dtype=np.float64).y
    same_result(r, mod.SoundLevelBatch("Z", **kw).run(y))
    assert r.leq.shape == (2, 13) and r.lmax.shape == (2, 13, 2) and r.sel.shape == (2,) and r.total_lmax.shape == (2, 2)
    c = mod.SoundLevelBatch("C", **kw).run(x)
    same_result(c, mod.SoundLevelBatch("Z", **kw).run(sosfilter.SosBatch(mod.weighting_sos("C")).run(x, dtype=np.float64).y))


def test_a_band_chain_is_its_parts_and_its_pieces(mod, chain_input):
    import torch
    from friture_amd import sosfilter
    x = chain_input
    kw = dict(interval=480, taus=(0.002, 0.125))
    batch = mod.SoundLevelBatch("A", bands="octave", **kw)
    r = batch.run(x)
    y = sosfilter.SosBatch(mod.weighting_sos("A")).run(x, dtype=np.float64).y
    fan = sosfilter.SosBatch(sosfilter.band_sos("octave", FS, 3)[1]).run(y, fan=True).y
    assert fan.shape == (2, 6, 6000) and len(batch.centres) == 6
    z = mod.SoundLevelBatch("Z", **kw).run(fan.reshape(12, 6000))
    assert r.leq.shape == (2, 6, 13) and r.level.shape == (2, 6, 13, 2) and r.sel.shape == (2, 6) and r.total_lmin.shape == (2, 6, 2)
    for name in RESULT_FIELDS:
        v = host(getattr(z, name))
        same_bits(getattr(r, name), v if name == "count" else v.reshape((2, 6) + v.shape[1:]))
    one = batch.run(x[0])                                        # [T]: the band axis leads
    assert one.leq.shape == (6, 13)
    same_bits(one.lmax, r.lmax[0])
    # pieces, both states carried, on the host and on the device
    for xx in (x, torch.from_numpy(x).cuda()):
        whole = batch.run(xx)                                    # the decibels are the kind's own log10: compared within a kind
        parts, state = in_pieces(batch, xx, (100, 481, 2049), method="run")
        for name in ("leq", "lmax", "lmin", "level", "peak_db", "energy", "peak", "count"):
            same_bits(joined(parts, name), getattr(whole, name))
        for name in RESULT_FIELDS[8:]:
            same_bits(getattr(parts[-1], name), getattr(whole, name))
        for name in ("energy", "peak", "count"):                 # the linear values have the same bits in both kinds
            same_bits(getattr(whole, name), getattr(r, name))
        np.testing.assert_allclose(host(whole.leq), r.leq, rtol=0, atol=1e-12)
        assert len(state.filters) == 2 and state.detector.final and state.detector.n == 6000
    with pytest.raises(ValueError, match="final"):
        batch.run(x, state=state)


def test_a_bad_argument_through_the_c_entry_point(seam, hip):
    import ctypes
    h = seam._handle()
    x = np.zeros((2, 100))
    vp = ctypes.c_void_p
    for rows, n, stride, n_before, flush, word in [(0, 100, 100, 0, 1, b"rows"), (2, 0, 100, 0, 1, b"bad input"), (2, 100, 99, 0, 1, b"stride"),
                                                   (2, 100, 100, 5, 1, b"n_before"), (2, 100, 100, 0, 2, b"flush")]:
        assert hip.frt_spl_run(h.h, vp(x.ctypes.data), 1, rows, n, stride, n_before, None, None, flush, 0, None, None, None) == -1
        assert b"frt_spl_run" in hip.frt_last_error() and word in hip.frt_last_error()
    assert hip.frt_spl_run(h.h, vp(x.ctypes.data), 1, 2, 100, 100, 0, None, None, 1, 0, None, None, None) == -1      # J = 1, no outputs
    assert b"null output" in hip.frt_last_error()
