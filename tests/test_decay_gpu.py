"""DecayBatch on the GPU against the numpy restatement of X3 in np.longdouble (tests/decay_helpers.py), and against itself for
everything the definition says does not matter: the other rows of a call, the slab size, a row stride, the input's dtype and
kind.

The bars are X3's, derived for T <= 2^17: a float64 sum of n non-negative terms in any order is within (n - 1) 2^-53 of exact,
1.5e-11 relative on E, about 1.3e-10 dB on L, the C values, level_db, noise_db and dynamic_range: 1e-9 dB.  An error d on
every L moves a fitted slope by at most 3 d / n per sample over a range of at least 10 dB, 4e-11 relative, and the fit's own
sums add about 2e-10: 1e-8 relative on the decay times, Ts, D50 and r2.  peak, onset and truncation are equal.  Device and
reference differ by rounding, so no index decision may sit on an edge: every case asserts on the reference alone that each
crossing of steps 4 and 6 keeps 1e-6 (dB, or relative for the block sums) from its threshold; a seed that does not is
replaced.  Every parity test prints its distances before it asserts.  Inputs and references are made once and shared."""
import ctypes
import functools
import math

import numpy as np
import pytest

import decay_helpers as dh

pytestmark = pytest.mark.gpu

FS = 48000
TL = 512                                    # decay.TILE


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import decay
    assert decay.TILE == TL
    return decay


def host(res):
    """A DecayResult with numpy fields."""
    return type(res)(*[v.cpu().numpy() if hasattr(v, "cpu") else v for v in res])


def same_bits(a, b, fields=dh.FLOATS + dh.INDICES + ("r2", "curve")):
    a, b = host(a), host(b)
    for f in fields:
        u, v = getattr(a, f), getattr(b, f)
        assert (u is None) == (v is None), f
        if u is not None:
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), f


def pick(res, rows):
    """The rows `rows` of a DecayResult with numpy fields."""
    res = host(res)
    return type(res)(*[None if v is None else v[rows] for v in res])


@functools.lru_cache(maxsize=None)
def seam_case(T, rows, f32, block=16, step=0):
    """(x [rows, T], the longdouble references) with the lead-ins 0, TL - 1, TL in turn (those that leave a sample), rt such
    that the decay has fallen 60 dB after half of what the lead-in leaves."""
    leads = [lead for lead in (0, TL - 1, TL) if lead < T]
    x = np.stack([dh.response(T, max(0.5 * (T - leads[i % len(leads)]), 8) / FS, 1000 * T + i, leads[i % len(leads)],
                              dtype=np.float32 if f32 else np.float64) for i in range(rows)])
    refs = dh.restate_rows(x, block=block, curve_step=step, real=np.longdouble)
    dh.check_gaps(refs)
    x.setflags(write=False)
    return x, refs


@pytest.mark.parametrize("T", [TL - 1, TL, TL + 1, 2 * TL + 3, 5 * TL + 17])
def test_parity_at_block_16_on_the_tile_seams(mod, T):
    """The smallest shapes at which the tile seams, the lane seams and the 8-lane block groups can go wrong; a lead-in of
    TL - 1 or TL in a row of TL - 1 .. TL + 1 samples leaves 0 .. 2 samples: the lead-ins that leave none are left out."""
    db = mod.DecayBatch(block=16)
    x, refs = seam_case(T, 3, False)
    dh.compare(host(db.run(x)), refs, f"T {T} float64 x 3")
    x, refs = seam_case(T, 65, True)
    dh.compare(host(db.run(x)), refs, f"T {T} float32 x 65")
    if T > 2 * TL:
        assert any(math.isfinite(r["t30"]) for r in refs) and {r["onset"] // TL for r in refs} >= {0, 1}


@functools.lru_cache(maxsize=None)
def default_case(T, f32):
    x = np.stack([dh.response(T, rt * T / FS, 7 * T + i, lead, dtype=np.float32 if f32 else np.float64)
                  for i, (rt, lead) in enumerate([(0.2, 0), (0.35, 1234), (0.5, 4001)])])
    refs = dh.restate_rows(x, real=np.longdouble)
    dh.check_gaps(refs)
    x.setflags(write=False)
    return x, refs


@pytest.mark.parametrize("T,f32", [(1 << 14, False), (1 << 17, True)])
def test_parity_at_the_defaults(mod, T, f32):
    x, refs = default_case(T, f32)
    assert all(math.isfinite(r["t30"]) and r["truncation"] < T for r in refs)
    dh.compare(host(mod.DecayBatch().run(x)), refs, f"T {T} {'float32' if f32 else 'float64'}")


@functools.lru_cache(maxsize=None)
def short_case(T, rt, seed):
    x = dh.response(T, rt, seed)[None]
    refs = dh.restate_rows(x, real=np.longdouble)
    dh.check_gaps(refs)
    x.setflags(write=False)
    return x, refs


def test_parity_of_short_rows_at_the_defaults(mod):
    """A row whose T30 range is not reached (EDT is), a row shorter than n50 and n80 (C = +inf, D50 = 1) and a row with T < W
    (no block: N0 = 0, noise_db = -inf, dynamic_range NaN)."""
    db = mod.DecayBatch()
    x, refs = short_case(700, 1.0, 11)
    assert math.isnan(refs[0]["t30"]) and math.isfinite(refs[0]["edt"])
    res = host(db.run(x))
    dh.compare(res, refs, "T 700")
    assert np.isnan(res.t30[0]) and np.isfinite(res.edt[0])
    x, refs = short_case(2000, 0.01, 12)
    assert refs[0]["c80"] == math.inf and refs[0]["d50"] == 1
    res = host(db.run(x))
    dh.compare(res, refs, "T 2000")
    assert res.c50[0] == math.inf and res.c80[0] == math.inf and res.d50[0] == 1.0
    x, refs = short_case(300, 0.002, 13)
    res = host(db.run(x))
    dh.compare(res, refs, "T 300")
    assert np.isnan(res.dynamic_range[0]) and res.noise_db[0] == -math.inf and res.truncation[0] == 300


def test_each_truncate_form_and_given_onsets(mod):
    """truncate=None, "auto" and integers (a tile edge, T, and two others), with the onsets found and given; the rows of one
    batch carry different onsets and truncations."""
    T = 4 * TL + 100
    x, auto = seam_case(T, 4, False)
    db = mod.DecayBatch(block=16)
    found = np.array([r["onset"] for r in auto])
    assert len(set(found)) > 1
    given_t1 = np.array([2 * TL, T, found[2] + 700, 3 * TL + 1])
    given_t0 = found + np.array([0, 3, TL, 1])
    assert np.all(given_t0 < given_t1)
    for onset in (None, given_t0):
        for truncate in (None, "auto", given_t1):
            refs = dh.restate_rows(x, onset=onset, truncate=truncate, block=16, real=np.longdouble)
            dh.check_gaps(refs)
            res = host(db.run(x, onset=onset, truncate=truncate))
            dh.compare(res, refs, f"onset {'given' if onset is not None else 'found'}, truncate {truncate if truncate is None or isinstance(truncate, str) else 'given'}")
    assert len({r["truncation"] for r in auto}) > 1


def test_closed_form_row_on_the_device(mod):
    """x[t] = A r^t with alternating signs, rt = 0.0517 s, T = 8192, truncate=None: every decay time is rt within 1e-9."""
    rt = 0.0517
    x, _ = dh.closed_form_row(8192, rt, FS)
    res = host(mod.DecayBatch().run(x, truncate=None))
    for name in ("edt", "t10", "t20", "t30"):
        print(name, float(getattr(res, name)) - rt)
        assert abs(float(getattr(res, name)) - rt) <= 1e-9
    assert (int(res.peak), int(res.onset), int(res.truncation)) == (0, 0, 8192)


def test_dead_rows_between_live_ones(mod):
    T = 2 * TL + 3
    live, refs = seam_case(T, 4, False, step=7)
    x = np.zeros((7, T))
    x[0::2] = live
    x[3, 100], x[5, T - 1] = math.nan, math.inf
    x[3, :50], x[5, :50] = 0.25, -0.25
    db = mod.DecayBatch(block=16)
    res = host(db.run(x, keep=("params", "curve"), curve_step=7))
    for f in dh.FLOATS + ("r2", "curve"):
        assert np.all(np.isnan(getattr(res, f)[1::2])), f
    for f in dh.INDICES:
        assert np.all(getattr(res, f)[1::2] == -1), f
    alone = db.run(live, keep=("params", "curve"), curve_step=7)
    same_bits(pick(res, slice(0, None, 2)), alone)
    dh.compare(host(alone), refs, "the live rows")


def test_bit_identity(mod):
    import torch
    T = 5 * TL + 17
    x, _ = seam_case(T, 65, True)
    db = mod.DecayBatch(block=16)
    kw = dict(keep=("params", "curve"), curve_step=7)
    whole = db.run(x, **kw)
    same_bits(db.run(x[17:18], **kw), pick(whole, slice(17, 18)))                       # a row alone
    same_bits(db.run(x, scratch_bytes=1, **kw), whole)                                   # one row per launch
    same_bits(db.run(x, scratch_bytes=200000, **kw), whole)                              # a few rows per launch
    big = np.zeros((65, T + 11), np.float32)
    big[:, 5:5 + T] = x
    same_bits(db.run(big[:, 5:5 + T], **kw), whole)                                      # a strided view, numpy
    same_bits(db.run(torch.from_numpy(big).cuda()[:, 5:5 + T], **kw), whole)             # read in place on the device
    same_bits(pick(db.run(x[3:4], **kw), 0), db.run(x[3], **kw))                         # [1, T] against [T]
    assert host(db.run(x[3])).edt.shape == () and host(db.run(x[3])).r2.shape == (4,)
    same_bits(db.run(x.astype(np.float64), **kw), whole)                                 # float32 against the same values as float64
    on_device = db.run(torch.from_numpy(np.array(x)).cuda(), **kw)                       # numpy against a CUDA tensor
    assert all(v.is_cuda for v in on_device)
    same_bits(on_device, whole)


@pytest.mark.parametrize("step", [1, 7, 48])
def test_curve(mod, step):
    T = 2 * TL + 3
    x, refs = seam_case(T, 3, False, step=step)
    db = mod.DecayBatch(block=16)
    res = host(db.run(x, keep=("params", "curve"), curve_step=step))
    assert res.curve.shape == (3, -(-T // step)) and res.curve.dtype == np.float64
    dh.compare(res, refs, f"curve at step {step}")
    for i, r in enumerate(refs):
        past = r["onset"] + np.arange(res.curve.shape[1]) * step >= r["truncation"]
        assert past.any() and np.all(np.isnan(res.curve[i][past])) and not np.any(np.isnan(res.curve[i][~past]))
    plain = db.run(x)
    assert plain.curve is None
    same_bits(plain, res, dh.FLOATS + dh.INDICES + ("r2",))


@functools.lru_cache(maxsize=None)
def room_case():
    from friture_amd import decay
    T, rts = 8192, ((0.020, 0.032), (0.028, 0.022))
    centres, edges = decay.band_edges("octave")
    edges, centres = edges[4:6], centres[4:6]                        # the 2 kHz and 4 kHz octaves
    filters = [decay.band_filter(lo, hi, FS) for lo, hi in edges]
    ir = np.zeros((2, T))
    for s in range(2):
        for b, h in enumerate(filters):
            M = (len(h) - 1) // 2
            noise = dh.response(T, rts[s][b], 50 + 2 * s + b, lead=300 + 40 * s, floor_db=-300.0)
            ir[s] += np.convolve(noise, h)[M:M + T]
    broadband = dh.restate_rows(ir, real=np.longdouble)
    bands = []
    for h in filters:
        M = (len(h) - 1) // 2
        y = np.stack([np.convolve(row, h)[M:M + T] for row in ir])
        bands.append(dh.restate_rows(y, onset=[r["onset"] for r in broadband], real=np.longdouble))
    dh.check_gaps(broadband + bands[0] + bands[1])
    ir.setflags(write=False)
    return ir, tuple(map(tuple, edges)), centres, rts, broadband, bands


def test_room_acoustics_against_the_numpy_pipeline(mod):
    """Two responses made of two decaying noises band-limited to the 2 kHz and 4 kHz octaves; the reference: band_filter, a
    float64 convolution, the restatement with the broadband onset.  ConvolveBatch's own bar, 1e-12 max|x| sum|h|, is about
    1e-10 relative on the energy at -35 dB: decay times within 1e-7 relative, C values within 1e-8 dB."""
    ir, edges, centres, rts, broadband, bands = room_case()
    room = mod.room_acoustics(ir, bands=edges)
    assert np.allclose(room.centres, centres, rtol=1e-12)
    dh.compare(host(room.broadband), broadband, "broadband")
    got = host(room.bands)
    assert got.edt.shape == (2, 2) and got.r2.shape == (2, 2, 4) and got.curve is None
    for b in range(2):
        res = pick(got, (slice(None), b))
        dh.compare(res, bands[b], f"band {centres[b]:.0f} Hz", db_bar=1e-8, rel_bar=1e-7)
        for s in range(2):
            print(f"  response {s}, {centres[b]:.0f} Hz: T30 {res.t30[s]:.5f} s, design rt {rts[s][b]:.5f} s")


@functools.lru_cache(maxsize=None)
def front_case():
    ir = np.stack([dh.response(6000, 0.03, 300 + s, lead=100 + 30 * s) for s in range(2)])
    ir.setflags(write=False)
    return ir


def bits_of(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.dtype, a.shape, a.tobytes()


@pytest.mark.parametrize("filters", ["fir", "butterworth"])
def test_room_acoustics_is_its_composition_bit_for_bit(mod, filters):
    """S = 2 responses of T = 6000 samples, two bands: room_acoustics against the calls it stands for, written out.  "fir":
    per band, band_filter, ConvolveBatch(h).run(ir).y[..., M : M + T], DecayBatch.run with the broadband onsets.  "butterworth":
    SosBatch(..).run(fan=True) and one DecayBatch.run on its [S B, T] view with the onsets repeated per band."""
    from friture_amd import convolve, sosfilter
    ir, bands, T = front_case(), [(500, 1000), (1000, 2000)], 6000
    room = mod.room_acoustics(ir, bands=bands, filters=filters)
    db = mod.DecayBatch()
    broadband = db.run(ir)
    same_bits(room.broadband, broadband)
    if filters == "fir":
        per_band = []
        for f_lo, f_hi in bands:
            h = mod.band_filter(f_lo, f_hi, FS)
            M = (len(h) - 1) // 2
            per_band.append(db.run(convolve.ConvolveBatch(h).run(ir).y[..., M:M + T], onset=broadband.onset))
        want = {f: np.stack([getattr(r, f) for r in per_band], 1) for f in dh.FLOATS + dh.INDICES + ("r2",)}
    else:
        sos = np.stack([sosfilter.butter_band_sos(f_lo, f_hi, FS, 3) for f_lo, f_hi in bands])
        y = sosfilter.SosBatch(sos).run(ir, fan=True, dtype="float64").y
        assert y.shape == (2, 2, T)
        res = db.run(y.reshape(4, T), onset=np.repeat(broadband.onset, 2))
        want = {f: getattr(res, f).reshape((2, 2) + getattr(res, f).shape[1:]) for f in dh.FLOATS + dh.INDICES + ("r2",)}
    assert room.bands.curve is None and room.bands.edt.shape == (2, 2) and room.bands.r2.shape == (2, 2, 4)
    assert not np.any(np.isnan(room.bands.t20))
    for f, v in want.items():
        assert bits_of(getattr(room.bands, f)) == bits_of(v), f


@pytest.mark.parametrize("filters", ["fir", "butterworth"])
def test_speech_transmission_is_its_composition_bit_for_bit(mod, filters):
    """The same responses through speech_transmission's seven octaves: MtfBatch.run over [onset, truncation) of the broadband
    DecayBatch.run, on the delayed views per band or on the bank's [S B, T] view, then sti_from_mtf."""
    from friture_amd import convolve, sosfilter, sti
    ir, T = front_case(), 6000
    got = sti.speech_transmission(ir, filters=filters)
    broadband = mod.DecayBatch().run(ir)
    mtf = sti.MtfBatch()
    if filters == "fir":
        per_band = []
        for f_lo, f_hi in sti.octave_bands():
            h = mod.band_filter(f_lo, f_hi, FS)
            M = (len(h) - 1) // 2
            per_band.append(mtf.run(convolve.ConvolveBatch(h).run(ir).y[..., M:M + T], start=broadband.onset, stop=broadband.truncation).m)
        m = np.stack(per_band, 1)
    else:
        sos = np.stack([sosfilter.butter_band_sos(f_lo, f_hi, FS, 3) for f_lo, f_hi in sti.octave_bands()])
        y = sosfilter.SosBatch(sos).run(ir, fan=True, dtype="float64").y
        m = mtf.run(y.reshape(14, T), start=np.repeat(broadband.onset, 7), stop=np.repeat(broadband.truncation, 7)).m.reshape(2, 7, 14)
    assert got.m.shape == (2, 7, 14) and not np.any(np.isnan(got.m)) and bits_of(got.m) == bits_of(m)
    for a, b in zip(got[1:4], sti.sti_from_mtf(m)):
        assert bits_of(a) == bits_of(b)


def test_a_bad_argument_through_the_c_entry_point(mod):
    from friture_amd import _lib
    h = _lib.Handle("decay", 48000.0, 480, -20.0, 0.1, 10.0)
    x = np.ones((2, 64))
    params, idx = np.full((2, 15), 7.0), np.full((2, 3), 7, np.int64)
    vp = ctypes.c_void_p

    def run(rows=2, n=64, dtype=1, stride=64, mode=1, trunc=None, step=0, scratch=1 << 20, curve=None, onset=None):
        return h.lib.frt_decay_run(h.h, vp(x.ctypes.data), dtype, rows, n, stride, onset, mode, trunc, step, scratch, vp(params.ctypes.data),
                                   vp(idx.ctypes.data), curve)

    bad_onset = np.array([0, 64], np.int64)
    for kw in (dict(rows=0), dict(n=0), dict(n=(1 << 24) + 1), dict(dtype=2), dict(stride=63), dict(mode=3), dict(mode=2), dict(step=-1),
               dict(step=4), dict(scratch=-1), dict(onset=vp(bad_onset.ctypes.data))):
        assert run(**kw) == -1, kw
        assert b"frt_decay_run" in h.lib.frt_last_error(), kw
    assert np.all(params == 7.0) and np.all(idx == 7)                # nothing was launched
    with pytest.raises(_lib.FritureHipError, match="frt_decay_create"):
        _lib.Handle("decay", 48000.0, 4, -20.0, 0.1, 10.0)
    assert run() == 0 and not np.any(params == 7.0)
