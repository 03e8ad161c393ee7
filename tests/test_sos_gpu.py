"""SosBatch on the GPU against the sequential recurrence in np.longdouble (tests/sos_helpers.py), and against itself for
everything X6 says does not matter: how a stream is cut into calls, the other rows of a call, the slab size, a row stride, the
input's dtype and kind, the handle.

The accuracy bar is measured, not fixed: per output row e_seq is the distance of the float64 sequential filter from the long
double one relative to the row's max |y|, on the test's own input, and the device must lie within max(64 e_seq, 1e-13) of the
long double one (a cell's start state goes through a 2K x 2K product where the sequential filter takes `cell` steps, so it
rounds in other places).  tests/test_sos_cpu.py shows that the float64 numpy restatement of the cell form meets the same bar on
the same inputs.  Every parity test prints its distances before it asserts.  Inputs and references are made once and shared."""
import ctypes
import functools

import numpy as np
import pytest

import decay_helpers as dh
import sos_helpers as sh
import sti_helpers
from sos_helpers import host, led, parity, run_pieces, same_bits, same_state

pytestmark = pytest.mark.gpu

FS = 48000
S = sh.SEAM_CELL


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import sosfilter
    return sosfilter


def float32_bar(y, name, args):
    """A float32 output is the one rounding of the float64 value: within 2^-24 relative of each value plus the float64 bar."""
    x, sos, fan, yld, y64 = sh.cached(name, *args)
    want = yld.astype(np.float64)
    y = host(y).astype(np.float64).reshape(want.shape)
    slack = sh.bar(y64, yld)[:, None] * np.abs(want).max(axis=1, keepdims=True)
    assert np.all(np.abs(y - want) <= 2.0 ** -24 * np.abs(want) + slack)


@pytest.mark.parametrize("kind", sh.SEAM_KINDS)
@pytest.mark.parametrize("T", sh.SEAM_LENGTHS)
def test_parity_on_the_seams_at_cell_32(mod, T, kind):
    """K = 3 in bank mode with F = 6 on 3 float64 rows; K = 1 with one filter for 65 float32 rows; K = 8 with one filter per row;
    K = 3 with F = 3 over 7 float32 rows; the lead-ins 0, 1 and 63 in turn."""
    x, sos, fan, yld, y64 = sh.cached("seam", T, kind)
    lead = (0, 1, 63)[(sh.SEAM_LENGTHS.index(T) + sh.SEAM_KINDS.index(kind)) % 3]
    res = mod.SosBatch(sos, cell=S).run(led(x, lead), fan=fan, dtype=np.float64)
    assert res.y.dtype == np.float64 and res.y.shape == ((x.shape[0], len(sos), T) if fan else x.shape)
    parity(res.y, "seam", (T, kind), f"T {T} {kind} lead {lead}")
    if T <= S:                                                   # one cell is the sequential filter
        same_bits(res.y.reshape(y64.shape), y64)
    if x.dtype == np.float32:
        y32 = mod.SosBatch(sos, cell=S).run(x, fan=fan).y
        assert y32.dtype == np.float32
        same_bits(y32, res.y.astype(np.float32))
        float32_bar(y32, "seam", (T, kind))


def test_parity_on_the_long_row(mod):
    """64 * 64 * 32 + 3 samples at cell 32: 65 runs, so level two of the scan walks; bank mode, F = 6, 3 float64 rows."""
    args = (sh.LONG_LENGTH, "bank6")
    x, sos, fan, yld, y64 = sh.cached("seam", *args)
    batch = mod.SosBatch(sos, cell=S)
    whole = batch.run(x, fan=True)
    parity(whole.y, "seam", args, "the long row")
    # and in pieces cut inside the second level's runs
    cuts = [0, 64 * S * 3 + 5, 64 * S * 64, 64 * S * 64 + 1, sh.LONG_LENGTH]
    state, parts = None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = batch.run(x[:, a:b], fan=True, state=state)
        state = r.state
        parts.append(r.y)
    same_bits(np.concatenate(parts, axis=-1), whole.y)
    same_state(state, whole.state)


@pytest.mark.parametrize("bands", ["octave", "third"])
def test_parity_at_the_default_cell(mod, hip, bands):
    x, sos, fan, yld, y64 = sh.cached("bank", bands)
    batch = mod.SosBatch(sos)
    assert batch.cell == hip.frt_sos_default_cell() == 256
    parity(batch.run(x, fan=True).y, "bank", (bands,), f"{bands} bank, order 3, 2^14 samples, cell {batch.cell}")


@pytest.mark.parametrize("cell", [32, 256, 1024])
def test_one_cell_is_the_sequential_filter(mod, cell):
    rng = np.random.default_rng(cell)
    x = rng.standard_normal((5, cell))
    _, sos = mod.band_sos("octave", FS, 3)
    y = mod.SosBatch(sos, cell=cell).run(x, fan=True).y
    same_bits(y.reshape(30, cell), sh.sequential(x, sos, True))
    try:
        from scipy.signal import sosfilt
    except ImportError:
        return
    for f in range(6):
        same_bits(y[:, f], sosfilt(sos[f], x, axis=-1))


@pytest.mark.parametrize("fan", [True, False])
def test_reverse_is_the_flipped_forward_run(mod, fan):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4, 64 * S + 77))
    batch = mod.SosBatch(mod.band_sos("octave", FS, 3)[1][:4], cell=S)
    back = batch.run(x, fan=fan, reverse=True)
    assert back.state is None
    forward = batch.run(np.ascontiguousarray(x[:, ::-1]), fan=fan).y
    same_bits(back.y, forward[..., ::-1])
    t = __import__("torch")
    same_bits(batch.run(t.from_numpy(x).cuda(), fan=fan, reverse=True).y, back.y)


@pytest.mark.parametrize("fan", [True, False])
def test_pieces_give_the_bits_of_the_whole(mod, fan):
    rng = np.random.default_rng(9)
    T = 64 * S * 2 + 2 * S + 5
    x = rng.standard_normal((3, T))
    batch = mod.SosBatch(mod.band_sos("third", FS, 3)[1][[2, 9, 16]], cell=S)
    whole = batch.run(x, fan=fan)
    for cut in (1, S - 1, S, S + 1, 64 * S, 64 * S + 1):
        y, state = run_pieces(batch, x, [cut], fan)
        same_bits(y, whole.y)
        same_state(state, whole.state)
    # one-sample pieces across a cell seam and across a run seam
    for seam in (S, 64 * S):
        y, state = run_pieces(batch, x, list(range(seam - 3, seam + 4)), fan)
        same_bits(y, whole.y)
        same_state(state, whole.state)
    cuts = np.sort(np.random.default_rng(10).choice(np.arange(1, T), 12, replace=False))
    y, state = run_pieces(batch, x, cuts.tolist(), fan)
    same_bits(y, whole.y)
    same_state(state, whole.state)
    # a state from numpy continues a CUDA stream, and an empty piece changes nothing
    t = __import__("torch")
    first = batch.run(x[:, :777], fan=fan)
    empty = batch.run(x[:, :0], fan=fan, state=first.state)
    assert empty.y.shape[-1] == 0 and empty.state is first.state
    rest = batch.run(t.from_numpy(x[:, 777:]).cuda(), fan=fan, state=first.state)
    same_bits(np.concatenate([first.y, host(rest.y)], axis=-1), whole.y)
    same_bits(rest.state.data, whole.state.data)


def test_what_does_not_matter(mod):
    t = __import__("torch")
    rng = np.random.default_rng(12)
    T = 64 * S + 300
    x = rng.standard_normal((5, T)).astype(np.float32)
    sos = mod.band_sos("octave", FS, 3)[1]
    batch = mod.SosBatch(sos, cell=S)
    for fan in (True, False):
        whole = batch.run(x, fan=fan, dtype=np.float64)
        for r in (0, 3):                                         # a row alone (row mode: with its own filter in front)
            alone = mod.SosBatch(sos if fan else sos[[r]], cell=S).run(x[r], fan=fan, dtype=np.float64)
            same_bits(alone.y, whole.y[r])
            same_bits(mod.SosBatch(sos if fan else sos[[r]], cell=S).run(x[r:r + 1], fan=fan, dtype=np.float64).y[0], alone.y)
        one = batch.run(x, fan=fan, dtype=np.float64, scratch_bytes=1)
        same_bits(one.y, whole.y)
        same_state(one.state, whole.state)
        wide = np.zeros((5, 2 * T + 3), np.float32)
        wide[:, 3:T + 3] = x
        same_bits(batch.run(wide[:, 3:T + 3], fan=fan, dtype=np.float64).y, whole.y)
        dev = t.from_numpy(wide).cuda()[:, 3:T + 3]
        assert not dev.is_contiguous()
        on_device = batch.run(dev, fan=fan, dtype=t.float64)
        assert on_device.y.is_cuda and on_device.state.data.is_cuda
        same_bits(on_device.y, whole.y)
        same_state(on_device.state._replace(data=host(on_device.state.data)), whole.state)
        same_bits(batch.run(x.astype(np.float64), fan=fan).y, whole.y)
        same_bits(mod.SosBatch(sos, cell=S).run(x, fan=fan, dtype=np.float64).y, whole.y)          # a second handle
        same_bits(mod.sosfilt(x, sos, cell=S, fan=fan, dtype=np.float64), whole.y)
        out = np.full(whole.y.shape, 7.0)
        assert batch.run(x, fan=fan, dtype=np.float64, out=out).y is out
        same_bits(out, whole.y)


def test_zero_rows_and_rows_that_are_not_finite(mod):
    rng = np.random.default_rng(13)
    T, at = 64 * S + 40, 3 * S + 7
    x = rng.standard_normal((6, T))
    sos = mod.band_sos("octave", FS, 3)[1][:3]
    batch = mod.SosBatch(sos, cell=S)
    for fan in (True, False):
        clean = batch.run(x, fan=fan).y
        bad = x.copy()
        bad[1] = 0.0
        bad[2, at] = np.nan
        bad[4, at] = np.inf
        y = batch.run(bad, fan=fan).y
        assert np.all(y[1] == 0)
        for r in (2, 4):
            same_bits(y[r][..., :at], clean[r][..., :at])
            assert not np.any(np.isfinite(y[r][..., at:]))
            assert np.all(np.isnan(y[r][..., at + 1:]))          # b1 = 0 in a band-pass: 0 * inf, one sample on
        assert np.all(np.isnan(y[2][..., at]))
        for r in (0, 3, 5):
            same_bits(y[r], clean[r])


def test_far_positions(mod):
    """T = 2^20, unit samples at 0 and at T - 300 through the order-3 125 Hz octave: the last 300 outputs against the closed-form
    impulse response (the first impulse's own response has long underflowed there).  The bar is the parity bar, relative to the
    response's peak, with e_seq measured on the float64 sequential response to a unit sample over the same 300 samples."""
    T, n = 1 << 20, 300
    sos = mod.band_sos("octave", FS, 3)[1][0]
    x = np.zeros(T, np.float32)
    x[0] = x[T - n] = 1.0
    y = mod.SosBatch(sos).run(x, dtype=np.float64).y
    h = sh.impulse_response(sos, 8192)
    peak = np.abs(h).max()
    unit = np.zeros((1, n))
    unit[0, 0] = 1.0
    e_seq = float(np.abs(sh.sequential(unit, sos)[0] - h[:n]).max() / peak)
    d = float(np.abs(y[T - n:] - h[:n]).max() / peak)
    d0 = float(np.abs(y[:n] - h[:n]).max() / peak)
    print(f"far positions: e_seq {e_seq:.2e}, device at T - 300 {d:.2e}, at 0 {d0:.2e}, bar {max(64 * e_seq, 1e-13):.2e}")
    assert d <= max(64 * e_seq, 1e-13) and d0 <= max(64 * e_seq, 1e-13)


@functools.lru_cache(maxsize=None)
def room_case(reverse):
    from friture_amd import decay, sosfilter
    T = 1 << 15
    ir = np.stack([dh.response(T, rt, 70 + s, lead=200 + 60 * s) for s, rt in enumerate((0.12, 0.2))])
    centres, edges = decay.band_edges("octave")
    sos = np.stack([sosfilter.butter_band_sos(lo, hi, FS, 3) for lo, hi in edges])
    broadband = dh.restate_rows(ir, real=np.longdouble)
    y = sh.sequential(ir, sos, True, np.longdouble, reverse=reverse).astype(np.float64).reshape(2, len(sos), T)
    onset = [r["onset"] for r in broadband]
    bands = [dh.restate_rows(y[:, b], onset=onset, real=np.longdouble) for b in range(len(sos))]
    dh.check_gaps(broadband + [r for band in bands for r in band])
    ir.setflags(write=False)
    return ir, centres, broadband, bands


@pytest.mark.parametrize("filters", ["butterworth", "butterworth-reversed"])
def test_room_acoustics_with_butterworth_bands(hip, filters):
    """Two decaying-noise responses of 2^15 samples; the reference: sos_helpers' long double bank, then decay_helpers with the
    broadband onset.  The bars are those of the FIR pipeline test in test_decay_gpu.py."""
    from friture_amd import decay
    ir, centres, broadband, bands = room_case(filters.endswith("reversed"))
    room = decay.room_acoustics(ir, filters=filters)
    assert np.allclose(room.centres, centres, rtol=1e-12)
    dh.compare(type(room.broadband)(*map(host, room.broadband)), broadband, "broadband")
    got = type(room.bands)(*map(host, room.bands))
    assert got.edt.shape == (2, 6) and got.r2.shape == (2, 6, 4) and got.curve is None
    for b in range(6):
        res = type(got)(*[None if v is None else v[:, b] for v in got])
        dh.compare(res, bands[b], f"{filters}, band {centres[b]:.0f} Hz", db_bar=1e-8, rel_bar=1e-7)
    one = decay.room_acoustics(ir[1], filters=filters)
    assert one.bands.edt.shape == (6,)
    same_bits(one.bands.t20, got.t20[1])


@pytest.mark.parametrize("filters", ["butterworth", "butterworth-reversed"])
def test_speech_transmission_with_butterworth_bands(hip, filters):
    from friture_amd import decay, sosfilter, sti
    T = 1 << 15
    ir = np.stack([dh.response(T, rt, 90 + s, lead=200 + 60 * s) for s, rt in enumerate((0.12, 0.3))])
    broadband = dh.restate_rows(ir, real=np.longdouble)
    dh.check_gaps(broadband)
    start, stop = (np.array([r[name] for r in broadband]) for name in ("onset", "truncation"))
    centres, sos = sosfilter.band_sos(sti.octave_bands(), FS, 3)
    y = sh.sequential(ir, sos, True, np.longdouble, reverse=filters.endswith("reversed")).astype(np.float64).reshape(2, 7, T)
    ref_m = np.stack([sti_helpers.restate_mtf(y[:, b], start=start, stop=stop, real=np.longdouble)[0] for b in range(7)], axis=1)
    ref = sti_helpers.restate_sti(ref_m, real=np.longdouble)
    res = sti.speech_transmission(ir, filters=filters)
    assert res.m.shape == (2, 7, 14) and res.sti.shape == (2,) and np.allclose(res.centres, centres, rtol=1e-12)
    d_m, d_sti = sti_helpers.distance(res.m, ref_m), sti_helpers.distance(res.sti, ref["sti"])
    print(f"{filters}: m {d_m:.3g} (bar 1e-08), sti {d_sti:.3g} (bar 1e-07); STI {res.sti}")
    assert d_m <= 1e-8 and d_sti <= 1e-7
    one = sti.speech_transmission(ir[1], filters=filters)
    assert one.sti.shape == () and one.m.shape == (7, 14)
    same_bits(one.m, res.m[1])


def test_a_bad_argument_through_the_c_entry_point(mod):
    from friture_amd import _lib
    sos = np.ascontiguousarray(mod.band_sos("octave", FS, 3)[1][:2])
    dp, vp = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    h = _lib.Handle("sos", sos.ctypes.data_as(dp), 2, 3, 32)
    x, y = np.ones((2, 64)), np.full((2, 2, 64), 7.0)
    state = np.zeros((4, 30))

    def run(rows=2, n=64, xdt=1, stride=64, fan=1, reverse=0, before=0, sin=None, sout=None, scratch=1 << 20, ydt=1, out=y):
        return h.lib.frt_sos_run(h.h, vp(x.ctypes.data), xdt, rows, n, stride, fan, reverse, before, sin, sout, scratch,
                                 None if out is None else vp(out.ctypes.data), ydt)

    for kw in (dict(rows=0), dict(n=0), dict(n=(1 << 24) + 1), dict(xdt=2), dict(ydt=2), dict(stride=63), dict(fan=2), dict(reverse=2),
               dict(before=-1), dict(before=5), dict(reverse=1, sin=vp(state.ctypes.data)), dict(reverse=1, sout=vp(state.ctypes.data)),
               dict(scratch=-1), dict(out=None)):
        assert run(**kw) == -1, kw
        assert b"frt_sos_run" in h.lib.frt_last_error(), kw
    assert np.all(y == 7.0)                                      # nothing was launched
    bad = sos.copy()
    bad[1, 2, 5] = 1.5
    with pytest.raises(_lib.FritureHipError, match="frt_sos_create.*pole"):
        _lib.Handle("sos", bad.ctypes.data_as(dp), 2, 3, 32)
    with pytest.raises(_lib.FritureHipError, match="frt_sos_create.*cell"):
        _lib.Handle("sos", sos.ctypes.data_as(dp), 2, 3, 48)
    assert run() == 0 and not np.any(y == 7.0)
