"""A sound level meter for whole recordings on the GPU: the quantities of IEC 61672-1.  Frequency weightings A, C and Z,
exponential time weightings (Fast 125 ms, Slow 1 s, or any 1 .. 4 time constants), and per logging interval Leq, the
time-weighted level at the interval's end, its maximum and minimum, and the peak; over the whole stream Leq, the sound exposure
level, LAFmax / LAFmin and the peak; percentile levels L10, L50, L90 from the logged levels.

The chain: x -> the weighting as a SosBatch cascade (weighting_sos; none for Z) -> with `bands`, one Butterworth band bank in
bank mode (sosfilter.band_sos) -> the detector (soundlevel.hip, frt_spl_*; the definition with its operation order: X7 in
include/friture_hip.h).  Between the stages the samples are float64.  The detector squares the weighted samples, q = w w, runs
e_i[n] = a_i e_i[n-1] + g_i q[n] (a_i = exp(-1 / (fs tau_i)), g_i = 1 - a_i made as -expm1) per time constant, time-parallel over
cells of `cell` samples on a grid anchored at the stream's absolute sample index, and reports per interval of `interval`
samples the energy (sum of q), max |w|, and each e_i's end value, maximum and minimum.  A stream of at most `cell` samples is the
sequential recurrence bit for bit; a recording cut into calls at any sample, any scratch_bytes, batch, row stride, input dtype
and host or device buffers give the bits of one whole call: run() returns the state that continues the streams.

The A and C weightings are the analogue prototypes of IEC 61672-1 (poles at f1 = 20.598997 Hz and f4 = 12194.217 Hz, both double;
A adds f2 = 107.65265 Hz and f3 = 737.86223 Hz; four zeros at s = 0 for A, two for C) through the plain bilinear transform,
without pre-warping, the gain set so that the response at 1 kHz is exactly 0 dB.  The digital response at f is the analogue one
at fs / pi tan(pi f / fs); at fs = 48 kHz the deviation from the analogue curve at f itself is, for A and C alike:
    10 Hz .. 500 Hz   at most 0.004 dB (0.0044 dB at the low end: the normalisation at 1 kHz, where the warp is -0.0044 dB)
    4 kHz             -0.04 dB
    8 kHz             -0.54 dB
    10 kHz            -1.22 dB
    12.5 kHz          -2.67 dB
    16 kHz            -6.4 dB
    20 kHz            -15.8 dB
It is documented, not corrected.  Out of scope: the Impulse time weighting, class conformity claims for a whole instrument,
fusing the weighting into the detector pass, a live chunk object, percentiles carried in the state.
There is no CPU fallback: run() goes to the HIP library."""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import numpy as np

from . import _batchio, _lib
from .sosfilter import SosBatch, band_sos

F1, F2, F3, F4 = 20.598997, 107.65265, 737.86223, 12194.217
MAX_TAUS = 4
MIN_CELL, MAX_CELL, MAX_INTERVAL = 16, 1024, 1 << 20
STATE_VECTORS, STATE_SCALARS = 9, 5          # X7: z p s q u imax imin tmax tmin [ntau] each; cellE intE intPeak totE totPeak

# data: [rows, 9 ntau + 5] float64; rows: detector rows; n: samples seen; final: made by a flushed call
DetectorState = namedtuple("DetectorState", "data rows n final settings")
# filters: the SosStates of the weighting and of the band bank (those that exist), detector: a DetectorState
SoundLevelState = namedtuple("SoundLevelState", "filters detector")
DetectorResult = namedtuple("DetectorResult", "energy peak last max min count total_energy total_peak total_max total_min total_count state")
SoundLevelResult = namedtuple("SoundLevelResult", "leq lmax lmin level peak_db energy peak count total_leq sel total_lmax total_lmin "
                                                  "total_peak_db state")


# ---- design: the A and C weightings, numpy only -----------------------------------------------------------------------------------

def weighting_sos(kind, fs=48000):
    """The frequency weighting `kind` of IEC 61672-1 as second-order sections [K, 6] (a0 = 1) for SosBatch: "A" [3, 6], "C"
    [2, 6], "Z" None.  The analogue prototype's real poles -2 pi f_k map to z = (2 fs - w) / (2 fs + w) (plain bilinear
    transform, no pre-warping), its zeros at s = 0 to z = 1 and those at infinity to z = -1.  Sections: the double pole f1 with
    two zeros at 1; for A, f2 and f3 with two zeros at 1; the double pole f4 with two zeros at -1.  The gain, spread evenly over
    the sections, makes the response at 1 kHz exactly 0 dB.  The deviation from the analogue curve (the same for A and C) is
    tabulated in the module's docstring."""
    if kind == "Z":
        return None
    if kind not in ("A", "C"):
        raise ValueError(f"weighting must be 'A', 'C' or 'Z', got {kind!r}")
    _batchio.check_fs(fs)
    fs2 = 2.0 * fs

    def pole(f):
        w = 2.0 * math.pi * f
        return (fs2 - w) / (fs2 + w)

    p1, p2, p3, p4 = pole(F1), pole(F2), pole(F3), pole(F4)
    rows = [([1.0, -2.0, 1.0], p1, p1)]
    if kind == "A":
        rows.append(([1.0, -2.0, 1.0], p2, p3))
    rows.append(([1.0, 2.0, 1.0], p4, p4))
    sos = np.array([b + [1.0, -(pa + pb), pa * pb] for b, pa, pb in rows], np.float64)
    zi = np.exp(-2j * np.pi * np.longdouble(1000.0) / np.longdouble(fs)).astype(np.clongdouble)
    s = sos.astype(np.longdouble)
    h = np.prod((s[:, 0] + s[:, 1] * zi + s[:, 2] * zi * zi) / (s[:, 3] + s[:, 4] * zi + s[:, 5] * zi * zi))
    sos[:, :3] *= float(np.abs(h) ** (np.longdouble(-1.0) / len(rows)))
    return sos


# ---- percentile levels --------------------------------------------------------------------------------------------------------

def percentile_levels(levels, percents=(10, 50, 90)):
    """L_N, the level exceeded N % of the time, for every N of `percents`, as an exact order statistic of the logged levels:
    levels [J] or [rows, J] (numpy array or tensor; for instance SoundLevelResult.level[..., 0]) gives [P] or [rows, P] of the
    same kind.  With a row sorted ascending as v[0 .. J - 1], L_N = v[floor((J - 1) (1 - N / 100) + 0.5)]: the index rule of
    loudness.loudness_range.  NaN for a row without levels.  Nothing in it waits for the device."""
    pct = [float(p) for p in percents]
    if any(not 0.0 <= p <= 100.0 for p in pct):
        raise ValueError(f"percents must lie in 0 .. 100, got {percents!r}")
    if levels.ndim not in (1, 2):
        raise ValueError(f"expected levels [J] or [rows, J], got {tuple(levels.shape)}")
    rows = levels.reshape(1, -1) if levels.ndim == 1 else levels
    R, J = rows.shape
    is_np = isinstance(levels, np.ndarray)
    if J == 0:
        if is_np:
            out = np.full((R, len(pct)), math.nan)
        else:
            import torch
            out = torch.full((R, len(pct)), math.nan, dtype=torch.float64, device=levels.device)
    else:
        index = [int(math.floor((J - 1) * (1.0 - p / 100.0) + 0.5)) for p in pct]
        if is_np:
            out = np.sort(rows.astype(np.float64), axis=1)[:, index]
        else:
            import torch
            out = rows.to(torch.float64).sort(dim=1).values[:, index]
    return out[0] if levels.ndim == 1 else out


# ---- the batch --------------------------------------------------------------------------------------------------------------------

def _integer(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {v!r}")
    return int(v)


def _db(v, scale):
    if isinstance(v, (np.ndarray, np.generic, float)):
        with np.errstate(divide="ignore", invalid="ignore"):
            return scale * np.log10(v)
    import torch
    return scale * torch.log10(v)


class SoundLevelBatch:
    """SoundLevelBatch(weighting="A", interval=4800, taus=(0.125, 1.0), fs=48000, cal_db=0.0, bands=None, order=3, cell=None)
    .run(x, state=None, flush=True, scratch_bytes=1 << 28) -> SoundLevelResult.  x: [T] or [S, T], float32 or float64, numpy
    array or CUDA tensor (strided row views are read in place).  weighting "A", "C" or "Z"; bands None, "octave", "third" or
    (f_lo, f_hi) pairs: Butterworth band-passes of `order` (sosfilter.band_sos) behind the weighting, and every result gets a
    band axis behind the stream axis.  interval: a multiple of 16 in 16 .. 2^20 samples; cell: a multiple of 16 in 16 .. 1024
    that divides it (None: the library's default for the interval); taus: 1 .. 4 time constants in seconds.
    Results are float64 and of x's kind, J the intervals the call emits (without flush those its last sample completes; flush
    adds the partial last one, after which the state is final); in dB, 10 log10 v + cal_db:
        leq [S, J] (energy / count), level [S, J, ntau] (the time-weighted level at the interval's end), lmax, lmin [S, J, ntau];
        peak_db [S, J] = 20 log10 peak + cal_db;
    linear: energy [S, J] (sum of squares), peak [S, J] (max |w|), count [J] int64 (samples per interval);
    over the emitted intervals of the whole stream so far: total_leq, sel (10 log10(energy / fs) + cal_db), total_peak_db [S],
    total_lmax, total_lmin [S, ntau].  Silence gives -inf.  The linear values have the same bits for numpy and CUDA input; the
    decibels are made from them with the kind's own log10.  With x [T] the stream axis is left out.  state: a SoundLevelState,
    the pair (the filter stages' SosStates, the detector's DetectorState)."""

    def __init__(self, weighting="A", interval=4800, taus=(0.125, 1.0), fs=48000, cal_db=0.0, bands=None, order=3, cell=None):
        _batchio.check_fs(fs)
        self.fs = float(fs)
        self.weighting = weighting
        wsos = weighting_sos(weighting, fs)
        self.interval = _integer("interval", interval, MIN_CELL, MAX_INTERVAL)
        if self.interval % 16:
            raise ValueError(f"interval must be a multiple of 16, got {interval!r}")
        if cell is None:
            cell = _lib.load().frt_spl_default_cell(self.interval)
        self.cell = _integer("cell", cell, MIN_CELL, MAX_CELL)
        if self.cell % 16 or self.interval % self.cell:
            raise ValueError(f"cell must be a multiple of 16 that divides the interval {self.interval}, got {cell!r}")
        t = np.atleast_1d(np.asarray(taus, np.float64))
        if t.ndim != 1 or not 1 <= t.size <= MAX_TAUS:
            raise ValueError(f"expected 1 .. {MAX_TAUS} time constants, got {taus!r}")
        if not np.all(np.isfinite(t) & (t > 0)):
            raise ValueError(f"time constants must be finite and positive, got {taus!r}")
        self.taus = np.ascontiguousarray(t)
        self.ntau = int(t.size)
        if not (isinstance(cal_db, (int, float, np.integer, np.floating)) and math.isfinite(cal_db)):
            raise ValueError(f"cal_db must be finite, got {cal_db!r}")
        self.cal_db = float(cal_db)
        self.tables()                                                # the library's own check of the time constants
        self._filters = []                                           # (SosBatch, fan)
        if wsos is not None:
            self._filters.append((SosBatch(wsos), False))
        self.centres, self.n_bands = None, 0
        band_key = None
        if bands is not None:
            self.centres, bsos = band_sos(bands, fs, order)
            self.n_bands = int(bsos.shape[0])
            self._filters.append((SosBatch(bsos), True))
            band_key = self._filters[-1][0].settings
        self.state_length = STATE_VECTORS * self.ntau + STATE_SCALARS
        self.settings = (str(weighting), self.interval, self.cell, tuple(self.taus.tolist()), self.fs, band_key)
        self._handle_ = None

    # ---- host only ------------------------------------------------------------------------------------------------------------
    def _taus_ptr(self):
        return self.taus.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def tables(self):
        """(a, g, A, A64), [ntau] each, as the library makes them in long double, rounded once (X7).  Needs no GPU."""
        out = [np.empty(self.ntau) for _ in range(4)]
        dp = ctypes.POINTER(ctypes.c_double)
        try:
            _lib.check(_lib.load().frt_spl_tables(self.fs, self._taus_ptr(), self.ntau, self.interval, self.cell,
                                                  *[o.ctypes.data_as(dp) for o in out]))
        except _lib.FritureHipError as e:
            raise ValueError(str(e)) from None
        return tuple(out)

    def _check_detector_state(self, det, rows):
        if det is None:
            return None, 0
        if not isinstance(det, tuple) or len(det) != 5:
            raise ValueError("the detector's state must be the DetectorState of an earlier call")
        data, srows, n, final, settings = det
        if tuple(settings) != self.settings:
            raise ValueError(f"state of other settings: {tuple(settings)} (want {self.settings})")
        if final:
            raise ValueError("state of a flushed call: it is final")
        want = (rows, self.state_length)
        if int(srows) != rows or data is None or tuple(data.shape) != want:
            raise ValueError(f"state of another shape: {None if data is None else tuple(data.shape)} for {srows} rows (want {want})")
        if int(n) < 0:
            raise ValueError(f"state of another stream: {n} samples")
        return data, int(n)

    def _check_state(self, state, rows):
        if state is None:
            return [None] * len(self._filters), None
        if not isinstance(state, tuple) or len(state) != 2:
            raise ValueError("state must be the SoundLevelState of an earlier run")
        filters, det = state
        self._check_detector_state(det, rows)
        if len(filters) != len(self._filters):
            raise ValueError(f"state of another shape: {len(filters)} filter stages (want {len(self._filters)})")
        return list(filters), det

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def _handle(self):
        if self._handle_ is None:
            self._handle_ = _lib.Handle("spl", self.fs, self._taus_ptr(), self.ntau, self.interval, self.cell)
        return self._handle_

    def detect(self, w, state=None, flush=True, scratch_bytes=1 << 28):
        """The detector alone, on rows w [T] or [R, T] that are already weighted -> DetectorResult of linear float64 values of
        w's kind: energy, peak [R, J]; last, max, min [R, J, ntau]; count [J] int64; over the emitted intervals of the stream so
        far total_energy, total_peak [R], total_max, total_min [R, ntau] and total_count (an integer); state: the DetectorState
        that continues the rows (final after a flush)."""
        w, is_np, squeeze, _ = _batchio.check_samples("SoundLevelBatch", w, None)
        rows, T = w.shape
        _batchio.check_streams(rows)
        _batchio.check_row_samples(T)
        _batchio.check_scratch_bytes(scratch_bytes)
        flush = bool(flush)
        data, n_in = self._check_detector_state(state, rows)
        h = self._handle()
        J = int(h.lib.frt_spl_intervals_for(self.interval, n_in, T, int(flush)))
        nt, NF = self.ntau, 2 + 3 * self.ntau
        w, wptr, code, row, _ = _batchio.strided_rows(w)
        vp, nfo = ctypes.c_void_p, ctypes.c_int64(0)

        def call(state_in, state_out, vals, count):
            _lib.check(h.lib.frt_spl_run(h.h, vp(wptr), code, rows, T, row, n_in, vp(_batchio.ptr(state_in)), vp(_batchio.ptr(state_out)),
                                         int(flush), int(scratch_bytes), vp(_batchio.ptr(vals)), vp(_batchio.ptr(count)), ctypes.byref(nfo)))
            assert nfo.value == J

        def outputs():
            return (_batchio.alloc(w, (rows, self.state_length)), _batchio.alloc(w, (rows, J, NF)), _batchio.alloc(w, (J,), np.int64))

        new, vals, count = _batchio.run_call(w, is_np, outputs, h.set_stream, call, data)
        n_out = n_in + T
        base = STATE_VECTORS * nt
        fields = [vals[..., 0], vals[..., 1], vals[..., 2:2 + nt], vals[..., 2 + nt:2 + 2 * nt], vals[..., 2 + 2 * nt:], count,
                  new[:, base + 3], new[:, base + 4], new[:, 7 * nt:8 * nt], new[:, 8 * nt:9 * nt]]
        if squeeze:
            fields = [f if f is count else f[0] for f in fields]
        return DetectorResult(*fields, n_out if flush else n_out // self.interval * self.interval,
                              DetectorState(new, rows, n_out, flush, self.settings))

    def run(self, x, state=None, flush=True, scratch_bytes=1 << 28):
        x, is_np, squeeze, _ = _batchio.check_samples("SoundLevelBatch", x, None)
        S, T = x.shape
        B = max(self.n_bands, 1)
        _batchio.check_streams(S * B)
        _batchio.check_row_samples(T)
        _batchio.check_scratch_bytes(scratch_bytes)
        fstates, det = self._check_state(state, S * B)
        w, new_filters = x, []
        for (sos, fan), st in zip(self._filters, fstates):
            r = sos.run(w, fan=fan, state=st, dtype="float64", scratch_bytes=scratch_bytes)
            w = r.y.reshape(-1, T)
            new_filters.append(r.state)
        d = self.detect(w, det, flush, scratch_bytes)

        def shaped(v):                                               # [S B, ..] -> [S, B, ..], [S, ..], [B, ..] or [..]
            v = v.reshape((S, B) + tuple(v.shape[1:]))
            v = v if self.n_bands else v[:, 0]
            return v[0] if squeeze else v

        energy, peak, last, vmax, vmin, tot_e, tot_p, tot_max, tot_min = (
            shaped(v) for v in (d.energy, d.peak, d.last, d.max, d.min, d.total_energy, d.total_peak, d.total_max, d.total_min))
        cal = self.cal_db
        fcount = d.count.astype(np.float64) if is_np else d.count.to(energy.dtype)
        mean_total = tot_e / d.total_count if d.total_count else tot_e * math.nan
        return SoundLevelResult(
            leq=_db(energy / fcount, 10.0) + cal, lmax=_db(vmax, 10.0) + cal, lmin=_db(vmin, 10.0) + cal, level=_db(last, 10.0) + cal,
            peak_db=_db(peak, 20.0) + cal, energy=energy, peak=peak, count=d.count,
            total_leq=_db(mean_total, 10.0) + cal, sel=_db(tot_e / self.fs, 10.0) + cal,
            total_lmax=_db(tot_max, 10.0) + cal, total_lmin=_db(tot_min, 10.0) + cal, total_peak_db=_db(tot_p, 20.0) + cal,
            state=SoundLevelState(tuple(new_filters), d.state))


def sound_levels(x, weighting="A", **kw):
    """SoundLevelBatch(weighting, **kw).run(x) in one flushed call."""
    return SoundLevelBatch(weighting, **kw).run(x)
