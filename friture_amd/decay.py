"""How long a measured room rings: reverberation times and clarity from impulse responses on the GPU (decay.hip, frt_decay_*;
the definition: X3 in include/friture_hip.h).  The step after impulse_response and ConvolveBatch: Schroeder's backward
integration and the ISO 3382 numbers of whole batches of responses (responses times bands), from samples to results on the
device.  (The two-channel quantities of ISO 3382-1, the inter-aural cross-correlation coefficients and the lateral energy
fractions of a pair of responses measured at one point: friture_amd/spatial.py, X8.)

A row x[0 .. T) is float32 or float64, 1 <= T <= 2^24; fs defaults to 48000.  All arithmetic is float64: e[t] = (double)x[t]^2.
Parameters: block W = 480 samples (10 ms at 48 kHz; any integer in 8 .. 65536), onset_db = -20, noise_tail = 0.1, margin_db = 10.
1. Peak: p is the smallest t with |x[t]| = max |x|.  A row that is all zero, or that holds a non-finite sample, is a dead row:
   NaN in every float output, -1 in every index output; it never faults and never affects its neighbours.
2. Onset: t0 is the smallest t with |x[t]| >= c |x[p]|, c the double nearest 10^(onset_db / 20), made on the host; the test is
   exact.  onset= may instead give t0 per row, integers [R] with 0 <= t0 < T (the bands of one response share the broadband
   onset).
3. Noise: nb = floor(T / W); q[k] = the sum of e over [k W, (k + 1) W); nt = max(1, ceil(noise_tail nb)); N0 = (the sum of the
   last nt block sums) / (nt W); nb = 0: N0 = 0.
4. Truncation: truncate="auto": t1 = k W for the smallest k > floor(p / W) with q[k] <= W N0 10^(margin_db / 10), T if there is
   none; truncate=None: t1 = T; integers [R] with t0 < t1 <= T give t1 directly.
5. Schroeder integral and decay curve, t0 <= t < t1: E[t] = e[t] + .. + e[t1 - 1], L[t] = 10 log10(E[t] / E[t0]).
6. Decay times over the ranges (hi, lo): EDT (0, -10), T10 (-5, -15), T20 (-5, -25), T30 (-5, -35).  a is the smallest t with
   L[t] <= hi (EDT: a = t0), b the smallest t with L[t] <= lo; a least-squares line of L[t] over k = t - a, a <= t < b (the sums
   of k and k^2 are closed forms); RT = -60 / (slope fs) seconds; r2 is the squared correlation coefficient of the same fit;
   NaN when lo is not reached before t1 or b - a < 2.
7. Energy ratios, n50 = round(0.05 fs), n80 = round(0.08 fs), E[u] = 0 for u >= t1: C50 = 10 log10((E[t0] - E[t0 + n50]) /
   E[t0 + n50]), C80 the same with n80, D50 = (E[t0] - E[t0 + n50]) / E[t0] (a short response gives C = +inf and D50 = 1);
   Ts = sum (t - t0) e[t] / E[t0] / fs over [t0, t1).
8. level_db = 10 log10 E[t0]; noise_db = 10 log10 N0; dynamic_range = 10 log10(max_k q[k] / (W N0)), NaN when nb = 0 and +inf
   when N0 = 0; the integers peak, onset, truncation.
9. keep=("params", "curve") with curve_step= gives L[t0 + j step] as float64 [R, ceil(T / step)]; entries past t1 are NaN.
The bits of a row do not depend on the other rows of the call, on scratch_bytes, on a row stride or on the input's dtype (the
order of the sums: X3).  Out of scope: a carried state (a decay is integrated from its end, so a response is given whole),
Lundeby's iteration, the tail-compensation term, noise subtraction, sample rates handled in any way other than the fs argument
(IIR band filters: room_acoustics(filters="butterworth"), X6, friture_amd/sosfilter.py).  There is no CPU fallback: run() goes to the HIP library.

The band front (band_edges, band_filter, band_front, band_axis) is composition, shared by room_acoustics and
sti.speech_transmission: a Kaiser-windowed linear-phase FIR per band, designed on the host, applied by ConvolveBatch, its delay
cut off by a strided view that the consumer reads in place; or, with filters="butterworth" / "butterworth-reversed", Butterworth
band-passes on the IEC 61260-1 base-ten band edges run as one bank by SosBatch."""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import numpy as np

from . import _batchio, _lib, convolve

TILE = 512                                  # samples per tile of the scan (frt_decay_tile)
MAX_SAMPLES = 1 << 24
MIN_BLOCK, MAX_BLOCK = 8, 65536

DecayResult = namedtuple("DecayResult", "edt t10 t20 t30 r2 c50 c80 d50 ts level_db noise_db dynamic_range peak onset truncation curve")
RoomResult = namedtuple("RoomResult", "centres broadband bands")


class DecayBatch:
    """DecayBatch(fs=48000, block=480, onset_db=-20.0, noise_tail=0.1, margin_db=10.0).run(ir, onset=None, truncate="auto",
    keep=("params",), curve_step=48, scratch_bytes=1 << 28) -> DecayResult.  ir: [R, T] or [T], float32 or float64, numpy array or
    CUDA tensor (strided row views are read in place).  The results are of ir's kind: edt, t10, t20, t30, c50, c80, d50, ts,
    level_db, noise_db, dynamic_range float64 [R], r2 float64 [R, 4] (of EDT, T10, T20, T30), peak, onset, truncation int64 [R],
    curve float64 [R, ceil(T / curve_step)] or None ([T] in: without the R axis).  The rows are cut into slabs whose scratch
    stays within scratch_bytes; the result has the same bits at any slab size."""

    def __init__(self, fs=48000, block=480, onset_db=-20.0, noise_tail=0.1, margin_db=10.0):
        if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or not MIN_BLOCK <= block <= MAX_BLOCK:
            raise ValueError(f"block must be an integer in {MIN_BLOCK} .. {MAX_BLOCK}, got {block!r}")
        _batchio.check_fs(fs)
        if not (math.isfinite(onset_db) and onset_db <= 0):
            raise ValueError(f"onset_db must be at most 0, got {onset_db!r}")
        if not 0 < noise_tail <= 1:
            raise ValueError(f"noise_tail must lie in (0, 1], got {noise_tail!r}")
        if not (math.isfinite(margin_db) and margin_db >= 0):
            raise ValueError(f"margin_db must be at least 0, got {margin_db!r}")
        self.fs, self.block = float(fs), int(block)
        self.onset_db, self.noise_tail, self.margin_db = float(onset_db), float(noise_tail), float(margin_db)
        self._handle_ = None

    def _handle(self):
        if self._handle_ is None:
            self._handle_ = _lib.Handle("decay", self.fs, self.block, self.onset_db, self.noise_tail, self.margin_db)
        return self._handle_

    def run(self, ir, onset=None, truncate="auto", keep=("params",), curve_step=48, scratch_bytes=1 << 28):
        x, is_np, squeeze, _ = _batchio.check_samples("DecayBatch", ir, None)
        R, T = x.shape
        _batchio.check_streams(R)
        _batchio.check_row_samples(T)
        _batchio.check_scratch_bytes(scratch_bytes)
        keep = tuple(keep) if isinstance(keep, (list, tuple)) else keep
        _batchio.check_keep(keep, ("params",), ("params", "curve"))
        step = 0
        if "curve" in keep:
            if isinstance(curve_step, bool) or not isinstance(curve_step, (int, np.integer)) or not 1 <= curve_step <= MAX_SAMPLES:
                raise ValueError(f"curve_step must be an integer in 1 .. 2^24, got {curve_step!r}")
            step = int(curve_step)
        t0 = None if onset is None else _batchio.row_integers("onset", onset, R, 0, T - 1)
        if truncate is None:
            mode, t1 = 0, None
        elif isinstance(truncate, str):
            if truncate != "auto":
                raise ValueError(f"truncate={truncate!r} ('auto', None or integers [{R}])")
            mode, t1 = 1, None
        else:
            mode, t1 = 2, _batchio.row_integers("truncate", truncate, R, 1, T)
            if t0 is not None and np.any(t1 <= t0):
                raise ValueError("truncate must lie behind the onset in every row")
        h = self._handle()
        x, xptr, code, row, _ = _batchio.strided_rows(x)
        vp = ctypes.c_void_p
        nc = -(-T // step) if step else 0

        def call(_, params, indices, curve):
            _lib.check(h.lib.frt_decay_run(h.h, vp(xptr), code, R, T, row, vp(_batchio.ptr(t0)), mode, vp(_batchio.ptr(t1)), step,
                                           int(scratch_bytes), vp(_batchio.ptr(params)), vp(_batchio.ptr(indices)), vp(_batchio.ptr(curve))))

        def outputs():
            return (_batchio.alloc(x, (R, 15)), _batchio.alloc(x, (R, 3), np.int64), _batchio.alloc(x, (R, nc)) if step else None)

        params, indices, curve = _batchio.run_call(x, is_np, outputs, h.set_stream, call, None)
        cut = (lambda a: a[0]) if squeeze else (lambda a: a)
        p, i = cut(params), cut(indices)
        return DecayResult(p[..., 0], p[..., 1], p[..., 2], p[..., 3], p[..., 4:8], p[..., 8], p[..., 9], p[..., 10], p[..., 11], p[..., 12],
                           p[..., 13], p[..., 14], i[..., 0], i[..., 1], i[..., 2], None if curve is None else cut(curve))


# ---- the band front: composition, no kernel of its own --------------------------------------------------------------------------

def band_edges(bands="octave"):
    """(centres [B], edges [B, 2]) in Hz.  "octave": the IEC 61260-1 base-ten centres 1000 G^k, k = -3 .. 2 (125 Hz .. 4 kHz),
    edges fm G^(-1/2), fm G^(1/2), G = 10^0.3; "third": 1000 G^(k / 3), k = -10 .. 7 (100 Hz .. 5 kHz), edges fm G^(-1/6),
    fm G^(1/6); or a sequence of (f_lo, f_hi) pairs, whose centres are the geometric means."""
    G = 10.0 ** 0.3
    if isinstance(bands, str):
        if bands == "octave":
            fm, half = np.array([1000.0 * G ** k for k in range(-3, 3)]), G ** 0.5
        elif bands == "third":
            fm, half = np.array([1000.0 * G ** (k / 3) for k in range(-10, 8)]), G ** (1 / 6)
        else:
            raise ValueError(f"bands={bands!r} ('octave', 'third' or (f_lo, f_hi) pairs)")
        return fm, np.stack([fm / half, fm * half], axis=1)
    edges = np.asarray(bands, np.float64)
    if edges.ndim != 2 or edges.shape[1] != 2 or not edges.shape[0] or not np.all((0 < edges[:, 0]) & (edges[:, 0] < edges[:, 1])):
        raise ValueError(f"bands must be (f_lo, f_hi) pairs with 0 < f_lo < f_hi, got {bands!r}")
    return np.sqrt(edges[:, 0] * edges[:, 1]), edges


RIPPLE_SUM_DB = 20 * math.log10(2)          # a band-pass is the difference of two low-passes: their ripples can add


def band_filter(f_lo, f_hi, fs=48000, attenuation_db=60.0, transition=0.25):
    """One band's linear-phase FIR [2 M + 1] float64: a Kaiser-windowed difference of the ideal low-passes at f_hi and f_lo.
    The transition bands are transition (f_hi - f_lo) wide, centred on the edges; M and beta come from Kaiser's formulas for
    that width and attenuation_db + 6 dB (the ripples of the two low-passes can add), so beyond the transition bands the
    response stays at or below -attenuation_db.  The delay is M samples.  ValueError when 2 M + 1 exceeds convolve.MAX_TAPS."""
    if not (0 < f_lo < f_hi < fs / 2):
        raise ValueError(f"expected 0 < f_lo < f_hi < fs / 2, got {f_lo!r}, {f_hi!r} at fs {fs!r}")
    if not attenuation_db > 21 or not 0 < transition <= 1:
        raise ValueError(f"attenuation_db {attenuation_db!r} (above 21), transition {transition!r} (in (0, 1])")
    if f_lo - transition * (f_hi - f_lo) / 2 <= 0 or f_hi + transition * (f_hi - f_lo) / 2 >= fs / 2:
        raise ValueError(f"the transition bands of {f_lo!r} .. {f_hi!r} Hz leave 0 .. fs / 2")
    A = attenuation_db + RIPPLE_SUM_DB
    dw = 2 * math.pi * transition * (f_hi - f_lo) / fs                                    # rad/sample
    M = int(math.ceil((A - 8) / (2.285 * dw) / 2))
    if 2 * M + 1 > convolve.MAX_TAPS:
        raise ValueError(f"{f_lo!r} .. {f_hi!r} Hz at fs {fs!r} needs {2 * M + 1} taps (at most {convolve.MAX_TAPS})")
    beta = 0.1102 * (A - 8.7) if A > 50 else 0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21)
    n = np.arange(-M, M + 1, dtype=np.float64)
    lo, hi = f_lo / fs, f_hi / fs                                                         # cycles/sample
    return (2 * hi * np.sinc(2 * hi * n) - 2 * lo * np.sinc(2 * lo * n)) * np.kaiser(2 * M + 1, beta)


FILTERS = ("fir", "butterworth", "butterworth-reversed")


def check_filters(filters):
    if filters not in FILTERS:
        raise ValueError(f"filters={filters!r} ({', '.join(repr(f) for f in FILTERS)})")


def band_front(ir, edges, fs, filters, order):
    """The responses ir [S, T] or [T] through the band-passes on `edges`, as (rows, spread) pairs that a consumer runs on as
    they come; spread(v) makes a per-response vector v [S] fit `rows`.  filters="fir": one pair per band, rows =
    ConvolveBatch(band_filter(..)).run(ir).y[..., M : M + T], the delay cut off by a view, and v as it is.  Otherwise: one
    pair, the [S B, T] view of one bank run of SosBatch over the Butterworth band-passes of `order` (backwards in time for
    "butterworth-reversed") in float64, and every entry of v (or a scalar) once per band: [S B].  A band is filtered only
    when its pair is asked for; band_axis is the way back."""
    T = ir.shape[-1]
    if filters == "fir":
        for f_lo, f_hi in edges:
            h = band_filter(f_lo, f_hi, fs)
            M = (len(h) - 1) // 2
            yield convolve.ConvolveBatch(h).run(ir).y[..., M:M + T], lambda v: v
        return
    from . import sosfilter
    sos = np.stack([sosfilter.butter_band_sos(f_lo, f_hi, fs, order) for f_lo, f_hi in edges])
    y = sosfilter.SosBatch(sos).run(ir, fan=True, reverse=filters == "butterworth-reversed", dtype="float64").y

    def spread(v):                                                   # numpy or tensor as it came
        return v.reshape(-1).repeat_interleave(len(edges)) if hasattr(v, "repeat_interleave") else np.repeat(np.asarray(v).reshape(-1), len(edges))
    yield y.reshape(-1, T), spread


def band_axis(ir, B, filters, values):
    """One result per pair of band_front (per row of its rows, with any axes behind) as one array with a band axis behind ir's
    response axis: [S, B, ..], and [B, ..] for ir [T]."""
    lead = tuple(ir.shape[:-1])
    if filters != "fir":
        return values[0].reshape(lead + (B,) + tuple(values[0].shape[1:]))
    if isinstance(ir, np.ndarray):
        return np.stack(values, len(lead))
    import torch
    return torch.stack(values, len(lead))


def room_acoustics(ir, bands="octave", fs=48000, filters="fir", order=3, **decay_settings):
    """The broadband and per-band decay of responses ir [S, T] or [T]: RoomResult(centres [B], broadband, bands), two
    DecayResults, every field of `bands` with a band axis behind the response axis ([S, B]; r2 [S, B, 4]).  One broadband
    DecayBatch.run finds the onsets.  filters="fir": per band, ConvolveBatch(band_filter(..)).run(ir).y[..., M : M + T] is read in
    place with those onsets.  filters="butterworth": Butterworth band-passes of `order` on the same band edges
    (sosfilter.band_sos); one bank run of SosBatch gives [S, B, T] in float64 and its [S B, T] view goes through one
    DecayBatch.run with the broadband onsets repeated: no loop over the bands and no delay to cut.  "butterworth-reversed" runs
    the bank backwards in time (ISO 3382: a band's own ringing then lies in front of the decay, not on it).  decay_settings:
    DecayBatch's parameters, and truncate / scratch_bytes of its run()."""
    check_filters(filters)
    run_settings = {k: decay_settings.pop(k) for k in ("truncate", "scratch_bytes") if k in decay_settings}
    centres, edges = band_edges(bands)
    db = DecayBatch(fs=fs, **decay_settings)
    broadband = db.run(ir, **run_settings)
    given = not (run_settings.get("truncate") is None or isinstance(run_settings["truncate"], str))       # truncations [S]
    results = []
    for rows, spread in band_front(ir, edges, fs, filters, order):
        if given:
            run_settings["truncate"] = spread(run_settings["truncate"])
        results.append(db.run(rows, onset=spread(broadband.onset), **run_settings))
    fields = [None if v[0] is None else band_axis(ir, len(centres), filters, v) for v in zip(*results)]
    return RoomResult(centres, broadband, DecayResult(*fields))


