"""How spacious a measured room sounds: the two-channel quantities of ISO 3382-1 from pairs of impulse responses on the GPU
(spatial.hip, frt_spatial_*; the definition: X8 in include/friture_hip.h).  The step beside DecayBatch for a dummy-head or an
omnidirectional / figure-of-eight measurement: the inter-aural cross-correlation coefficients of Annex B and the sums behind
the lateral energy fractions of Annex A, from samples to results on the device.

A pair is two rows of T samples, 1 <= T <= 2^24, float32 or float64: row 0 is l (the left ear, or the omnidirectional microphone),
row 1 is r (the right ear, or the figure-of-eight).  All arithmetic is float64 on samples converted to double.  Settings: fs =
48000; max_lag M, an integer number of samples in 0 .. 128, default round(fs / 1000), the +-1 ms of the standard; windows, 1 to 4
(start, stop) pairs in seconds behind the onset, stop None for "to the end", turned into samples a_w = round(start fs), b_w =
round(stop fs) with 0 <= a_w < b_w; onset_db = -20.
1. End: stop= gives e per pair, integers [S] with 1 <= e <= T (default T).  A sample of either row outside [0, e) counts as zero
   and is never read into a result, whatever it holds, NaN included.
2. Dead pair: [0, e) holds a non-finite sample in either row, or both rows are all zero there: NaN in every float output, -1 in
   every index output; it never faults and never changes its neighbours' bits.
3. Peak and onset: P = max |x| over both rows and [0, e); peak is the smallest t with max(|l[t]|, |r[t]|) = P; t0 is the smallest
   t with max(|l[t]|, |r[t]|) >= c P, c the double nearest 10^(onset_db / 20), made on the host; the test is exact.  onset= may
   instead give t0 per pair, integers [S] in 0 .. e - 1 (the bands of one response share the broadband onset).
4. Windows: [A_w, B_w) = [min(t0 + a_w, e), min(t0 + b_w, e)), B_w = e for a stop of None.  An empty window is legal.
5. Sums over t in [A_w, B_w): El_w = sum l[t]^2, Er_w = sum r[t]^2, X_w = sum |l[t] r[t]|, C_w[tau] = sum l[t] r[t + tau] for
   tau = -M .. M; r[t + tau] may lie outside the window but not outside [0, e).
6. IACF_w[tau] = C_w[tau] / sqrt(El_w Er_w), iacc_w = max |IACF_w[tau]|, lag_index k_w = the smallest tau + M that attains it,
   tau_w = (k_w - M) / fs seconds.  El_w Er_w = 0 (an empty or silent window): iacc, tau and iacf NaN, lag_index -1, the sums as
   they are.
The bits of a pair do not depend on the other pairs of the call, on scratch_bytes, on any stride, on the input's dtype or on numpy
against CUDA (the order of the sums: X8).  A window's bits do depend on the cut points that the other windows put inside it: every
sample is summed once, in the segments between the windows' ends.  Out of scope: fractional lags, M > 128, a carried state (the
onset anchors everything, so a response is given whole), L_J's 10 m free-field reference (the caller supplies a reference
energy), head-related or microphone calibration of any kind.  There is no CPU fallback: run() goes to the HIP library.

lateral_fractions and binaural_acoustics are composition, no kernel of their own."""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import numpy as np

from . import _batchio, _lib, decay

TILE = 2048                                 # samples per tile of the correlation (frt_spatial_tile)
MAX_LAG, MAX_WINDOWS = 128, 4
DEFAULT_WINDOWS = ((0, 0.08), (0.08, None), (0, None))
LATERAL_WINDOWS = ((0, 0.08), (0.005, 0.08), (0.08, None), (0, None))

SpatialResult = namedtuple("SpatialResult", "iacc tau cross_abs energy lag_index peak onset iacf")
LateralResult = namedtuple("LateralResult", "lf lfc late_lateral lj")
BinauralResult = namedtuple("BinauralResult", "centres broadband bands iacc_e3")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def window_samples(windows, fs):
    """((a_w, b_w), ..) in samples from (start, stop) pairs in seconds, b_w = -1 for a stop of None; ValueError for anything but
    1 to 4 pairs with 0 <= a_w < b_w."""
    try:
        pairs = [tuple(w) for w in windows]
    except TypeError:
        raise ValueError(f"windows must be (start, stop) pairs, got {windows!r}") from None
    if not 1 <= len(pairs) <= MAX_WINDOWS or any(len(w) != 2 for w in pairs):
        raise ValueError(f"windows must be 1 .. {MAX_WINDOWS} (start, stop) pairs, got {windows!r}")
    out = []
    for start, stop in pairs:
        ok = isinstance(start, (int, float, np.integer, np.floating)) and math.isfinite(start) and start >= 0
        ok = ok and (stop is None or (isinstance(stop, (int, float, np.integer, np.floating)) and math.isfinite(stop)))
        if not ok:
            raise ValueError(f"a window is (start >= 0, stop or None) in seconds, got {(start, stop)!r}")
        a = int(math.floor(start * fs + 0.5))
        b = -1 if stop is None else int(math.floor(stop * fs + 0.5))
        if a >= 1 << 31 or b > 1 << 31 or (b != -1 and b <= a):
            raise ValueError(f"a window needs 0 <= round(start fs) < round(stop fs) <= 2^31, got {(start, stop)!r} at fs {fs!r}")
        out.append((a, b))
    return tuple(out)


class SpatialBatch:
    """SpatialBatch(fs=48000, max_lag=None, windows=((0, 0.08), (0.08, None), (0, None)), onset_db=-20.0).run(pairs, onset=None,
    stop=None, keep=("params",), scratch_bytes=1 << 28) -> SpatialResult.  pairs: [S, 2, T] or [2, T], float32 or float64, numpy
    array or CUDA tensor (strided views, pair stride and row stride, are read in place).  The results are of the pairs' kind: iacc,
    tau, cross_abs float64 [S, W], energy float64 [S, W, 2] (El, Er), lag_index int64 [S, W], peak, onset int64 [S], iacf float64
    [S, W, 2 M + 1] with keep=("params", "iacf"), otherwise None ([2, T] in: without the S axis).  The pairs are cut into slabs
    whose scratch stays within scratch_bytes; the result has the same bits at any slab size."""

    def __init__(self, fs=48000, max_lag=None, windows=DEFAULT_WINDOWS, onset_db=-20.0):
        _batchio.check_fs(fs)
        if max_lag is None:
            max_lag = int(math.floor(fs / 1000 + 0.5))
            if max_lag > MAX_LAG:
                raise ValueError(f"max_lag defaults to round(fs / 1000) = {max_lag} at fs {fs!r}, above {MAX_LAG}: give one")
        if not _is_int(max_lag) or not 0 <= max_lag <= MAX_LAG:
            raise ValueError(f"max_lag must be an integer in 0 .. {MAX_LAG}, got {max_lag!r}")
        if not (isinstance(onset_db, (int, float, np.integer, np.floating)) and math.isfinite(onset_db) and onset_db <= 0):
            raise ValueError(f"onset_db must be at most 0, got {onset_db!r}")
        self.fs, self.max_lag, self.onset_db = float(fs), int(max_lag), float(onset_db)
        self.windows = window_samples(windows, self.fs)
        self._handle_ = None

    def _handle(self):
        if self._handle_ is None:
            W = len(self.windows)
            a = (ctypes.c_int64 * W)(*[w[0] for w in self.windows])
            b = (ctypes.c_int64 * W)(*[w[1] for w in self.windows])
            self._handle_ = _lib.Handle("spatial", self.fs, self.max_lag, a, b, W, self.onset_db)
        return self._handle_

    def run(self, pairs, onset=None, stop=None, keep=("params",), scratch_bytes=1 << 28):
        x, is_np, squeeze, _ = _batchio.check_samples("SpatialBatch", pairs, None, dual=True)
        S, _, T = x.shape
        _batchio.check_streams(S)
        _batchio.check_row_samples(T)
        _batchio.check_scratch_bytes(scratch_bytes)
        keep = tuple(keep) if isinstance(keep, (list, tuple)) else keep
        _batchio.check_keep(keep, ("params",), ("params", "iacf"))
        e = None if stop is None else _batchio.row_integers("stop", stop, S, 1, T)
        t0 = None if onset is None else _batchio.row_integers("onset", onset, S, 0, T - 1)
        if t0 is not None and e is not None and np.any(t0 >= e):
            raise ValueError("onset must lie before stop in every pair")
        h = self._handle()
        x, xptr, code, row, pair = _batchio.strided_rows(x, dual=True)
        vp = ctypes.c_void_p
        W, nl = len(self.windows), 2 * self.max_lag + 1

        def call(_, params, indices, iacf):
            _lib.check(h.lib.frt_spatial_run(h.h, vp(xptr), code, S, T, row, pair, vp(_batchio.ptr(t0)), vp(_batchio.ptr(e)), int(scratch_bytes),
                                             vp(_batchio.ptr(params)), vp(_batchio.ptr(indices)), vp(_batchio.ptr(iacf))))

        def outputs():
            return (_batchio.alloc(x, (S, W, 5)), _batchio.alloc(x, (S, W + 2), np.int64),
                    _batchio.alloc(x, (S, W, nl)) if "iacf" in keep else None)

        params, indices, iacf = _batchio.run_call(x, is_np, outputs, h.set_stream, call, None)
        cut = (lambda a: a[0]) if squeeze else (lambda a: a)
        p, i = cut(params), cut(indices)
        return SpatialResult(p[..., 0], p[..., 1], p[..., 2], p[..., 3:5], i[..., :W], i[..., W], i[..., W + 1],
                             None if iacf is None else cut(iacf))


# ---- composition, no kernel of its own -------------------------------------------------------------------------------------------

def lateral_fractions(pairs, fs=48000, ref_energy=None, **run_settings):
    """The lateral energy measures of ISO 3382-1 Annex A from pairs [S, 2, T] or [2, T] of an omnidirectional response (row 0)
    and a figure-of-eight response (row 1): LateralResult(lf, lfc, late_lateral, lj), each [S] (or a scalar array) of the pairs'
    kind.  One SpatialBatch.run with max_lag = 0 and the windows (0, 0.08), (0.005, 0.08), (0.08, None), (0, None) behind the onset:
    lf = Er(5 .. 80 ms) / El(0 .. 80 ms), lfc = X(5 .. 80 ms) / El(0 .. 80 ms) with X = sum |l r|, late_lateral = Er(80 ms ..),
    lj = 10 log10(late_lateral / ref_energy) when ref_energy (the energy of the omnidirectional response at 10 m in a free field,
    a scalar or [S]) is given, otherwise None.  The ratios are elementwise; run_settings: onset, stop, scratch_bytes of run()."""
    r = SpatialBatch(fs=fs, max_lag=0, windows=LATERAL_WINDOWS).run(pairs, **run_settings)
    omni_early = r.energy[..., 0, 0]
    lf = r.energy[..., 1, 1] / omni_early
    lfc = r.cross_abs[..., 1] / omni_early
    late = r.energy[..., 2, 1]
    lj = None
    if ref_energy is not None:
        on_device = hasattr(late, "is_cuda")
        ratio = late / (ref_energy if on_device else np.asarray(ref_energy, np.float64))
        lj = 10.0 * (ratio.log10() if on_device else np.log10(ratio))
    return LateralResult(lf, lfc, late, lj)


def binaural_acoustics(pairs, bands="octave", fs=48000, filters="fir", order=3, **settings):
    """The broadband and per-band inter-aural cross-correlation of binaural pairs [S, 2, T] or [2, T]: BinauralResult(centres [B],
    broadband, bands, iacc_e3), two SpatialResults, every field of `bands` with a band axis behind the response axis ([S, B, W];
    energy [S, B, W, 2]).  One broadband SpatialBatch.run finds the onsets.  The rows go through decay.band_front ear by ear, as
    [2 S, T] (all left rows, then all right rows: a view for [2, T], one copy otherwise), so that the band rows of a pair lie a
    fixed stride apart and are read in place: filters="fir" gives one SpatialBatch.run per band, the filter's delay cut from both
    rows alike, so lags are unchanged; the Butterworth choices give one SosBatch bank run and one SpatialBatch.run over [S B]
    pairs, the broadband onsets repeated per band.  iacc_e3, for bands="octave": the mean (a + b + c) / 3 of the first window's
    iacc (the early one, with the default windows) over the 500 Hz, 1 kHz and 2 kHz octaves, [S]; otherwise None.  settings:
    SpatialBatch's max_lag, windows, onset_db, and stop / keep / scratch_bytes of its run()."""
    decay.check_filters(filters)
    run_settings = {k: settings.pop(k) for k in ("stop", "keep", "scratch_bytes") if k in settings}
    centres, edges = decay.band_edges(bands)
    sb = SpatialBatch(fs=fs, **settings)
    broadband = sb.run(pairs, **run_settings)
    x3 = pairs if pairs.ndim == 3 else pairs[None]
    S, _, T = x3.shape
    ears = x3[0] if S == 1 else (np.ascontiguousarray(x3.transpose(1, 0, 2)) if isinstance(x3, np.ndarray)
                                 else x3.transpose(0, 1).contiguous()).reshape(2 * S, T)
    onset = broadband.onset.reshape(-1)
    results = []
    for rows, spread in decay.band_front(ears, edges, fs, filters, order):
        n = rows.shape[0] // 2                                              # S, or S B with the band index fastest
        both = rows.reshape(2, n, T) if isinstance(rows, np.ndarray) else rows.view(2, n, T)
        if "stop" in run_settings:
            run_settings["stop"] = spread(_batchio.row_integers("stop", run_settings["stop"], onset.shape[0], 1, T))
        view = both.transpose(1, 0, 2) if isinstance(both, np.ndarray) else both.transpose(0, 1)
        if pairs.ndim == 2 and filters == "fir":
            view = view[0]                                                  # [2, T] in: no response axis in front of the band axis
        results.append(sb.run(view, onset=spread(onset), **run_settings))
    like = pairs[..., 0, :]
    fields = [None if v[0] is None else decay.band_axis(like, len(centres), filters, v) for v in zip(*results)]
    per_band = SpatialResult(*fields)
    e3 = None
    if isinstance(bands, str) and bands == "octave":
        i = per_band.iacc
        e3 = (i[..., 2, 0] + i[..., 3, 0] + i[..., 4, 0]) / 3
    return BinauralResult(centres, broadband, per_band, e3)
