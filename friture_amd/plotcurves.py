"""The plot curves of the spectrum and octave-spectrum docks (friture/spectrumPlotWidget.py SpectrumPlotWidget, friture/histplot.py
HistPlot) without Qt, on the GPU (curves.hip, frt_curves_run).

Per refresh the widgets turn a dB row into the filled signal curve (screen-space y and its intensity z) and, carried across
refreshes, a peak-hold curve that holds for 64 refreshes and then falls by c, 2c, 3c, ... (c = 20 log10(1 - 3e-6) 5000).  The bin
edges and their screen positions depend only on the settings: they are computed here on the host in the reference's numpy
operations and cached.  `SpectrumPlot` and `HistPlot` are the widgets' setdata (one device call and one synchronisation per
refresh, the peak state on the device); `CurveBatch` runs S streams x R refreshes x B bins in one call with the state carried in
and out."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import _batchio, _lib
from ._batchio import ptr as _ptr
from .constants import SAMPLING_RATE
from .plotting import frequency_scales as fscales

PEAK_DECAY_RATE = 1.0 - 3e-6                                       # spectrumPlotWidget.py:20, histplot.py:31
PEAK_DECAY_STEP = 20.0 * np.log10(PEAK_DECAY_RATE) * 5000          # the reset decay and its increment
PEAK_RESET = -500.0
HIST_FMIN, HIST_FMAX = 44, 22000                                   # HistPlot's fixed horizontal axis


class ScreenTransform:
    """CoordinateTransform (friture/plotting/coordinateTransform.py) with length 1 and no borders, toScreen only."""

    def __init__(self, coord_min, coord_max, scale=fscales.Linear):
        self.scale = scale
        self.setRange(coord_min, coord_max)

    def setRange(self, coord_min, coord_max):
        self.coord_min = coord_min
        self.coord_max = coord_max
        self.coord_clipped_min = max(1e-20, coord_min)
        self.coord_clipped_max = max(self.coord_clipped_min, coord_max)
        self.coord_ratio_log = np.log10(self.coord_clipped_max / self.coord_clipped_min)

    def setScale(self, scale):
        self.scale = scale

    def toScreen(self, x):
        if self.scale is fscales.Logarithmic:
            if self.coord_clipped_min == self.coord_clipped_max:
                return 0 + 0. * x
            x = (x < 1e-20) * 1e-20 + (x >= 1e-20) * x
            return np.log10(x / self.coord_clipped_min) * 1 / self.coord_ratio_log + 0
        if self.coord_max == self.coord_min:
            return 0 + 0. * x
        t, t0, t1 = self.scale.transform(x), self.scale.transform(self.coord_min), self.scale.transform(self.coord_max)
        return (t - t0) * 1 / (t1 - t0) + 0


def bin_edges(x):
    """The left and right edge of every bin of a spectrum's frequency vector (spectrumPlotWidget.py:137-142)."""
    x_left = np.zeros(x.shape)
    x_right = np.zeros(x.shape)
    x_left[0] = 1e-10
    x_left[1:] = (x[1:] + x[:-1]) / 2.0
    x_right[:-1] = x_left[1:]
    x_right[-1] = float(SAMPLING_RATE / 2)
    return x_left, x_right


def frequency_to_note(freq):
    if np.isnan(freq) or freq <= 0:
        return ""
    semitone = round(np.log2(freq / 440) * 12) + 9                 # semitones above C4 (A4 = 440 Hz is C4 + 9)
    names = ["C", "C♯", "D", "D♯", "E", "F", "F♯", "G", "G♯", "A", "A♯", "B"]
    return f"{names[semitone % 12]}{int(np.floor(semitone / 12)) + 4}"


def format_frequency(freq):
    """The pitch label text of the reference's format_frequency (friture/pitch_tracker_data.py)."""
    if freq < 1000:
        return f"{freq:.0f} Hz ({frequency_to_note(freq)})"
    return f"{freq / 1000:.1f} kHz ({frequency_to_note(freq)})"


def fmax_text(fmax):
    return "%.1f Hz" % fmax if fmax < 2e2 else "%d Hz" % np.rint(fmax)


def reset_state(bins, streams=None):
    """The state compute_peaks resets to on a bin-count change: peak -500, int 0, decay c; [3, B] or [S, 3, B]."""
    st = np.empty((3, bins))
    st[0], st[1], st[2] = np.ones(bins) * PEAK_RESET, 0.0, np.ones(bins) * 20.0 * np.log10(PEAK_DECAY_RATE) * 5000
    return st if streams is None else np.repeat(st[None], streams, axis=0)


def initial_state(bins, streams=None):
    """What a fresh widget's first compute_peaks of `bins` bins starts from: its three-element initial state (zeros, zeros,
    PEAK_DECAY_RATE) is kept when bins == 3, reset otherwise."""
    if bins != 3:
        return reset_state(bins, streams)
    st = np.array([np.zeros(3), np.zeros(3), np.ones(3) * PEAK_DECAY_RATE])
    return st if streams is None else np.repeat(st[None], streams, axis=0)


def _run(y, dtype, S, R, B, ld_r, ld_s, cmin, cmax, state, peaks, keep_last, sy, z, sp, zp):
    lib = _lib.init()
    _lib.check(lib.frt_curves_run(y, dtype, S, R, B, ld_r, ld_s, float(cmin), float(cmax), _ptr(state), int(peaks), int(keep_last),
                                  _ptr(sy), _ptr(z), _ptr(sp), _ptr(zp)))


class _Curves:
    """What both widgets share: the vertical transform, the peak state (on the device) and the one call per refresh."""

    def __init__(self):
        self.paused = False
        self.vertical = ScreenTransform(0, 1)
        self._state_host = initial_state(3)             # the widgets' three-element initial state, uploaded on first use
        self._state = None
        self.signal = None
        self.peak = None

    def setspecrange(self, spec_min, spec_max):
        if spec_min > spec_max:
            spec_min, spec_max = spec_max, spec_min
        self.vertical.setRange(spec_min, spec_max)

    def pause(self):
        self.paused = True

    def restart(self):
        self.paused = False

    def peak_state(self):
        """(peak, peak_int, peak_decay) as the widget holds them."""
        st = self._state_host if self._state is None else self._state.cpu().numpy()
        return st[0].copy(), st[1].copy(), st[2].copy()

    def _curves(self, y, peaks):
        """scaled_y, z and (peaks) scaled_peak, z_peak of one refresh; the state is reset on a bin-count change."""
        import torch
        y = np.ascontiguousarray(y)
        if y.dtype not in (np.float32, np.float64):
            y = y.astype(np.float64)
        B = y.shape[0]
        if peaks:
            if self._state is None or self._state.shape[1] != B:
                st = self._state_host if self._state is None and B == 3 else reset_state(B)
                self._state = torch.from_numpy(np.ascontiguousarray(st)).cuda()
        out = np.empty((4 if peaks else 2, B))
        _run(y.ctypes.data, int(y.dtype == np.float64), 1, 1, B, B, B, self.vertical.coord_min, self.vertical.coord_max,
             self._state if peaks else None, peaks, 1, out[0], out[1], out[2] if peaks else None, out[3] if peaks else None)
        return out


class SpectrumPlot(_Curves):
    """SpectrumPlotWidget without Qt.  After setdata: `signal` and `peak` hold the arguments of the two
    FilledCurve.setData calls (scaled_x_left, scaled_x_right, scaled_y, z, baseline); `fmax_label` and `fpitch_label` hold
    (text, screen position) as setFmax / setFpitch receive them.  `peak` keeps its last value while peaks are disabled."""

    def __init__(self):
        super().__init__()
        self.horizontal = ScreenTransform(0, 22000)
        self.peaks_enabled = True
        self.baseline_data_units = False
        self.fmax_label = None
        self.fpitch_label = None
        self._edges = None

    def setfreqscale(self, scale):
        self.horizontal.setScale(scale)
        self._edges = None

    def setfreqrange(self, minfreq, maxfreq):
        self.xmin, self.xmax = minfreq, maxfreq
        self.horizontal.setRange(minfreq, maxfreq)
        self._edges = None

    def set_peaks_enabled(self, enabled):
        self.peaks_enabled = enabled

    def set_baseline_displayUnits(self, baseline=0.):
        self.baseline_data_units = False

    def set_baseline_dataUnits(self, baseline=0.):
        self.baseline_data_units = True

    def screen_edges(self, x):
        """(scaled_x_left, scaled_x_right) of a frequency vector; cached until x, the scale or the range changes."""
        if self._edges is None or self._edges[0].shape != x.shape or not np.array_equal(self._edges[0], x):
            xl, xr = bin_edges(x)
            self._edges = (np.array(x, copy=True), self.horizontal.toScreen(xl), self.horizontal.toScreen(xr))
        return self._edges[1], self._edges[2]

    def setdata(self, x, y, fmax, fpitch):
        if self.paused:
            return
        self.fmax_label = (fmax_text(fmax), self.horizontal.toScreen(fmax))
        self.fpitch_label = (format_frequency(fpitch), self.horizontal.toScreen(fpitch))
        sxl, sxr = self.screen_edges(x)
        baseline = 1.0 - self.vertical.toScreen(0.0) if self.baseline_data_units else 1.0
        out = self._curves(y, self.peaks_enabled)
        self.signal = (sxl, sxr, out[0], out[1], baseline)
        if self.peaks_enabled:
            self.peak = (sxl, sxr, out[2], out[3], baseline)


class HistPlot(_Curves):
    """HistPlot without Qt.  After setdata: `signal`, `peak` as SpectrumPlot's, and `bar_labels` = (bar_label_x, fc, scaled_y)
    as setBarLabels receives them."""

    def __init__(self):
        super().__init__()
        self.horizontal = ScreenTransform(HIST_FMIN, HIST_FMAX, fscales.Logarithmic)
        self.bar_labels = None
        self._edges = None

    def screen_edges(self, fl, fh):
        e = self._edges
        if e is None or e[0].shape != fl.shape or not (np.array_equal(e[0], fl) and np.array_equal(e[1], fh)):
            sxl, sxr = self.horizontal.toScreen(fl), self.horizontal.toScreen(fh)
            self._edges = (np.array(fl, copy=True), np.array(fh, copy=True), sxl, sxr, (sxl + sxr) / 2)
        return self._edges[2:]

    def setdata(self, fl, fh, fc, y):
        if self.paused:
            return
        sxl, sxr, bx = self.screen_edges(np.asarray(fl), np.asarray(fh))
        scaled_y, z, scaled_peak, z_peak = self._curves(y, True)
        self.signal = (sxl, sxr, scaled_y, z, 1.)
        self.peak = (sxl, sxr, scaled_peak, z_peak, 1.)
        self.bar_labels = (bx, fc, scaled_y)


class CurveResult(NamedTuple):
    scaled_y: object        # [S, R', B] float64 (R' = R, or 1 with keep="last"); [R', B] for a [R, B] input
    z: object
    scaled_peak: object
    z_peak: object
    state: object           # [S, 3, B] float64: peak, peak_int, peak_decay after the last refresh ([3, B] for a [R, B] input)


class CurveBatch:
    """S streams x R refreshes x B bins of dB rows in one call: the widgets' signal and peak curves at a fixed spec range, peaks
    on, no pause.  run(y, state=None, keep="all" | "last") takes a [S, R, B] or [R, B] float32/float64 numpy array or CUDA
    tensor (FirBank.energies(..., as_db=True) output is read in place; rows and streams may be strided, bins contiguous).
    state: None starts as a fresh widget does (initial_state), else a [S, 3, B] array carried from an earlier run (not
    modified).  Results are numpy for numpy input and CUDA tensors for CUDA input."""

    def __init__(self, spec_min=0, spec_max=1):
        if spec_min > spec_max:
            spec_min, spec_max = spec_max, spec_min
        self.spec_min, self.spec_max = spec_min, spec_max

    def run(self, y, state=None, keep="all"):
        assert keep in ("all", "last")
        squeeze = y.ndim == 2
        if squeeze:
            y = y[None]
        S, R, B = y.shape
        Ro = R if keep == "all" else 1
        y, ptr, dtype, (ld_s, ld_r, _) = _batchio.source(y, strided=True)
        if isinstance(y, np.ndarray):
            st = initial_state(B, S) if state is None else np.array(np.asarray(state).reshape(S, 3, B), np.float64, copy=True)
        else:
            import torch
            if state is None:                           # built on the device: nothing goes up
                st = torch.empty((S, 3, B), dtype=torch.float64, device=y.device)
                fresh = initial_state(B)
                for i in range(3):
                    st[:, i] = float(fresh[i, 0])
            else:
                st = torch.as_tensor(state, dtype=torch.float64).to(y.device).reshape(S, 3, B).clone()
        outs = [_batchio.alloc(y, (S, Ro, B)) for _ in range(4)]
        _run(ptr, dtype, S, R, B, ld_r, ld_s, self.spec_min, self.spec_max, st, True, keep == "last", *outs)
        if squeeze:
            outs, st = [o[0] for o in outs], st[0]
        return CurveResult(*outs, st)
