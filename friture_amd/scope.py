"""The oscilloscope of friture/scope.py (Scope_Widget) without Qt, on the GPU (scope.hip, frt_scope_run).

Trigger mode (timerange <= 500 ms): the widget reads 2 x width samples, finds the first rising edge of channel 0 through
(max * 2.) / 3. in the middle width samples, and shows the 2 (width // 2) samples around it; without an edge it keeps what it
showed.  Scrolling mode (timerange > 500 ms): the last width samples.  `Scope` is the widget's handle_new_data (one device call
and one synchronisation per refresh); `ScopeBatch` runs S streams x C rows x T samples refreshed at a schedule of stream ends
in one call."""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _batchio, _lib
from ._batchio import chunk_ends
from .constants import SAMPLING_RATE

SMOOTH_DISPLAY_TIMER_PERIOD_MS = 25                   # scope.py:30
DEFAULT_TIMERANGE = 2 * SMOOTH_DISPLAY_TIMER_PERIOD_MS
SCROLLING_THRESHOLD_MS = 500.0
NO_TRIGGER = -(1 << 63)                               # FRT_SCOPE_NO_TRIGGER
TRACE_RAW, TRACE_SCALED = 1, 2                        # FRT_SCOPE_TRACE_*
_KINDS = {None: 0, "raw": TRACE_RAW, "scaled": TRACE_SCALED}


def width_for(timerange):
    """scope.py:79-80, host arithmetic as the reference rounds it (25.3 ms -> 1214, 10.9 ms -> 523)."""
    time = timerange * 1e-3
    return int(time * SAMPLING_RATE)


def is_scrolling(timerange):
    return timerange > SCROLLING_THRESHOLD_MS


def trace_length(width, scrolling):
    return width if scrolling else 2 * (width // 2)


def time_axis(width, timerange, length):
    """scope.py:126-128: (time, scaled_t) of a trace of `length` samples; depends only on the width and the timerange."""
    time = (np.arange(length) - width // 2) / float(SAMPLING_RATE)
    return time, (time * 1e3 + timerange / 2.) / timerange


def _run(x, dtype, streams, rows, n, ld_row, ld_stream, ends, width, scrolling, start, trace, kind):
    lib = _lib.init()
    ends = np.ascontiguousarray(ends, np.int64)
    _lib.check(lib.frt_scope_run(x, dtype, streams, rows, n, ld_row, ld_stream, ends.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                 ends.shape[0], width, int(scrolling), start, trace, kind))


class Scope:
    """Scope_Widget.handle_new_data (scope.py:78-135).  set_buffer takes the audio buffer the widget reads (anything with
    data(length): a RingBuffer, a DeviceRingBuffer, Friture's AudioBuffer).  After a refresh: time, y, y2 (None for one
    channel) as the widget holds them, and scaled_t, scaled_y, scaled_y2 as the curves last received them (Curve.setData);
    `triggered` says whether this refresh drew, `trace_start` where its trace starts in the window it read."""

    def __init__(self):
        self.audiobuffer = None
        self.set_timerange(DEFAULT_TIMERANGE)
        self.time = np.zeros(10)
        self.y = np.zeros(10)
        self.y2 = np.zeros(10)
        self.scaled_t = np.zeros(10)
        self.scaled_y = np.zeros(10)
        self.scaled_y2 = np.zeros(10)
        self.triggered = False
        self.trace_start = None
        self._axis = None

    def set_buffer(self, buffer):
        self.audiobuffer = buffer

    def set_timerange(self, timerange):
        self.timerange = timerange

    def handle_new_data(self, floatdata):
        width = width_for(self.timerange)
        two = floatdata.shape[0] > 1
        rows = 2 if two else 1
        scrolling = is_scrolling(self.timerange)
        window = self.audiobuffer.data(width if scrolling else 2 * width)[:rows]
        n = window.shape[1]
        L = trace_length(width, scrolling)
        start = np.empty(1, np.int64)
        trace = np.empty((2, rows, L))
        if isinstance(window, np.ndarray):                # host ring: one staged call
            window = np.ascontiguousarray(window, np.float64)
            ptr, dtype, ld = window.ctypes.data, 1, n
        else:                                             # DeviceRingBuffer: the view's device address, nothing goes up
            assert window.is_cuda and window.stride(1) == 1
            ptr, dtype, ld = window.data_ptr(), 0 if str(window.dtype) == "torch.float32" else 1, window.stride(0)
        _run(ptr if n else None, dtype, 1, rows, n, ld, 0, [n], width, scrolling, start.ctypes.data, trace.ctypes.data,
             TRACE_RAW | TRACE_SCALED)
        self.triggered = bool(start[0] != NO_TRIGGER)
        if not self.triggered:
            self.trace_start = None
            return                                        # scope.py:111-112: the previous curves stay
        self.trace_start = int(start[0])
        self.y = trace[0, 0]
        self.y2 = trace[0, 1] if two else None
        if self._axis is None or self._axis[:2] != (width, self.timerange):
            self._axis = (width, self.timerange) + time_axis(width, self.timerange, L)
        self.time, self.scaled_t = self._axis[2], self._axis[3]
        self.scaled_y = trace[1, 0]
        if two:
            self.scaled_y2 = trace[1, 1]


class ScopeResult(NamedTuple):
    starts: object          # [S, K] int64 (or [K] for a [C, T] input): absolute index of each trace's first sample
    triggered: object       # [S, K] bool: the refresh drew (always True in scrolling mode)
    traces: object          # [S, C, K, L] float64 (or [C, K, L]), or None; slots of refreshes without a trigger hold zeros

    def carry_forward(self):
        """What the widget shows after each refresh: (src, shown).  src[..., k] is the last refresh <= k that triggered, -1
        while the widget still shows its initial zeros(10); shown[..., k, :] is that refresh's trace (zeros where src < 0)."""
        trig = np.asarray(self.triggered.cpu() if hasattr(self.triggered, "cpu") else self.triggered)
        K = trig.shape[-1]
        src = np.where(trig, np.arange(K), -1)
        src = np.maximum.accumulate(src, axis=-1)
        if self.traces is None:
            return src, None
        tr = np.asarray(self.traces.cpu() if hasattr(self.traces, "cpu") else self.traces)
        idx = np.maximum(src, 0)
        if tr.ndim == 3:                                 # [C, K, L]
            shown = tr[:, idx, :]
            shown[:, src < 0, :] = 0.0
        else:                                            # [S, C, K, L]
            shown = np.take_along_axis(tr, idx[:, None, :, None], axis=2)
            shown = np.where((src < 0)[:, None, :, None], 0.0, shown)
        return src, shown


class ScopeBatch:
    """S streams x C rows x T samples refreshed at a schedule, in one call: the batch form of Scope at a fixed timerange.
    run(x, chunk=512 | ends=..., traces=None | "raw" | "scaled") takes a [S, C, T] or [C, T] float32/float64 numpy array
    or CUDA tensor (rows may be strided); the refresh k sees the stream up to ends[k] (default: the ends of `chunk`-sample
    chunks), zeros before its start — the widget's ring has lost nothing by its first refresh, so this is what a widget fed
    chunk by chunk computes.  Results are numpy for numpy input and CUDA tensors for CUDA input."""

    def __init__(self, timerange_ms=DEFAULT_TIMERANGE):
        self.timerange = timerange_ms
        self.width = width_for(timerange_ms)
        self.scrolling = is_scrolling(timerange_ms)
        self.length = trace_length(self.width, self.scrolling)

    def time_axis(self):
        return time_axis(self.width, self.timerange, self.length)

    def run(self, x, chunk=512, ends=None, traces=None):
        kind = _KINDS[traces]
        squeeze = x.ndim == 2
        if squeeze:
            x = x[None]
        S, C, T = x.shape
        ends = chunk_ends(T, chunk) if ends is None else np.asarray(ends, np.int64)
        K, L = ends.shape[0], self.length
        if isinstance(x, np.ndarray):
            x = np.ascontiguousarray(x)                  # host input is staged whole; a CUDA tensor's rows may stay strided
        x, ptr, dtype, (ld_stream, ld_row, _) = _batchio.source(x, strided=True)
        starts = _batchio.alloc(x, (S, K), np.int64)
        tr = _batchio.alloc(x, (S, C, K, L), zero=True) if kind else None
        sp, tp = _batchio.ptr(starts), _batchio.ptr(tr)
        _run(ptr if T else None, dtype, S, C, T, ld_row, ld_stream, ends, self.width, self.scrolling, sp, tp, kind)
        trig = starts != NO_TRIGGER
        if squeeze:
            starts, trig, tr = starts[0], trig[0], (tr[0] if kind else None)
        return ScopeResult(starts, trig, tr)
