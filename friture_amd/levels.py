"""The level meters of friture/levels.py (Levels_Widget) without Qt, on the GPU (levels.hip, frt_levels_*).

Per channel and chunk: the peak hold/decay of max|y|, the exponentially smoothed RMS of y^2 (exp_smoothed_value), their
dB values, dB_to_IEC and the BallisticPeak hold-then-decay machine (friture/ballistic_peak.py).  `Levels` is the widget's
handle_new_data for one or two channels (one device round trip per chunk); `LevelsBatch` runs C channels x T samples cut
into chunks, plus the long-time levels of friture/longlevels.py, in one call."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _batchio, _lib
from .constants import SAMPLING_RATE

SMOOTH_DISPLAY_TIMER_PERIOD_MS = 25        # levels.py:30
PEAK_DECAY_RATE = (1.0 - 3E-6/500.)        # ballistic_peak.py:22
PEAK_FALLOFF = 32                          # ballistic_peak.py:24
FIELDS = 6                                 # FRT_LEVELS_METER_FIELDS: rms, old_max, level_rms, level_max, peak_iec, branch
FOLLOW, HOLD, DECAY, DECAY_FLOOR = 0, 1, 2, 3
BRANCH_NAMES = ("follow", "hold", "decay", "decay_floor")
DEFAULT_HISTORY_SECONDS = 600              # longlevels_settings.py:23 (DEFAULT_MAXTIME)

_DP = ctypes.POINTER(ctypes.c_double)


def meter_coefficients():
    """levels.py:57-74, as the reference computes them: (alpha, kernel, alpha2)."""
    response_time = 0.300
    w = 0.65
    n = response_time * SAMPLING_RATE
    N = 5*n
    alpha = 1. - (1. - w) ** (1. / (n + 1))
    kernel = (1. - alpha) ** (np.arange(0, N)[::-1])
    response_time_peaks = 0.025
    n2 = response_time_peaks / (SMOOTH_DISPLAY_TIMER_PERIOD_MS / 1000.)
    alpha2 = 1. - (1. - w) ** (1. / (n2 + 1))
    return alpha, np.ascontiguousarray(kernel, np.float64), alpha2


def ndec_for(response_time):
    """longlevels.py:215: how many times to decimate to end up with 100 points in the kernel."""
    return int(max(0, np.floor((np.log2(response_time * SAMPLING_RATE/100.)))))


class _Handle(_lib.Handle):
    """One frt_levels object: channels, Ndec, ring of history_len entries."""

    def __init__(self, channels, ndec, history_len, kernel=None, alpha=0.0, alpha2=0.0):
        from .longlevels import gauss
        if kernel is None:
            kernel = np.zeros(1)
        self._kernel = np.ascontiguousarray(kernel, np.float64)
        g11 = np.ascontiguousarray(gauss(11, 2.), np.float64)
        g41 = np.ascontiguousarray(gauss(10*4+1, 2.*4), np.float64)
        self.channels = channels
        super().__init__("levels", channels, ndec, int(history_len), self._kernel.ctypes.data_as(_DP), self._kernel.shape[0], float(alpha),
                         float(alpha2), g11.ctypes.data_as(_DP), g41.ctypes.data_as(_DP), PEAK_DECAY_RATE)

    def set_ndec(self, ndec):
        _lib.check(self.lib.frt_levels_set_ndec(self.h, int(ndec)))

    def reset(self):
        _lib.check(self.lib.frt_levels_reset(self.h))

    def get_state(self):
        s = np.empty(self.lib.frt_levels_state_length(self.h), np.float64)
        _lib.check(self.lib.frt_levels_get_state(self.h, s.ctypes.data_as(_DP)))
        return s

    def set_state(self, s):
        s = np.ascontiguousarray(s, np.float64)
        assert s.shape == (self.lib.frt_levels_state_length(self.h),)
        _lib.check(self.lib.frt_levels_set_state(self.h, s.ctypes.data_as(_DP)))

    def blocks_for(self, n):
        return int(self.lib.frt_levels_blocks_for(self.h, int(n)))

    def push(self, x, meters=True, long=False):
        """x: [nch][n] float64 host; returns (meters [nch][FIELDS] or None, long [nch][nb][2] or None)."""
        x = np.ascontiguousarray(x, np.float64)
        nch, n = x.shape
        m = np.empty((nch, FIELDS)) if meters else None
        nb = self.blocks_for(n) if long else 0
        lo = np.empty((nch, nb, 2)) if long else None
        got = ctypes.c_int64(0)
        _lib.check(self.lib.frt_levels_push(self.h, x.ctypes.data if n else None, nch, n, m.ctypes.data if meters else None,
                                            lo.ctypes.data if long else None, ctypes.byref(got)))
        assert got.value == nb
        return m, lo

    def history(self, count):
        out = np.empty((self.channels, int(count)))
        _lib.check(self.lib.frt_levels_history(self.h, int(count), out.ctypes.data))
        return out


class Levels:
    """Levels_Widget.handle_new_data (levels.py:85-124) for channel 0 and, when the chunk has more than one, channel 1.
    After a call: level_rms, level_max, peak_iec (channel 0), level_rms_2, level_max_2, peak_iec_2 (channel 1, while
    two_channels), and `branch` / `branch_2`, the BallisticPeak branch each took."""

    def __init__(self):
        self.alpha, self.kernel, self.alpha2 = meter_coefficients()
        self._h = _Handle(2, 13, 1, self.kernel, self.alpha, self.alpha2)
        self.two_channels = False
        self.level_rms = self.level_max = self.peak_iec = None
        self.level_rms_2 = self.level_max_2 = self.peak_iec_2 = None
        self.branch = self.branch_2 = None

    def handle_new_data(self, floatdata):
        if floatdata.shape[0] > 1 and not self.two_channels:
            self.two_channels = True
        elif floatdata.shape[0] == 1 and self.two_channels:
            self.two_channels = False
        nch = 2 if self.two_channels else 1
        m, _ = self._h.push(floatdata[:nch])
        self.level_rms, self.level_max, self.peak_iec, self.branch = float(m[0, 2]), float(m[0, 3]), float(m[0, 4]), int(m[0, 5])
        if self.two_channels:
            self.level_rms_2, self.level_max_2, self.peak_iec_2, self.branch_2 = (float(m[1, 2]), float(m[1, 3]), float(m[1, 4]),
                                                                                  int(m[1, 5]))
        return m

    def get_state(self):
        return self._h.get_state()

    def set_state(self, s):
        self._h.set_state(s)


class LevelsBatch:
    """C channels x T samples per call, cut into chunks of `chunk` samples (a short last chunk is a short chunk): the
    meters of every chunk and the long-time level of every complete block of 2^Ndec samples, state carried across calls.
    run(x) takes a [C, T] float32/float64 numpy array or CUDA tensor and returns (meters [C, nchunks, FIELDS],
    long [C, nblocks, 2] = {level, dB}) of the same kind."""

    def __init__(self, channels, response_time=20, chunk=512, history_seconds=DEFAULT_HISTORY_SECONDS):
        self.channels, self.chunk = channels, int(chunk)
        self.alpha, self.kernel, self.alpha2 = meter_coefficients()
        self.ndec = ndec_for(response_time)
        self.history_len = int(history_seconds * SAMPLING_RATE / 2 ** self.ndec)
        self._h = _Handle(channels, self.ndec, self.history_len, self.kernel, self.alpha, self.alpha2)

    def run(self, x, meters=True, long=True):
        h = self._h
        assert x.ndim == 2 and x.shape[0] == self.channels
        x, ptr, dtype, _ = _batchio.source(x, strided=False)
        n = x.shape[1]
        nb = h.blocks_for(n) if long else 0
        m = _batchio.alloc(x, (self.channels, -(-n // self.chunk), FIELDS)) if meters else None
        lo = _batchio.alloc(x, (self.channels, nb, 2)) if long else None
        if not isinstance(x, np.ndarray):
            import torch
            h.set_stream(ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
        got = ctypes.c_int64(0)
        _lib.check(h.lib.frt_levels_run(h.h, ptr if n else None, dtype, n, n, self.chunk, _batchio.ptr(m), _batchio.ptr(lo),
                                        ctypes.byref(got)))
        assert got.value == nb
        return m, lo

    def history(self, count=None):
        """The last `count` (default: all) long-level dB values per channel, oldest first (0 before the first block)."""
        return self._h.history(self.history_len if count is None else count)

    def get_state(self):
        return self._h.get_state()

    def set_state(self, s):
        self._h.set_state(s)

    def reset(self):
        self._h.reset()
