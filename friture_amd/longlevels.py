"""The long-time level history of friture/longlevels.py (LongLevelWidget) without Qt, on the GPU (levels.hip).

Per complete block of 2^Ndec samples of channel 0: y^2 -> Ndec x (FIR gauss(11, 2), [::2]) -> FIR gauss(41, 8) with carried
state -> 10 log10(max(level, 1e-150)) -> the widget's ring buffer -> the curve.  The decimation stages, the FIR and the dB
run in one device call per chunk; the ring and the curve's read-out are the reference's host code."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .constants import SAMPLING_RATE
from .levels import _Handle, ndec_for
from .ringbuffer import RingBuffer

DEFAULT_MAXTIME = 600          # longlevels_settings.py:23-27
DEFAULT_LEVEL_MIN = -70
DEFAULT_LEVEL_MAX = -20
DEFAULT_RESPONSE_TIME = 20


def gauss(n=11, sigma=1):
    """longlevels.py:49-51"""
    r = range(-int(n/2), int(n/2)+1)
    return [1 / (sigma * np.sqrt(2*np.pi)) * np.exp(-float(x)**2/(2*sigma**2)) for x in r]


class Subsampler:
    """longlevels.py:54-91: push(x) runs x through Ndec stages of (FIR gauss(11, 2), [::2]) with the stage states carried;
    [::2] keeps index 0 of each push at every stage.  One device call per push."""

    def __init__(self, Ndec):
        self.Ndec = Ndec
        self._h = _Handle(1, Ndec, 1)

    def push(self, x):
        if x.size == 0:
            return x
        x = np.ascontiguousarray(x, np.float64)
        lib = self._h.lib
        m = int(lib.frt_levels_subsample_length(self._h.h, x.shape[0]))
        out = np.empty(m)
        got = ctypes.c_int64(0)
        _lib.check(lib.frt_levels_subsample(self._h.h, x.ctypes.data, 1, x.shape[0], x.shape[0], out.ctypes.data, ctypes.byref(got)))
        return out


class LongLevels:
    """LongLevelWidget (longlevels.py:94-232) without Qt.  handle_new_data(floatdata) takes the chunk the widget's audio
    buffer received; curve() returns the last (scaled_t, scaled_y) the widget handed to its Curve (None before the first
    complete block); level_rms is the last block's dB value."""

    def __init__(self, response_time=DEFAULT_RESPONSE_TIME, length_seconds=DEFAULT_MAXTIME):
        self.level_min = DEFAULT_LEVEL_MIN
        self.level_max = DEFAULT_LEVEL_MAX
        self.level = None
        self.level_rms = -200.
        self._h = None
        self._curve = None
        self.length_seconds = length_seconds
        self.setresptime(response_time)
        self.ringbuffer = RingBuffer()

    def handle_new_data(self, floatdata):
        _, lo = self._h.push(floatdata[0:1], meters=False, long=True)
        nb = lo.shape[1]
        if nb > 0:
            self.level = lo[0, -1, 0]
            self.level_rms = lo[0, -1, 1]
            self.ringbuffer.push(np.ascontiguousarray(lo[0:1, :, 1]), 0)
            self.time = np.arange(self.length_samples) / self.subsampled_sampling_rate
            levels = self.ringbuffer.data(self.length_samples)
            scaled_t = self.time / self.length_seconds
            scaled_y = np.clip(1. - (levels[0, :] - self.level_min) / (self.level_max - self.level_min), 0., 1.)
            self._curve = (scaled_t, scaled_y)
        return lo

    def curve(self):
        return self._curve

    def setmin(self, value):
        self.level_min = value

    def setmax(self, value):
        self.level_max = value

    def setduration(self, value):
        self.length_seconds = value
        self.length_samples = int(self.length_seconds * self.subsampled_sampling_rate)

    def setresptime(self, value):
        self.response_time = value
        self.Ndec = ndec_for(value)
        self.subsampled_sampling_rate = SAMPLING_RATE / 2 ** (self.Ndec)
        if self._h is None:
            self._h = _Handle(1, self.Ndec, 1)
        else:
            self._h.set_ndec(self.Ndec)      # new subsampler and FIR state; the samples not yet consumed are kept
        if self.length_seconds:
            self.setduration(self.length_seconds)
