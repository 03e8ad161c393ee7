"""Recordings at other sample rates for the 48 kHz chains: a rational-ratio polyphase sample-rate converter on the GPU
(resample.hip, frt_resample_*).

Every chain of the package assumes SAMPLING_RATE; `Resampler(rate_in)` reads [S, T] at any integer rate and writes [S, T'] at
SAMPLING_RATE, state carried across calls like the batch classes.  With g = gcd(rate_in, rate_out): L = rate_out / g,
M = rate_in / g, Q = max(L, M), C = zeros * Q.  The prototype h[0 .. 2C] is a Kaiser-windowed sinc whose stop band begins at the
narrower of the two Nyquist frequencies (nothing folds back), scaled to sum L; the output is zero-phase,

    y[m] = sum_k h[C + m M - k L] x[k]        over every k with 0 <= C + m M - k L <= 2C, x[k] = 0 outside the stream,

K = ceil((2C + 1) / L) taps per output from the first input kb(m) = ceil((m M - C) / L) on.  After N inputs a stream that is not
flushed has emitted max(0, ceil((N L - C) / M)) outputs (those whose taps have all arrived), a flushed one ceil(N L / M) (later
inputs are zeros); the carried tail is the last K - 1 inputs.  There is no CPU fallback: run() goes to the HIP library."""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import numpy as np

from . import _batchio, _lib
from .constants import SAMPLING_RATE

MAX_COEFFICIENTS = 1 << 20                  # L * K, the device table (frt_resample_create refuses more)

ResampleState = namedtuple("ResampleState", "tail n_in n_out")      # tail [S, K - 1] float64; inputs taken, outputs emitted
ResampleResult = namedtuple("ResampleResult", "y state")


def _positive_int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} must be a positive integer, got {v!r}")
    return int(v)


def _dtype_name(d):
    return str(d).split(".")[-1] if type(d).__module__.startswith("torch") else np.dtype(d).name


class Resampler:
    """run(x, state=None, flush=True, dtype=None) -> ResampleResult(y, state).  x: [S, T] ([T]: one stream), float32 or float64,
    numpy array or CUDA tensor (rows read in place); y: [S, T'] of the same kind, in x's dtype unless `dtype` says otherwise.
    Arithmetic is float64 whatever the dtypes; a float32 output is one rounding of the float64 sum.  flush=False keeps the
    outputs whose taps reach past the end for the next call, which continues with `state`; a recording cut into calls gives the
    bits of one call.  After flush=True the state is final."""

    def __init__(self, rate_in, rate_out=SAMPLING_RATE, zeros=64, attenuation_db=100.0):
        self.rate_in, self.rate_out = _positive_int("rate_in", rate_in), _positive_int("rate_out", rate_out)
        self.zeros = _positive_int("zeros", zeros)
        if self.rate_in == self.rate_out:
            raise ValueError(f"rate_in == rate_out == {self.rate_in}: nothing to resample")
        if not attenuation_db > 21.0:
            raise ValueError(f"attenuation_db {attenuation_db!r} (above 21, where the Kaiser formulas hold)")
        g = math.gcd(self.rate_in, self.rate_out)
        self.L, self.M = self.rate_out // g, self.rate_in // g
        self.Q = max(self.L, self.M)
        self.C = self.zeros * self.Q
        self.K = -(-(2 * self.C + 1) // self.L)
        if self.L * self.K > MAX_COEFFICIENTS:
            raise ValueError(f"{self.rate_in} -> {self.rate_out}: L * K = {self.L} * {self.K} coefficients (at most {MAX_COEFFICIENTS})")
        self.attenuation_db = float(attenuation_db)
        self.beta = 0.1102 * (self.attenuation_db - 8.7)
        self.dw = (self.attenuation_db - 8) / (2.285 * 2 * self.C)                 # transition width, rad/sample
        self.fc = 0.5 / self.Q - self.dw / (4 * np.pi)                             # cycles/sample: the middle of the transition
        n = np.arange(2 * self.C + 1, dtype=np.float64)
        h = 2 * self.fc * np.sinc(2 * self.fc * (n - self.C)) * np.kaiser(2 * self.C + 1, self.beta)
        self.prototype = np.ascontiguousarray(h * (self.L / np.sum(h)), np.float64)
        self._handles = {}

    # ---- host only ------------------------------------------------------------------------------------------------------------
    @property
    def latency_in(self):
        """The group delay of the prototype in input samples."""
        return self.C / self.L

    def n_out(self, n_in, flush=True):
        """Outputs emitted after n_in inputs in total."""
        n_in = int(n_in)
        if flush:
            return -(-(n_in * self.L) // self.M)
        return max(0, -(-(n_in * self.L - self.C) // self.M))

    def _check_state(self, state, S):
        if state is None:
            return None, 0, 0
        tail, n_in, n_out = state
        if tuple(tail.shape) != (S, self.K - 1):
            raise ValueError(f"state of another shape: tail {tuple(tail.shape)} (want {(S, self.K - 1)})")
        n_in, n_out = int(n_in), int(n_out)
        if n_in < 0 or n_out != self.n_out(n_in, False):
            if n_in >= 0 and n_out == self.n_out(n_in, True):
                raise ValueError("the state is final: it was flushed")
            raise ValueError(f"state of another stream: {n_out} outputs after {n_in} inputs")
        return tail, n_in, n_out

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def _handle(self, S):
        if S not in self._handles:
            self._handles[S] = _lib.Handle("resample", self.L, self.M, self.C, self.prototype.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), S)
        return self._handles[S]

    def run(self, x, state=None, flush=True, dtype=None):
        x, is_np, squeeze, _ = _batchio.check_samples("Resampler", x, None)
        S, T = x.shape
        out_name = _dtype_name(x.dtype if dtype is None else dtype)
        if out_name not in ("float32", "float64"):
            raise TypeError(f"dtype must be float32 or float64, got {dtype}")
        tail, n_in, n_out = self._check_state(state, S)
        total = self.n_out(n_in + T, flush)
        n_new, Kt = total - n_out, self.K - 1
        h = self._handle(S)
        x, xptr, code, ld, _ = _batchio.strided_rows(x)
        vp = ctypes.c_void_p

        def call(tail_in, y, tail_out):
            _lib.check(h.lib.frt_resample_run(h.h, vp(xptr) if T else None, code, T, ld, vp(_batchio.ptr(tail_in)), vp(_batchio.ptr(tail_out)),
                                              n_in, n_out, n_new, vp(_batchio.ptr(y)) if n_new else None,
                                              int(out_name == "float64"), max(n_new, 1)))

        # a fresh stream starts from a zero tail on the device, and a carried one is copied
        y, tail_out = _batchio.run_call(x, is_np, lambda: (_batchio.alloc(x, (S, n_new), out_name), _batchio.alloc(x, (S, Kt))), h.set_stream,
                                        call, tail, device_state=lambda dev, tail: _batchio.carried(dev, tail, (S, Kt)))
        return ResampleResult(y[0] if squeeze else y, ResampleState(tail_out, n_in + T, total))


def to_48k(x, rate_in):
    """x at SAMPLING_RATE: x itself when rate_in is SAMPLING_RATE already, otherwise Resampler(rate_in).run(x).y."""
    if _positive_int("rate_in", rate_in) == SAMPLING_RATE:
        return x
    return Resampler(rate_in).run(x).y
