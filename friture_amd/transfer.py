"""What a system does to a signal: Welch cross-spectra, the transfer function H1 and the coherence between a reference row
and a measured row, on the GPU (transfer.hip, frt_transfer_*; the definition: X1 in include/friture_hip.h).  The step after
the delay estimator in a loudspeaker or room measurement: find the delay, align, then look at magnitude, phase and coherence.

A stream is a pair of rows at one sample rate (nothing here depends on it): x = row 0, the reference, y = row 1, the measured
signal.  fft_size N is a power of two in 64 .. 8192, hop >= 1 (it may exceed N; default N // 2), window "hann"
(tables.hann_symmetric(N), the STFT's) or N float64 values, average = K >= 1 frames per estimate or None for one running
estimate over everything seen, delay an integer d with |d| <= 96000 samples.  Frame f is x[a + f hop : .. + N] and
y[b + f hop : .. + N] with a = max(0, -d), b = max(0, d): a positive delay means that the measured row lags.  After n samples
in total there are F(n) = max(0, (n - |d| - N) // hop + 1) frames.  Per frame X = rfft(x w) / N and Y = rfft(y w) / N over the
bins 0 .. N/2 (with this scale sxx is the package's PSD).  Estimate e is the mean over its frames of |X|^2 (sxx), |Y|^2 (syy)
and conj(X) Y (sxy, the convention of scipy.signal.csd(x, y)); with average=K it covers the frames e K .. e K + K - 1 and is
emitted by the call in which its last frame completes, with average=None every call that has seen at least one frame returns
one estimate over all frames so far.  The device also writes h1 = sxy / sxx and coherence = |sxy|^2 / (sxx syy), both 0 where
the denominator is 0 (a silent row).  The order of the sums is part of the definition: runs of RUN = 16 consecutive frames on
the estimate's own frame grid (the last may be short), a run summed in frame order, the run sums added in run order, then the
division by the frame count; no atomics, so a recording cut into calls anywhere, any slab size and any batch give the same
bits.  Out of scope: N = 16384, fractional delays, exponential averaging, more than two rows per stream, resampling (to_48k
first).  The impulse response behind h1 and its use on a signal: convolve.impulse_response, convolve.ConvolveBatch (X2).  There
is no CPU fallback: run() goes to the HIP library."""
from __future__ import annotations

import ctypes
import hashlib
from collections import namedtuple

import numpy as np

from . import _batchio, _lib
from .constants import SAMPLING_RATE

RUN = 16                                    # frames per run of the summation order
MIN_FFT_SIZE, MAX_FFT_SIZE = 64, 8192
MAX_DELAY = 96000
MAX_HOP = 1 << 30

# data: one float64 array (its layout: state_layout); pairs; samples taken; pending: unconsumed samples of the reference row;
# settings: those of the TransferBatch that made it
TransferState = namedtuple("TransferState", "data streams n_in pending settings")
TransferResult = namedtuple("TransferResult", "sxx syy sxy h1 coherence frames freq state")


def frames_after(n, fft_size, hop, delay=0):
    """F(n): the frames after n samples in total."""
    return max(0, (int(n) - abs(delay) - fft_size) // hop + 1)


def state_layout(S, fft_size, hop, delay, n_in):
    """name -> (offset, shape) of the parts of a state's data after n_in samples, and its length."""
    F = frames_after(n_in, fft_size, hop, delay)
    a, b, bins = max(0, -delay), max(0, delay), fft_size // 2 + 1
    parts = (("sum", (S, bins * 4)), ("open_run", (S, bins * 4)), ("row0", (S, n_in - min(n_in, a + F * hop))),
             ("row1", (S, n_in - min(n_in, b + F * hop))))
    out, at = {}, 0
    for name, shape in parts:
        out[name] = (at, shape)
        at += shape[0] * shape[1]
    return out, at


def magnitude_db(res):
    """20 log10 |h1| of a TransferResult (-inf where h1 = 0), of its kind."""
    h = res.h1
    if isinstance(h, np.ndarray):
        with np.errstate(divide="ignore"):
            return 20.0 * np.log10(np.abs(h))
    import torch
    return 20.0 * torch.log10(torch.abs(h))


def phase(res):
    """angle(h1) of a TransferResult in radians, of its kind."""
    h = res.h1
    if isinstance(h, np.ndarray):
        return np.angle(h)
    import torch
    return torch.angle(h)


class TransferBatch:
    """run(x, state=None, scratch_bytes=1 << 28) -> TransferResult.  x: [S, 2, T] or [2, T], float32 or float64, numpy array or
    CUDA tensor (strided views are read in place); row 0 is the reference, row 1 the measured signal.  Results are of x's
    kind: sxx, syy, coherence [S, E, bins] float64, sxy, h1 [S, E, bins] complex128 (without the S axis for [2, T]), frames [E]
    int64 (the frames behind each estimate); freq [bins] is a host vector in Hz at SAMPLING_RATE; state continues the streams
    in the next call, and a recording cut into calls at any sample gives the bits of one call.  The launches are cut into
    time slabs whose run partials stay within scratch_bytes; the result has the same bits at any slab size."""

    def __init__(self, fft_size=8192, hop=None, window="hann", average=None, delay=0):
        def integer(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)

        if not integer(fft_size) or fft_size < MIN_FFT_SIZE or fft_size & (fft_size - 1) or fft_size > MAX_FFT_SIZE:
            raise ValueError(f"fft_size must be a power of two in {MIN_FFT_SIZE} .. {MAX_FFT_SIZE}, got {fft_size!r}")
        self.fft_size = int(fft_size)
        hop = self.fft_size // 2 if hop is None else hop
        if not integer(hop) or not 1 <= hop <= MAX_HOP:
            raise ValueError(f"hop must be an integer in 1 .. 2^30, got {hop!r}")
        self.hop = int(hop)
        if average is not None and (not integer(average) or average < 1):
            raise ValueError(f"average must be None or an integer >= 1, got {average!r}")
        self.average = None if average is None else int(average)
        if not integer(delay) or abs(delay) > MAX_DELAY:
            raise ValueError(f"delay must be an integer with |delay| <= {MAX_DELAY}, got {delay!r}")
        self.delay = int(delay)
        if isinstance(window, str):
            if window != "hann":
                raise ValueError(f"window={window!r} ('hann' or {self.fft_size} float64 values)")
            from .tables import hann_symmetric
            self.window, key = np.ascontiguousarray(hann_symmetric(self.fft_size), np.float64), "hann"
        else:
            self.window = np.ascontiguousarray(window, np.float64)
            if self.window.shape != (self.fft_size,) or not np.all(np.isfinite(self.window)):
                raise ValueError(f"window must be {self.fft_size} finite values, got shape {self.window.shape}")
            key = hashlib.sha1(self.window.tobytes()).hexdigest()
        self.bins = self.fft_size // 2 + 1
        self.freq = np.arange(self.bins, dtype=np.float64) * (SAMPLING_RATE / self.fft_size)
        self.settings = (self.fft_size, self.hop, self.average, self.delay, key)
        self._handle_ = None

    # ---- host only ------------------------------------------------------------------------------------------------------------
    def frames_after(self, n):
        """F(n): the frames after n samples in total."""
        return frames_after(n, self.fft_size, self.hop, self.delay)

    def estimates_after(self, n):
        """The estimates emitted by the calls that took a stream to n samples in total (average=None: see emitted)."""
        F = self.frames_after(n)
        return F // self.average if self.average else int(F > 0)

    def emitted(self, n_before, n_after):
        """The estimates a call returns that takes a stream from n_before to n_after samples."""
        if self.average is None:
            return int(self.frames_after(n_after) > 0)
        return self.estimates_after(n_after) - self.estimates_after(n_before)

    def state_parts(self, state):
        """The parts of a state as views of its data: sum and open_run [S, bins, 4] (sxx, syy, Re sxy, Im sxy), row0, row1."""
        layout, _ = state_layout(state.streams, self.fft_size, self.hop, self.delay, int(state.n_in))
        parts = {name: state.data[at:at + shape[0] * shape[1]].reshape(shape) for name, (at, shape) in layout.items()}
        for name in ("sum", "open_run"):
            parts[name] = parts[name].reshape(state.streams, self.bins, 4)
        return parts

    def _check_state(self, state, S):
        if state is None:
            return None, 0
        data, streams, n_in, pending, settings = state
        if tuple(settings) != self.settings:
            raise ValueError(f"state of other settings: {tuple(settings)} (want {self.settings})")
        if int(streams) != S:
            raise ValueError(f"state of another shape: {streams} streams (want {S})")
        n_in = int(n_in)
        layout, want = state_layout(S, self.fft_size, self.hop, self.delay, max(n_in, 0))
        if n_in < 0 or int(pending) != layout["row0"][1][1]:
            raise ValueError(f"state of another stream: {pending} pending samples after {n_in}")
        if data.ndim != 1 or data.shape[0] != want:
            raise ValueError(f"state of another shape: data {tuple(data.shape)} (want {(want,)})")
        return data, n_in

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def _handle(self):
        if self._handle_ is None:
            self._handle_ = _lib.Handle("transfer", self.fft_size, self.hop, self.window.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                        self.average or 0, self.delay)
        return self._handle_

    def run(self, x, state=None, scratch_bytes=1 << 28):
        x, is_np, squeeze, _ = _batchio.check_samples("TransferBatch", x, state, dual=True)
        S, T = x.shape[0], x.shape[2]
        _batchio.check_streams(S)
        _batchio.check_scratch_bytes(scratch_bytes)
        data, n_in = self._check_state(state, S)
        N = n_in + T
        E, bins = self.emitted(n_in, N), self.bins
        layout, state_len = state_layout(S, self.fft_size, self.hop, self.delay, N)
        h = self._handle()
        x, xptr, code, row, pair = _batchio.strided_rows(x, dual=True)
        vp, seb = ctypes.c_void_p, S * E * bins
        n_est = ctypes.c_int64(0)

        def call(state_in, state_out, out, frames):
            _lib.check(h.lib.frt_transfer_run(h.h, vp(xptr) if T else None, code, S, T, row, pair, vp(_batchio.ptr(state_in)),
                                              vp(_batchio.ptr(state_out)), n_in, int(scratch_bytes), vp(_batchio.ptr(out)) if seb else None,
                                              ctypes.byref(n_est)))

        def outputs():
            frames = _batchio.alloc(x, (E,), np.int64)
            frames[...] = self.average or self.frames_after(N)
            return _batchio.alloc(x, (state_len,)), _batchio.alloc(x, (7 * seb,)), frames

        new, out, frames = _batchio.run_call(x, is_np, outputs, h.set_stream, call, data)
        if is_np:
            cplx = lambda a: a.view(np.complex128).reshape(S, E, bins)
        else:
            import torch
            cplx = lambda a: torch.view_as_complex(a.reshape(S, E, bins, 2))
        assert n_est.value == E
        fields = [out[4 * seb:5 * seb].reshape(S, E, bins), out[5 * seb:6 * seb].reshape(S, E, bins), cplx(out[:2 * seb]),
                  cplx(out[2 * seb:4 * seb]), out[6 * seb:].reshape(S, E, bins)]
        if squeeze:
            fields = [f[0] for f in fields]
        return TransferResult(*fields, frames, self.freq, TransferState(new, S, N, layout["row0"][1][1], self.settings))
