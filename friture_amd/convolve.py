"""Applying a response to a signal: uniformly partitioned FFT convolution of recordings with a caller's FIR on the GPU
(convolve.hip, frt_convolve_*; the definition: X2 in include/friture_hip.h), and the impulse response behind a measured
transfer function (frt_irfft_rows).  The step after TransferBatch: auralise a measured room on dry material, deconvolve a
sweep with its inverse filter, apply a correction or a linear-phase EQ, or check a measured H1 by convolving the reference
row with its impulse response and subtracting the measured one.

A stream is one row x[s][t], t counted from the start of the stream across calls, x = 0 before it.  The taps h are L float64
values, 1 <= L <= 2^18, one filter for all streams ([L]) or one per stream ([S, L]); y[s][t] = sum_{l < L} h[s][l] x[s][t - l]
in float64 whatever the input dtype.  block B is a power of two in 64 .. 4096 (default: the smallest >= L, clamped), P =
ceil(L / B) <= 4096 partitions.  Output block j is y[j B .. j B + B) on the grid of absolute sample indices: the last B
samples of the inverse real 2 B-point transform of sum_p X_{j - p} H_p, summed in p from 0 (overlap-save).  A block's bits
depend on its whole window, so a call with flush=False emits complete blocks only (floor(n / B) B outputs after n samples in
total) and returns the state that continues the streams; flush=True continues with zeros, emits up to n + L - 1 and ends the
streams.  A recording cut into calls at any sample, any scratch_bytes and any batch give the bits of one whole call.  Out of
scope: fractional or time-varying filters, non-uniform partitions, a low-latency live object, a direct time-domain path for
short L; deconvolution by spectral division is friture_amd/deconvolve.py.  There is no CPU fallback: run() goes to the HIP library."""
from __future__ import annotations

import ctypes
import hashlib
from collections import namedtuple

import numpy as np

from . import _batchio, _lib

MIN_BLOCK, MAX_BLOCK = 64, 4096
MAX_TAPS = 1 << 18
MAX_PARTITIONS = 4096
TILE = 2                                    # output blocks per tile of the block kernel (no result depends on it)
MIN_IRFFT, MAX_IRFFT = 64, 8192

# tail: the carried input samples [S, ..] float64 (state_start(n_in) .. n_in - 1), None after a flush; streams; samples taken;
# outputs emitted; settings: those of the ConvolveBatch that made it
ConvolveState = namedtuple("ConvolveState", "tail streams n_in n_out settings")
ConvolveResult = namedtuple("ConvolveResult", "y state")


def default_block(L):
    """The smallest power of two >= L, clamped to 64 .. 4096."""
    return min(MAX_BLOCK, max(MIN_BLOCK, 1 << (int(L) - 1).bit_length()))


def emitted_after(n, L, block, flushed=False):
    """The outputs a stream has emitted after n samples in total."""
    return int(n) + L - 1 if flushed else int(n) // block * block


def state_start(n, block, partitions):
    """The first input sample that the state after n samples carries."""
    return max(0, (int(n) // block - partitions) * block)


def _dtype_name(dtype):
    name = str(np.dtype(dtype)) if isinstance(dtype, (str, type, np.dtype)) else str(dtype).split(".")[-1]
    if name not in ("float32", "float64"):
        raise TypeError(f"dtype must be float32 or float64, got {dtype!r}")
    return name


class ConvolveBatch:
    """ConvolveBatch(h, block=None).run(x, state=None, flush=True, dtype=None, scratch_bytes=1 << 28) -> ConvolveResult(y, state).
    h: [L] or [S, L], anything np.asarray takes.  x: [S, T] or [T], float32 or float64, numpy array or CUDA tensor (strided views
    are read in place).  y is of x's kind and dtype (or `dtype`): [S, n] or [n] with n = emitted_after(total, flush) minus
    what the calls before emitted.  state continues the streams in the next call (None after a flush).  The launches are cut
    into time slabs whose window spectra stay within scratch_bytes; the result has the same bits at any slab size."""

    def __init__(self, h, block=None):
        taps = np.asarray(h)
        if taps.dtype.kind not in "fiu" or taps.ndim not in (1, 2):
            raise ValueError(f"h must be real taps [L] or [S, L], got {taps.dtype} {taps.shape}")
        taps = np.ascontiguousarray(taps, np.float64)
        self.per_stream = taps.ndim == 2
        self.taps = taps.reshape(-1, taps.shape[-1])
        self.filters, self.L = self.taps.shape
        if not 1 <= self.L <= MAX_TAPS:
            raise ValueError(f"h must have 1 .. 2^18 taps, got {self.L}")
        if not 1 <= self.filters <= 65535:
            raise ValueError(f"expected 1 .. 65535 filters, got {self.filters}")
        if not np.all(np.isfinite(self.taps)):
            raise ValueError("h must be finite")
        if block is None:
            block = default_block(self.L)
        if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or not MIN_BLOCK <= block <= MAX_BLOCK or block & (block - 1):
            raise ValueError(f"block must be a power of two in {MIN_BLOCK} .. {MAX_BLOCK}, got {block!r}")
        self.block = int(block)
        self.partitions = -(-self.L // self.block)
        if self.partitions > MAX_PARTITIONS:
            raise ValueError(f"{self.partitions} partitions of block {self.block} for {self.L} taps (at most {MAX_PARTITIONS})")
        self.settings = (self.L, self.block, self.partitions, self.filters, self.per_stream, hashlib.sha1(self.taps.tobytes()).hexdigest())
        self._handle_ = None

    # ---- host only ------------------------------------------------------------------------------------------------------------
    def emitted_after(self, n, flushed=False):
        """The outputs a stream has emitted after n samples in total."""
        return emitted_after(n, self.L, self.block, flushed)

    def state_length(self, n):
        """The samples per stream that the state after n samples carries."""
        return int(n) - state_start(n, self.block, self.partitions)

    def _check_state(self, state, S):
        if state is None:
            return None, 0
        tail, streams, n_in, n_out, settings = state
        if tuple(settings) != self.settings:
            raise ValueError(f"state of other settings: {tuple(settings)} (want {self.settings})")
        if tail is None:
            raise ValueError("state of a flushed stream: it is final")
        if int(streams) != S:
            raise ValueError(f"state of another shape: {streams} streams (want {S})")
        n_in = int(n_in)
        if n_in < 0 or int(n_out) != self.emitted_after(max(n_in, 0)):
            raise ValueError(f"state of another stream: {n_out} outputs after {n_in} samples")
        want = (S, self.state_length(n_in))
        if tuple(tail.shape) != want:
            raise ValueError(f"state of another shape: tail {tuple(tail.shape)} (want {want})")
        return tail, n_in

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def _handle(self):
        if self._handle_ is None:
            self._handle_ = _lib.Handle("convolve", self.taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), self.L, self.filters, self.block)
        return self._handle_

    def run(self, x, state=None, flush=True, dtype=None, scratch_bytes=1 << 28):
        x, is_np, squeeze, _ = _batchio.check_samples("ConvolveBatch", x, None)
        S, T = x.shape
        _batchio.check_streams(S)
        if self.per_stream and self.filters != S:
            raise ValueError(f"{self.filters} filters for {S} streams")
        _batchio.check_scratch_bytes(scratch_bytes)
        out_name = _dtype_name(dtype) if dtype is not None else str(x.dtype).split(".")[-1]
        tail, n_in = self._check_state(state, S)
        flush = bool(flush)
        N = n_in + T
        n_out = self.emitted_after(N, flush) - self.emitted_after(n_in)
        n_tail = 0 if flush else self.state_length(N)
        h = self._handle()
        x, xptr, code, row, _ = _batchio.strided_rows(x)
        vp = ctypes.c_void_p
        got = ctypes.c_int64(0)

        def call(state_in, state_out, y):
            _lib.check(h.lib.frt_convolve_run(h.h, vp(xptr) if T else None, code, S, T, row, vp(_batchio.ptr(state_in)),
                                              vp(_batchio.ptr(state_out)), n_in, int(flush), int(scratch_bytes),
                                              vp(_batchio.ptr(y)) if n_out else None, int(out_name == "float64"), n_out, ctypes.byref(got)))

        def outputs():                                               # a flushed stream has no state
            return None if flush else _batchio.alloc(x, (S, n_tail)), _batchio.alloc(x, (S, n_out), out_name)

        new, y = _batchio.run_call(x, is_np, outputs, h.set_stream, call, tail)
        assert got.value == n_out
        return ConvolveResult(y[0] if squeeze else y, ConvolveState(new, S, N, self.emitted_after(N, flush), self.settings))


def convolve(x, h, block=None):
    """np.convolve(x[s], h[s]) per row in one flushed call, on the device: [S, T + L - 1] (or [T + L - 1]) of x's kind and dtype."""
    return ConvolveBatch(h, block).run(x).y


def impulse_response(res_or_h1):
    """The impulse response behind a transfer function: irfft over the last axis of a TransferResult's h1 (or of an h1 itself),
    [..., bins] complex128 -> [..., N] float64 with N = 2 (bins - 1) a power of two in 64 .. 8192, of h1's kind
    (frt_irfft_rows).  As numpy.fft.irfft, the imaginary parts of bins 0 and N / 2 do not count."""
    h1 = getattr(res_or_h1, "h1", res_or_h1)
    is_np = isinstance(h1, np.ndarray)
    if not is_np and not (type(h1).__module__.startswith("torch") and h1.is_cuda):
        raise TypeError("impulse_response takes a TransferResult, a numpy array or a CUDA tensor")
    if "complex128" not in str(h1.dtype) or h1.ndim < 1:
        raise TypeError(f"h1 must be complex128 [..., bins], got {h1.dtype} {tuple(h1.shape)}")
    bins = h1.shape[-1]
    N = 2 * (bins - 1)
    if not MIN_IRFFT <= N <= MAX_IRFFT or N & (N - 1):
        raise ValueError(f"h1 must have N / 2 + 1 bins, N a power of two in {MIN_IRFFT} .. {MAX_IRFFT}, got {bins}")
    lead = tuple(h1.shape[:-1])
    rows = int(np.prod(lead, dtype=np.int64))
    lib, vp = _lib.init(), ctypes.c_void_p
    if is_np:
        spec = np.ascontiguousarray(h1)
        out = np.empty(lead + (N,), np.float64)
        _lib.check(lib.frt_irfft_rows(vp(spec.ctypes.data), rows, N, vp(out.ctypes.data), None))
        return out
    import torch
    with _batchio.null_stream(h1, False):
        spec = torch.view_as_real(h1.contiguous())
        out = torch.empty(lead + (N,), dtype=torch.float64, device=h1.device)
        _lib.check(lib.frt_irfft_rows(vp(spec.data_ptr()), rows, N, vp(out.data_ptr()), None))
    return out
