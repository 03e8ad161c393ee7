"""Measuring a long impulse response: deconvolution of recordings by regularised spectral division on the GPU, and the float64
real transform of whole rows that it is built on (deconvolve.hip, frt_deconvolve_*, frt_rfft_long_rows, frt_irfft_long_rows;
the definition: X4 in include/friture_hip.h).  The step between a recording and DecayBatch: play an exponential sweep, record
the room, divide the spectra (ISO 18233), and read reverberation time and clarity from the response:
load_wav -> DeconvolveBatch -> room_acoustics.

n is a power of two in 2^13 .. 2^24; all arithmetic is float64.  rfft_rows(x, n) is numpy.fft.rfft(x, n) over the last axis of
rows of T <= n samples, irfft_rows(X, n, keep) the first keep samples of numpy.fft.irfft(X, n).  A reference x of Lx <= n
samples, one for all rows ([Lx]) or one per row ([S, Lx]), gives at creation P = |X|^2, Pmax = max P and G = conj(X) / (P + r Pmax),
r a scalar reg >= 0 or one value >= 0 per bin ([n/2 + 1]: a frequency-dependent, Kirkeby-style regularisation), G = 0 where
the denominator is 0.  A measured row y of T <= n samples gives H = Y G and h = irfft(H, n)[:keep].  The division is circular:
with n >= T the acausal part, the harmonic-distortion responses of a sweep, sits at the end of h (harmonic_offsets).  A row's
bits depend on its own samples, n, the reference and r only: not on the batch, scratch_bytes, a row stride, the input's dtype
or numpy versus CUDA input.  Out of scope: n that is no power of two or below 2^13 (impulse_response's range), multi-channel
inversion, windowing of the result, minimum-phase or inverse-filter design.  There is no CPU fallback: run() goes to the HIP
library.  exp_sweep and harmonic_offsets are host numpy, given so that a measurement is defined end to end."""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import numpy as np

from . import _batchio, _lib

MIN_N, MAX_N = 1 << 13, 1 << 24

DeconvolveResult = namedtuple("DeconvolveResult", "h spectrum")


def exp_sweep(f0, f1, length, fs=48000, fade=0):
    """The exponential sweep sin(2 pi f0 Td / K (exp(t K / Td) - 1)), K = ln(f1 / f0), Td = length / fs, t = 0 .. (length - 1) / fs,
    as float64 [length] on the host; the first and last `fade` samples carry a raised-cosine fade."""
    if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or length < 2:
        raise ValueError(f"length must be an integer >= 2, got {length!r}")
    if not (math.isfinite(fs) and fs > 0 and math.isfinite(f0) and math.isfinite(f1) and 0 < f0 < f1 <= fs / 2):
        raise ValueError(f"expected 0 < f0 < f1 <= fs / 2, got {f0!r}, {f1!r} at fs {fs!r}")
    if isinstance(fade, bool) or not isinstance(fade, (int, np.integer)) or not 0 <= 2 * fade <= length:
        raise ValueError(f"fade must be an integer in 0 .. length / 2, got {fade!r}")
    Td, K = length / fs, math.log(f1 / f0)
    t = np.arange(length, dtype=np.float64) / fs
    x = np.sin(2 * np.pi * f0 * Td / K * np.expm1(t * K / Td))
    if fade:
        ramp = np.sin(np.linspace(0.0, np.pi / 2, fade)) ** 2
        x[:fade] *= ramp
        x[length - fade:] *= ramp[::-1]
    return x


def harmonic_offsets(sweep_len, f0, f1, orders=(2, 3)):
    """sweep_len ln(k) / ln(f1 / f0) per order k, float64: the k-th harmonic's response of an exp_sweep measurement starts
    that many samples before the linear one, at h[n - offset] of the circular result."""
    if not (0 < f0 < f1) or sweep_len < 1:
        raise ValueError(f"expected 0 < f0 < f1 and sweep_len >= 1, got {f0!r}, {f1!r}, {sweep_len!r}")
    orders = np.asarray(orders)
    if orders.dtype.kind not in "iu" or np.any(orders < 1):
        raise ValueError(f"orders must be integers >= 1, got {orders!r}")
    return sweep_len * np.log(orders.astype(np.float64)) / math.log(f1 / f0)


def default_n(Lx):
    """The smallest power of two >= 2 Lx, at least 2^13."""
    return max(MIN_N, 1 << (2 * int(Lx) - 1).bit_length())


def _check_n(n):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not MIN_N <= n <= MAX_N or n & (n - 1):
        raise ValueError(f"n must be a power of two in 2^13 .. 2^24, got {n!r}")
    return int(n)


def _check_keep(keep, n):
    if keep is None:
        return n
    if isinstance(keep, bool) or not isinstance(keep, (int, np.integer)) or not 1 <= keep <= n:
        raise ValueError(f"keep must be an integer in 1 .. n = {n}, got {keep!r}")
    return int(keep)


class DeconvolveBatch:
    """DeconvolveBatch(x, n=None, reg=1e-6).run(y, keep=None, spectrum=False, scratch_bytes=1 << 28) -> DeconvolveResult(h, spectrum).
    x: the reference, [Lx] or [S, Lx], anything np.asarray takes (a tensor comes to the host).  n: default the smallest power of
    two >= 2 Lx, at least 2^13.  reg: a scalar >= 0 or [n/2 + 1] values >= 0.  y: [S, T] or [T], T <= n, float32 or float64, numpy
    array or CUDA tensor (strided row views are read in place).  h: float64 [S, keep] (keep defaults to n) of y's kind;
    spectrum: H as complex128 [S, n/2 + 1], or None.  The rows are cut into slabs whose scratch stays within scratch_bytes; the
    result has the same bits at any slab size."""

    def __init__(self, x, n=None, reg=1e-6):
        if hasattr(x, "cpu"):
            x = x.cpu().numpy()
        ref = np.asarray(x)
        if ref.dtype.kind not in "fiu" or ref.ndim not in (1, 2):
            raise ValueError(f"x must be a real reference [Lx] or [S, Lx], got {ref.dtype} {ref.shape}")
        ref = np.ascontiguousarray(ref, np.float64)
        self.per_row = ref.ndim == 2
        self.ref = ref.reshape(-1, ref.shape[-1])
        self.refs, self.Lx = self.ref.shape
        if not 1 <= self.refs <= 65535:
            raise ValueError(f"expected 1 .. 65535 references, got {self.refs}")
        if self.Lx < 1:
            raise ValueError("x must have at least one sample")
        if n is None:
            n = default_n(self.Lx)
            if n > MAX_N:
                raise ValueError(f"a reference of {self.Lx} samples needs n = {n} (at most 2^24): give n")
        self.n = _check_n(n)
        if self.Lx > self.n:
            raise ValueError(f"x must have 1 .. n = {self.n} samples, got {self.Lx}")
        if not np.all(np.isfinite(self.ref)):
            raise ValueError("x must be finite")
        if hasattr(reg, "cpu"):
            reg = reg.cpu().numpy()
        r = np.asarray(reg)
        if r.dtype.kind not in "fiu" or r.shape not in ((), (self.n // 2 + 1,)):
            raise ValueError(f"reg must be a scalar or [{self.n // 2 + 1}] values, got {r.dtype} {r.shape}")
        if not np.all(np.isfinite(r)) or np.any(r < 0):
            raise ValueError("reg must be finite and >= 0")
        self.reg, self.reg_bins = (float(r), None) if r.ndim == 0 else (0.0, np.ascontiguousarray(r, np.float64))
        self._handle_ = None

    def _handle(self):
        if self._handle_ is None:
            dp = ctypes.POINTER(ctypes.c_double)
            bins = None if self.reg_bins is None else self.reg_bins.ctypes.data_as(dp)
            self._handle_ = _lib.Handle("deconvolve", self.ref.ctypes.data_as(dp), self.Lx, self.refs, self.n, self.reg, bins)
        return self._handle_

    def run(self, y, keep=None, spectrum=False, scratch_bytes=1 << 28):
        x, is_np, squeeze, _ = _batchio.check_samples("DeconvolveBatch", y, None)
        S, T = x.shape
        _batchio.check_streams(S)
        if not 1 <= T <= self.n:
            raise ValueError(f"expected 1 .. n = {self.n} samples per row, got {T}")
        if self.per_row and self.refs != S:
            raise ValueError(f"{self.refs} references for {S} rows")
        keep = _check_keep(keep, self.n)
        _batchio.check_scratch_bytes(scratch_bytes)
        h = self._handle()
        x, xptr, code, row, _ = _batchio.strided_rows(x)
        vp = ctypes.c_void_p
        bins = self.n // 2 + 1

        def call(_, out, spec):
            _lib.check(h.lib.frt_deconvolve_run(h.h, vp(xptr), code, S, T, row, keep, int(scratch_bytes), vp(_batchio.ptr(out)), keep,
                                                vp(_batchio.ptr(spec))))

        def outputs():
            return _batchio.alloc(x, (S, keep)), _batchio.alloc(x, (S, bins), np.complex128) if spectrum else None

        out, spec = _batchio.run_call(x, is_np, outputs, h.set_stream, call, None)
        if squeeze:
            out, spec = out[0], None if spec is None else spec[0]
        return DeconvolveResult(out, spec)


def deconvolve(y, x, n=None, reg=1e-6, keep=None):
    """h of DeconvolveBatch(x, n, reg).run(y, keep) in one call."""
    return DeconvolveBatch(x, n, reg).run(y, keep).h


def rfft_rows(x, n, scratch_bytes=1 << 28):
    """numpy.fft.rfft(x, n) over the last axis on the device: x [..., T], T <= n, float32 or float64, numpy array or CUDA tensor
    -> complex128 [..., n/2 + 1] of x's kind (frt_rfft_long_rows); n a power of two in 2^13 .. 2^24."""
    is_np = isinstance(x, np.ndarray)
    if not is_np and not (type(x).__module__.startswith("torch") and x.is_cuda):
        raise TypeError("rfft_rows takes a numpy array or a CUDA tensor")
    if str(x.dtype).split(".")[-1] not in ("float32", "float64"):
        raise TypeError(f"samples must be float32 or float64, got {x.dtype}")
    n = _check_n(n)
    if x.ndim < 1 or not 1 <= x.shape[-1] <= n:
        raise ValueError(f"expected [..., T] with 1 <= T <= n = {n}, got {tuple(x.shape)}")
    _batchio.check_scratch_bytes(scratch_bytes)
    lead, T = tuple(x.shape[:-1]), x.shape[-1]
    rows = int(np.prod(lead, dtype=np.int64))
    _batchio.check_streams(rows)
    x2 = x if x.ndim == 2 else x.reshape(rows, T)
    x2, xptr, code, row, _ = _batchio.strided_rows(x2)
    lib, vp = _lib.init(), ctypes.c_void_p

    def call(_, spec):
        _lib.check(lib.frt_rfft_long_rows(vp(xptr), code, rows, T, row, n, int(scratch_bytes), vp(_batchio.ptr(spec)), None))

    spec, = _batchio.run_call(x2, is_np, lambda: (_batchio.alloc(x2, (rows, n // 2 + 1), np.complex128),), lambda: None, call, None)
    return spec.reshape(lead + (n // 2 + 1,))


def irfft_rows(spec, n, keep=None, scratch_bytes=1 << 28):
    """The first keep samples (default n) of numpy.fft.irfft(spec, n) over the last axis on the device: spec complex128
    [..., n/2 + 1], numpy array or CUDA tensor -> float64 [..., keep] of spec's kind (frt_irfft_long_rows).  The imaginary
    parts of bins 0 and n/2 do not count."""
    is_np = isinstance(spec, np.ndarray)
    if not is_np and not (type(spec).__module__.startswith("torch") and spec.is_cuda):
        raise TypeError("irfft_rows takes a numpy array or a CUDA tensor")
    if "complex128" not in str(spec.dtype):
        raise TypeError(f"spec must be complex128, got {spec.dtype}")
    n = _check_n(n)
    if spec.ndim < 1 or spec.shape[-1] != n // 2 + 1:
        raise ValueError(f"expected [..., n/2 + 1 = {n // 2 + 1}], got {tuple(spec.shape)}")
    keep = _check_keep(keep, n)
    _batchio.check_scratch_bytes(scratch_bytes)
    lead = tuple(spec.shape[:-1])
    rows = int(np.prod(lead, dtype=np.int64))
    _batchio.check_streams(rows)
    flat = np.ascontiguousarray(spec).reshape(rows, -1) if is_np else spec.contiguous().reshape(rows, -1)
    lib, vp = _lib.init(), ctypes.c_void_p

    def call(_, out):
        _lib.check(lib.frt_irfft_long_rows(vp(_batchio.ptr(flat)), rows, n, keep, int(scratch_bytes), vp(_batchio.ptr(out)), keep, None))

    out, = _batchio.run_call(flat, is_np, lambda: (_batchio.alloc(flat, (rows, keep)),), lambda: None, call, None)
    return out.reshape(lead + (keep,))
