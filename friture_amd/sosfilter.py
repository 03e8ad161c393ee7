"""IIR filters over whole recordings on the GPU: cascades of second-order sections, one filter per row or a bank of filters per
row, forward or reversed in time, with a carried state (sosfilter.hip, frt_sos_*; the definition: X6 in include/friture_hip.h),
and the Butterworth fractional-octave band-passes of room acoustics (ISO 3382) designed in numpy.

A filter is K sections (1 <= K <= 8) [b0 b1 b2 a0 a1 a2]; a0 != 1 is normalised on the host, a pole with |p| >= 1 is refused.
One sample through one section, in float64, every product rounded on its own:
    y = b0 x + z0;   z0 = (b1 x - a1 y) + z1;   z1 = b2 x - a2 y
and the sections run in order: the operation order of scipy.signal.sosfilt.  float32 input widens exactly.  Output rows are
(input row, filter):
    bank mode (fan=True): x [S, T] gives y [S, F, T], every input row through all F <= 64 filters;
    row mode: x [R, T] gives y [R, T], row r through filter r % F (F = 1: one filter for all rows, F = R: one per row).
reverse=True is flip(forward(flip(x))) from the zero state on whole rows; a state passed together with it is refused.  y is
float64, or float32 as the one rounding of the float64 value.
The rows are run time-parallel over cells of `cell` samples (a power of two in 32 .. 1024) on a grid anchored at the stream's
absolute sample index, the cell transition M = A^cell and M^64 made on the host in long double (the order of operations: X6).
A stream of at most `cell` samples is the sequential filter bit for bit; a longer one differs from it by rounding alone.  A
recording cut into calls at any sample, any scratch_bytes, batch, row stride, input dtype and host or device buffers give the
bits of one whole call: run() returns the state that continues the streams.  Out of scope: design families other than
Butterworth band-passes (the A and C weightings are in soundlevel.py), padding or steady-state initial conditions for zero-phase use, decimating banks, a live chunk object.
There is no CPU fallback: run() goes to the HIP library."""
from __future__ import annotations

import ctypes
import hashlib
import math
from collections import namedtuple

import numpy as np

from . import _batchio, _lib

MAX_SECTIONS, MAX_FILTERS = 8, 64
MIN_CELL, MAX_CELL = 32, 1024
MAX_SAMPLES = 1 << 24
STATE_VECTORS = 5                            # running state, partial zero-state run, S_c, partial Q, U_r (X6)

# data: [output rows, 5 * 2K] float64; rows: output rows; n: samples seen; settings: those of the SosBatch that made it
SosState = namedtuple("SosState", "data rows n settings")
SosResult = namedtuple("SosResult", "y state")


def _dtype_name(dtype):
    name = str(np.dtype(dtype)) if isinstance(dtype, (str, type, np.dtype)) else str(dtype).split(".")[-1]
    if name not in ("float32", "float64"):
        raise TypeError(f"dtype must be float32 or float64, got {dtype!r}")
    return name


class SosBatch:
    """SosBatch(sos, cell=None).run(x, fan=False, reverse=False, state=None, out=None, dtype=None, scratch_bytes=1 << 28) ->
    SosResult(y, state).  sos: [K, 6] (one filter) or [F, K, 6], anything np.asarray takes.  x: [T], [R, T] or [S, T], float32 or
    float64, numpy array or CUDA tensor (strided row views are read in place).  y is of x's kind and dtype (or `dtype`): [R, T],
    with fan=True [S, F, T] (without the row axis when x has none); out= takes a contiguous array of that kind, shape and dtype
    instead of a new one.  state continues the streams in the next call (None with reverse).  The rows are cut into slabs whose
    scratch stays within scratch_bytes; the result has the same bits at any slab size."""

    def __init__(self, sos, cell=None):
        s = np.asarray(sos)
        if s.dtype.kind not in "fiu" or s.ndim not in (2, 3) or s.shape[-1] != 6:
            raise ValueError(f"sos must be real sections [K, 6] or [F, K, 6], got {s.dtype} {s.shape}")
        s = np.ascontiguousarray(s, np.float64).reshape((-1,) + s.shape[-2:])
        self.filters, self.sections = s.shape[:2]
        if not 1 <= self.sections <= MAX_SECTIONS:
            raise ValueError(f"expected 1 .. {MAX_SECTIONS} sections, got {self.sections}")
        if not 1 <= self.filters <= MAX_FILTERS:
            raise ValueError(f"expected 1 .. {MAX_FILTERS} filters, got {self.filters}")
        if not np.all(np.isfinite(s)):
            raise ValueError("sos must be finite")
        if np.any(s[..., 3] == 0):
            raise ValueError("a0 must not be 0")
        self.raw = s
        self.sos = s / s[..., 3:4]                                   # a0 = 1: each quotient rounded once, as the library does
        self.sos[..., 3] = 1.0
        if not np.all(np.isfinite(self.sos)):
            raise ValueError("sos is not finite after the division by a0")
        a1, a2 = self.sos[..., 4], self.sos[..., 5]
        bad = ~((np.abs(a2) < 1) & (np.abs(a1) < 1 + a2))
        if np.any(bad):
            f, k = np.argwhere(bad)[0]
            raise ValueError(f"filter {f} section {k} has a pole with |p| >= 1 (a1 {a1[f, k]!r}, a2 {a2[f, k]!r})")
        if cell is None:
            cell = _lib.load().frt_sos_default_cell()
        if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or not MIN_CELL <= cell <= MAX_CELL or cell & (cell - 1):
            raise ValueError(f"cell must be a power of two in {MIN_CELL} .. {MAX_CELL}, got {cell!r}")
        self.cell = int(cell)
        self.state_length = STATE_VECTORS * 2 * self.sections
        self.settings = (self.filters, self.sections, self.cell, hashlib.sha1(self.sos.tobytes()).hexdigest())
        self._handle_ = None

    # ---- host only ------------------------------------------------------------------------------------------------------------
    def tables(self):
        """(coef [F, K, 5] = b0 b1 b2 a1 a2, M [F, 2K, 2K], M64 [F, 2K, 2K]) as the library makes them: M = A^cell in long double,
        rounded once.  Needs no GPU."""
        F, K = self.filters, self.sections
        coef, M, M64 = np.empty((F, K, 5)), np.empty((F, 2 * K, 2 * K)), np.empty((F, 2 * K, 2 * K))
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(_lib.load().frt_sos_tables(self.raw.ctypes.data_as(dp), F, K, self.cell, coef.ctypes.data_as(dp), M.ctypes.data_as(dp),
                                              M64.ctypes.data_as(dp)))
        return coef, M, M64

    def _check_state(self, state, orows):
        if state is None:
            return None, 0
        data, rows, n, settings = state
        if tuple(settings) != self.settings:
            raise ValueError(f"state of other settings: {tuple(settings)} (want {self.settings})")
        want = (orows, self.state_length)
        if int(rows) != orows or data is None or tuple(data.shape) != want:
            raise ValueError(f"state of another shape: {None if data is None else tuple(data.shape)} for {rows} rows (want {want})")
        if int(n) < 0:
            raise ValueError(f"state of another stream: {n} samples")
        return data, int(n)

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def _handle(self):
        if self._handle_ is None:
            self._handle_ = _lib.Handle("sos", self.raw.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), self.filters, self.sections, self.cell)
        return self._handle_

    def run(self, x, fan=False, reverse=False, state=None, out=None, dtype=None, scratch_bytes=1 << 28):
        x, is_np, squeeze, _ = _batchio.check_samples("SosBatch", x, None)
        R, T = x.shape
        _batchio.check_streams(R)
        if T > MAX_SAMPLES:
            raise ValueError(f"expected at most 2^24 samples per row and call, got {T}")
        _batchio.check_scratch_bytes(scratch_bytes)
        fan, reverse = bool(fan), bool(reverse)
        if reverse and state is not None:
            raise ValueError("reverse runs whole rows from the zero state: it takes no state")
        F = self.filters
        orows = R * F if fan else R
        out_name = _dtype_name(dtype) if dtype is not None else str(x.dtype).split(".")[-1]
        shape = (R, F, T) if fan else (R, T)
        if out is not None:
            same_kind = isinstance(out, np.ndarray) if is_np else (not isinstance(out, np.ndarray) and getattr(out, "is_cuda", False))
            want = shape[1:] if squeeze else shape
            contiguous = same_kind and (out.flags.c_contiguous if is_np else out.is_contiguous())
            if not same_kind or tuple(out.shape) != want or str(out.dtype).split(".")[-1] != out_name or not contiguous:
                raise ValueError(f"out must be a contiguous {out_name} array of x's kind and shape {want}")
        data, n_in = self._check_state(state, orows)
        if T == 0:                                                   # nothing to do: the streams stand where they stood
            y = out if out is not None else _batchio.alloc(x, shape[1:] if squeeze else shape, out_name)
            if state is None and not reverse:
                state = SosState(_batchio.alloc(x, (orows, self.state_length), zero=True), orows, 0, self.settings)
            return SosResult(y, None if reverse else state)
        h = self._handle()
        x, xptr, code, row, _ = _batchio.strided_rows(x)
        vp = ctypes.c_void_p

        def call(state_in, state_out, y):
            _lib.check(h.lib.frt_sos_run(h.h, vp(xptr), code, R, T, row, int(fan), int(reverse), n_in, vp(_batchio.ptr(state_in)),
                                         vp(_batchio.ptr(state_out)), int(scratch_bytes), vp(_batchio.ptr(y)), int(out_name == "float64")))

        def outputs():
            return (None if reverse else _batchio.alloc(x, (orows, self.state_length)),
                    out if out is not None else _batchio.alloc(x, shape, out_name))

        new, y = _batchio.run_call(x, is_np, outputs, h.set_stream, call, data)
        if out is None and squeeze:
            y = y[0]
        return SosResult(y, None if reverse else SosState(new, orows, n_in + T, self.settings))


def sosfilt(x, sos, cell=None, **kw):
    """SosBatch(sos, cell).run(x, **kw).y in one call."""
    return SosBatch(sos, cell).run(x, **kw).y


# ---- design: Butterworth band-passes, numpy only --------------------------------------------------------------------------------

def butter_band_sos(f_lo, f_hi, fs=48000, order=3):
    """The Butterworth band-pass of the given order between f_lo and f_hi (its -3 dB edges) as [order, 6] sections (a0 = 1): the
    analogue low-pass prototype's poles exp(i pi (2 k + order + 1) / (2 order)), the band-pass transform s -> (s^2 + w0^2) /
    (bw s) with the edges pre-warped (w = 2 fs tan(pi f / fs)), the bilinear transform, each conjugate pole pair with one zero
    at z = 1 and one at z = -1 as a section, the gain spread evenly over the sections.  The squared magnitude is 1 / (1 +
    W^(2 order)), W = (w^2 - w_lo w_hi) / (w (w_hi - w_lo)), w = tan(pi f / fs)."""
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= order <= MAX_SECTIONS:
        raise ValueError(f"order must be an integer in 1 .. {MAX_SECTIONS}, got {order!r}")
    if not (math.isfinite(fs) and 0 < f_lo < f_hi < fs / 2):
        raise ValueError(f"expected 0 < f_lo < f_hi < fs / 2, got {f_lo!r}, {f_hi!r} at fs {fs!r}")
    N, fs2 = int(order), 2.0 * fs
    w1, w2 = fs2 * math.tan(math.pi * f_lo / fs), fs2 * math.tan(math.pi * f_hi / fs)
    bw, w0sq = w2 - w1, w1 * w2
    k = np.arange(N)
    proto = np.exp(1j * np.pi * (2 * k + N + 1) / (2 * N))           # left half-plane, |p| = 1
    half = proto * bw / 2
    root = np.sqrt(half * half - w0sq + 0j)
    analogue = np.concatenate([half + root, half - root])            # 2 N poles; N zeros at s = 0, N at infinity
    poles = (fs2 + analogue) / (fs2 - analogue)
    gain = (bw ** N) * (fs2 ** N) / np.real(np.prod(fs2 - analogue))
    upper = poles[poles.imag > 1e-14 * np.abs(poles)]
    real = np.sort(poles[np.abs(poles.imag) <= 1e-14 * np.abs(poles)].real)
    pairs = [(-2.0 * p.real, p.real * p.real + p.imag * p.imag) for p in upper[np.argsort(np.abs(upper))]]
    pairs += [(-(real[i] + real[i + 1]), real[i] * real[i + 1]) for i in range(0, len(real) - 1, 2)]
    if len(pairs) != N or len(real) % 2:
        raise ValueError(f"the poles of {f_lo!r} .. {f_hi!r} Hz at fs {fs!r}, order {N}, do not pair into {N} sections")
    g = gain ** (1.0 / N)
    return np.array([[g, 0.0, -g, 1.0, a1, a2] for a1, a2 in pairs], np.float64)


def band_sos(bands="octave", fs=48000, order=3):
    """(centres [B], sos [B, order, 6]): Butterworth band-passes on the IEC 61260-1 base-ten band edges of decay.band_edges
    ("octave", "third" or (f_lo, f_hi) pairs)."""
    from . import decay
    centres, edges = decay.band_edges(bands)
    return centres, np.stack([butter_band_sos(lo, hi, fs, order) for lo, hi in edges])
