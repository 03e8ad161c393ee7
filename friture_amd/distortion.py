"""What a system does to a tone: the level and frequency of the fundamental, the harmonics, the residual noise, THD, THD+N,
SINAD and SNR of recordings of a sine, frame by frame and over the whole recording, on the GPU (distortion.hip, frt_tone_*;
the definition: X9 in include/friture_hip.h).  The first measurement of an audio analyser, next to the linear ones of
TransferBatch and DeconvolveBatch.

A stream is one row.  fft_size N is a power of two in 512 .. 16384, hop >= 1 (it may exceed N; default N // 2), window
("kaiser", beta) (numpy.kaiser(N, beta)) or N float64 values, lobe L the half-width of a spectral line in bins (1 .. 16;
for a Kaiser window ceil(sqrt(1 + (beta / pi)^2)) + 1 by default, required with an array window), harmonics H the highest
order (2 .. 32), band (f_lo, f_hi) in Hz: the bins ka = max(L + 1, ceil(f_lo N / fs)) .. kb = min(N/2, floor(f_hi N / fs)),
by default L + 1 .. N/2; f0 in Hz, a scalar or one value per stream: the fundamental is searched over ka + L .. kb - L,
with f0 only within L bins of rint(f0 N / fs); gate_db: a live frame whose fundamental lies below it does not count.

Frame f is x[f hop : f hop + N]; X = rfft(x w), Q[k] = c_k |X[k]|^2 / (N sum w^2) with c_k = 2 except c_0 = c_N/2 = 1 (a
unit sine's line sums to 0.5).  c1 = the arg-max of Q over the search range (lowest index on ties), P1 = sum Q[c1 - L ..
c1 + L], kappa = sum k Q[k] / P1, freq = kappa fs / N.  Order h = 2 .. H sits at c_h = rint(h kappa); it is present when
c_h + L <= kb, its lobe is [max(c_h - L, c_(h-1) + L + 1), c_h + L] (a bin counts once, for the lowest order), P_h its sum;
an absent order is NaN.  The residual R is the sum of Q over ka .. kb outside every lobe: no power is a difference.  A frame
with a non-finite sample or with Q all zero over the search range is dead (NaN, peak_bin -1); a live frame with P1 below
the gate keeps its values and is not valid.  The totals per stream are n_valid and the left folds in frame order over the
valid frames of kappa, P1, R and each P_h; every order of summation is fixed (X9), so a recording cut into calls anywhere,
any slab size and any batch give the same bits.  Out of scope: frames above 16384 (fundamentals below about (2 L + 1) fs /
N: decimate first), weighting curves, spurs / SFDR, two-tone intermodulation, harmonic phases, notch-filter time-domain
THD+N, multi-tone signals, a live chunk object, DeconvolveBatch's harmonic responses.  There is no CPU fallback: run() goes
to the HIP library."""
from __future__ import annotations

import ctypes
import hashlib
import math
from collections import namedtuple

import numpy as np

from . import _batchio, _lib

MIN_FFT_SIZE, MAX_FFT_SIZE = 512, 16384
MAX_HOP = 1 << 30
MAX_LOBE, MAX_ORDER = 16, 32

# data: one float64 array (its layout: state_layout); streams; samples taken; pending: carried samples per stream; settings:
# those of the ToneBatch that made it
ToneState = namedtuple("ToneState", "data streams n_in pending settings")


def frames_after(n, fft_size, hop):
    """F(n): the complete frames after n samples in total."""
    n = int(n)
    return 0 if n < fft_size else (n - fft_size) // hop + 1


def state_layout(S, fft_size, hop, harmonics, n_in):
    """name -> (offset, shape) of the parts of a state's data after n_in samples, and its length."""
    F = frames_after(n_in, fft_size, hop)
    parts = (("totals", (S, 3 + harmonics)), ("row", (S, n_in - min(n_in, F * hop))))
    out, at = {}, 0
    for name, shape in parts:
        out[name] = (at, shape)
        at += shape[0] * shape[1]
    return out, at


def kaiser_lobe(beta):
    """The default half-width in bins of a line under a Kaiser window: its first null, rounded up, and one bin."""
    return int(math.ceil(math.sqrt(1.0 + (beta / math.pi) ** 2))) + 1


def _log10(a):
    if isinstance(a, np.ndarray) or np.isscalar(a):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.log10(a)
    import torch
    return torch.log10(a)


def _nansum_last(a):
    if isinstance(a, np.ndarray):
        return np.nansum(a, axis=-1)
    import torch
    return torch.nansum(a, dim=-1)


class _Levels:
    """The derived dB figures of fund (P1), resid (R) and harmonics (P_2 .. P_H; NaN: absent), elementwise on the arrays where
    they live."""

    def _ratio_db(self, num, den):
        with np.errstate(divide="ignore", invalid="ignore"):
            return 10.0 * _log10(num / den)

    @property
    def harmonic_sum(self):
        return _nansum_last(self.harmonics)

    @property
    def thd_db(self):
        return self._ratio_db(self.harmonic_sum, self.fund)

    @property
    def thdn_db(self):
        return self._ratio_db(self.harmonic_sum + self.resid, self.fund)

    @property
    def sinad_db(self):
        return -self.thdn_db

    @property
    def snr_db(self):
        return self._ratio_db(self.fund, self.resid)

    @property
    def level_db(self):
        return 10.0 * _log10(2.0 * self.fund)

    @property
    def harmonics_db(self):
        """10 log10(P_h / P1), orders 2 .. H along the last axis."""
        return self._ratio_db(self.harmonics, self.fund[..., None])


class ToneTotal(_Levels):
    """Per stream: n_valid int64 [S] and the means over the valid frames of freq, fund, resid [S] and harmonics [S, H - 1] (the
    totals of X9 divided by n_valid; NaN without a valid frame), with the dB properties of a ToneResult."""

    def __init__(self, n_valid, freq, fund, resid, harmonics):
        self.n_valid, self.freq, self.fund, self.resid, self.harmonics = n_valid, freq, fund, resid, harmonics

    def __repr__(self):
        return f"ToneTotal(n_valid={self.n_valid!r}, freq={self.freq!r}, thd_db={self.thd_db!r}, thdn_db={self.thdn_db!r})"


class ToneResult(_Levels):
    """freq (Hz), fund (P1), resid (R) [S, F] float64, harmonics [S, F, H - 1] (P_2 .. P_H, NaN: absent), peak_bin int32 [S, F]
    (-1: dead), valid bool [S, F], of the input's kind and without the S axis for [T]; total: a ToneTotal; state.  thd_db,
    thdn_db, sinad_db, snr_db, level_db, harmonics_db: elementwise on these arrays."""

    def __init__(self, freq, fund, resid, harmonics, peak_bin, valid, total, state):
        self.freq, self.fund, self.resid, self.harmonics = freq, fund, resid, harmonics
        self.peak_bin, self.valid, self.total, self.state = peak_bin, valid, total, state


class ToneBatch:
    """run(x, state=None, scratch_bytes=1 << 28) -> ToneResult.  x: [S, T] or [T], float32 or float64, numpy array or CUDA
    tensor (strided row views are read in place).  state continues the streams in the next call: it carries the last
    N - hop samples (or what exists of them), the counts and the totals, and a recording cut into calls at any sample gives
    the bits of one call.  The launches are cut into time slabs whose frame records stay within scratch_bytes; the result
    has the same bits at any slab size."""

    def __init__(self, fft_size=8192, hop=None, window=("kaiser", 20.0), lobe=None, harmonics=10, band=None, f0=None, gate_db=None,
                 fs=48000):
        def integer(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)

        def real(v):
            return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v)

        if not integer(fft_size) or fft_size < MIN_FFT_SIZE or fft_size & (fft_size - 1) or fft_size > MAX_FFT_SIZE:
            raise ValueError(f"fft_size must be a power of two in {MIN_FFT_SIZE} .. {MAX_FFT_SIZE}, got {fft_size!r}")
        N = self.fft_size = int(fft_size)
        hop = N // 2 if hop is None else hop
        if not integer(hop) or not 1 <= hop <= MAX_HOP:
            raise ValueError(f"hop must be an integer in 1 .. 2^30, got {hop!r}")
        self.hop = int(hop)
        _batchio.check_fs(fs)
        self.fs = float(fs)
        if isinstance(window, tuple):
            if len(window) != 2 or window[0] != "kaiser" or not real(window[1]) or window[1] < 0:
                raise ValueError(f"window={window!r} (('kaiser', beta >= 0) or {N} float64 values)")
            beta = float(window[1])
            self.window, key = np.ascontiguousarray(np.kaiser(N, beta), np.float64), ("kaiser", beta)
            lobe = kaiser_lobe(beta) if lobe is None else lobe
        elif isinstance(window, str):
            raise ValueError(f"window={window!r} (('kaiser', beta >= 0) or {N} float64 values)")
        else:
            self.window = np.ascontiguousarray(window, np.float64)
            if self.window.shape != (N,) or not np.all(np.isfinite(self.window)) or not np.any(self.window):
                raise ValueError(f"window must be {N} finite values, not all zero, got shape {self.window.shape}")
            key = hashlib.sha1(self.window.tobytes()).hexdigest()
            if lobe is None:
                raise ValueError("lobe is required with an array window")
        if not integer(lobe) or not 1 <= lobe <= MAX_LOBE:
            raise ValueError(f"lobe must be an integer in 1 .. {MAX_LOBE}, got {lobe!r}")
        L = self.lobe = int(lobe)
        if not integer(harmonics) or not 2 <= harmonics <= MAX_ORDER:
            raise ValueError(f"harmonics must be an integer in 2 .. {MAX_ORDER}, got {harmonics!r}")
        self.harmonics = int(harmonics)
        ka, kb = L + 1, N // 2
        if band is not None:
            if not isinstance(band, (tuple, list)) or len(band) != 2 or not all(real(v) for v in band) or not 0 <= band[0] <= band[1]:
                raise ValueError(f"band must be (f_lo, f_hi) with 0 <= f_lo <= f_hi in Hz, got {band!r}")
            ka = max(ka, int(math.ceil(band[0] * N / self.fs)))
            kb = min(kb, int(math.floor(band[1] * N / self.fs)))
        self.ka, self.kb = ka, kb
        if f0 is None:
            centre = None
        else:
            f0 = np.atleast_1d(np.asarray(f0.cpu() if hasattr(f0, "cpu") else f0, np.float64))
            if f0.ndim != 1 or not f0.size or not np.all(np.isfinite(f0)) or np.any(f0 < 0) or np.any(f0 > self.fs):
                raise ValueError(f"f0 must be a frequency in 0 .. fs or one per stream, got {f0!r}")
            centre = np.rint(f0 * N / self.fs).astype(np.int64)
        klo, khi = ka + L, kb - L
        if centre is None:
            klo, khi = np.array([klo]), np.array([khi])
        else:
            klo, khi = np.maximum(klo, centre - L), np.minimum(khi, centre + L)
        if np.any(klo > khi):
            s = int(np.argmax(klo > khi))
            raise ValueError(f"the search range of stream {s} is empty: bins {int(klo[s])} .. {int(khi[s])} (band bins {ka} .. {kb}, "
                             f"lobe {L}" + (f", f0 {float(f0[s])} Hz" if centre is not None else "") + ")")
        self.klo, self.khi = np.ascontiguousarray(klo, np.int32), np.ascontiguousarray(khi, np.int32)
        if gate_db is None:
            self.gate_db, self.gate = None, 0.0
        else:
            if not isinstance(gate_db, (int, float, np.integer, np.floating)) or isinstance(gate_db, bool) or math.isnan(gate_db) \
                    or gate_db > 300:
                raise ValueError(f"gate_db must be a level in dB (at most 300), got {gate_db!r}")
            self.gate_db = float(gate_db)
            self.gate = 0.0 if self.gate_db == -math.inf else 10.0 ** (self.gate_db / 10.0)
        self.bins = N // 2 + 1
        self.settings = (N, self.hop, key, L, self.harmonics, ka, kb, hashlib.sha1(self.klo.tobytes() + self.khi.tobytes()).hexdigest(),
                         self.gate, self.fs)
        self._handle_ = None

    # ---- host only ------------------------------------------------------------------------------------------------------------
    def frames_after(self, n):
        """F(n): the complete frames after n samples in total."""
        return frames_after(n, self.fft_size, self.hop)

    def state_parts(self, state):
        """The parts of a state as views of its data: totals [S, 3 + H] (the sums of kappa, P1, R, P_2 .. P_H, then n_valid) and
        row [S, pending]."""
        layout, _ = state_layout(state.streams, self.fft_size, self.hop, self.harmonics, int(state.n_in))
        return {name: state.data[at:at + shape[0] * shape[1]].reshape(shape) for name, (at, shape) in layout.items()}

    def _check_state(self, state, S):
        if state is None:
            return None, 0
        data, streams, n_in, pending, settings = state
        if tuple(settings) != self.settings:
            raise ValueError(f"state of other settings: {tuple(settings)} (want {self.settings})")
        if int(streams) != S:
            raise ValueError(f"state of another shape: {streams} streams (want {S})")
        n_in = int(n_in)
        layout, want = state_layout(S, self.fft_size, self.hop, self.harmonics, max(n_in, 0))
        if n_in < 0 or int(pending) != layout["row"][1][1]:
            raise ValueError(f"state of another stream: {pending} pending samples after {n_in}")
        if data.ndim != 1 or data.shape[0] != want:
            raise ValueError(f"state of another shape: data {tuple(data.shape)} (want {(want,)})")
        return data, n_in

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def _handle(self):
        if self._handle_ is None:
            ip = ctypes.POINTER(ctypes.c_int)
            self._handle_ = _lib.Handle("tone", self.fft_size, self.hop, self.window.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                        self.lobe, self.harmonics, self.ka, self.kb, self.klo.ctypes.data_as(ip),
                                        self.khi.ctypes.data_as(ip), len(self.klo), self.gate)
        return self._handle_

    def run(self, x, state=None, scratch_bytes=1 << 28):
        x, is_np, squeeze, _ = _batchio.check_samples("ToneBatch", x, state)
        S, T = x.shape
        _batchio.check_streams(S)
        _batchio.check_scratch_bytes(scratch_bytes)
        if len(self.klo) not in (1, S):
            raise ValueError(f"f0 has {len(self.klo)} values for {S} streams")
        data, n_in = self._check_state(state, S)
        n_out, H, RW = n_in + T, self.harmonics, 3 + self.harmonics
        F = self.frames_after(n_out) - self.frames_after(n_in)
        layout, state_len = state_layout(S, self.fft_size, self.hop, H, n_out)
        h = self._handle()
        x, xptr, code, row, _ = _batchio.strided_rows(x)
        vp, sf = ctypes.c_void_p, S * F
        n_frames = ctypes.c_int64(0)

        def call(state_in, state_out, out):
            _lib.check(h.lib.frt_tone_run(h.h, vp(xptr) if T else None, code, S, T, row, vp(_batchio.ptr(state_in)),
                                          vp(_batchio.ptr(state_out)), n_in, int(scratch_bytes), vp(_batchio.ptr(out)) if sf else None,
                                          ctypes.byref(n_frames)))

        def outputs():
            return _batchio.alloc(x, (state_len,)), _batchio.alloc(x, (RW * sf,))

        new, out = _batchio.run_call(x, is_np, outputs, h.set_stream, call, data)
        assert n_frames.value == F
        scale = self.fs / self.fft_size
        flags = out[(2 + H) * sf:].reshape(S, F)
        live = flags >= 0
        if is_np:
            whole = flags.astype(np.int64)
            peak_bin, valid = np.where(live, whole >> 1, -1).astype(np.int32), live & ((whole & 1) == 1)
        else:
            import torch
            whole = flags.to(torch.int64)
            peak_bin, valid = torch.where(live, whole >> 1, -1).to(torch.int32), live & ((whole & 1) == 1)
        fields = [out[:sf].reshape(S, F) * scale, out[sf:2 * sf].reshape(S, F), out[2 * sf:3 * sf].reshape(S, F),
                  out[3 * sf:(2 + H) * sf].reshape(S, F, H - 1), peak_bin, valid]
        totals = new[:S * RW].reshape(S, RW)
        count = totals[:, RW - 1]
        if is_np:
            n_valid = count.astype(np.int64)
            with np.errstate(divide="ignore", invalid="ignore"):
                mean = totals[:, :RW - 1] / count[:, None]
        else:
            n_valid = count.to(torch.int64)
            mean = totals[:, :RW - 1] / count[:, None]
        total = [n_valid, mean[:, 0] * scale, mean[:, 1], mean[:, 2], mean[:, 3:]]
        if squeeze:
            fields, total = [f[0] for f in fields], [t[0] for t in total]
        return ToneResult(*fields, ToneTotal(*total), ToneState(new, S, n_out, layout["row"][1][1], self.settings))


def tone_distortion(x, **settings):
    """The totals (a ToneTotal) of one call over the recording x with ToneBatch(**settings)."""
    return ToneBatch(**settings).run(x).total
