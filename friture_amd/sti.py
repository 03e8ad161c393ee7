"""Whether speech is intelligible in a measured room: the modulation transfer function of impulse responses and the Speech
Transmission Index from it, on the GPU (mtf.hip, frt_mtf_*, frt_sti_run; the definition: X5 in include/friture_hip.h).  The step
after DeconvolveBatch and room_acoustics: IEC 60268-16:2011 by Schroeder's indirect method, for whole batches of responses.

Modulation transfer (the kernel).  A row x[0 .. T) is float32 or float64, 1 <= T <= 2^24; all arithmetic is float64 and e[t] =
(double)x[t]^2.  A handle holds fs (default 48000; DecayBatch's range) and nf modulation frequencies F_j in Hz, 1 <= nf <= 16,
0 < F_j < fs / 2.  Per row, over [start, stop) with integers 0 <= start < stop <= T per row (default 0, T):
    S0 = sum e[t];  S_j = sum e[t] exp(-2 pi i F_j t / fs), t counted from the row's sample 0;  m_j = |S_j| / S0.
Outputs per row: m [nf] and energy = S0, float64.  A row that is all zero over the interval, or holds a non-finite sample there,
gives NaN in m (energy is then 0, NaN or inf); it never faults and never touches its neighbours.  A bad start / stop in a host
array is refused before the library; in a device array it makes the row dead (NaN in m and energy).  The bits of a row depend on
its own samples, start, stop and the frequencies only: not on the other rows, scratch_bytes, a row stride, the dtype (float32
widens exactly) or host against device input (the order of the sums: X5).

STI from m [S, 7, nf], the octave bands 1000 G^k, k = -3 .. 3, G = 10^0.3 (125 Hz .. 8 kHz), a small kernel of its own:
1. Corrections, at most one of two: snr_db [S, 7] or [7]: m' = m / (1 + 10^(-snr / 10)).  Or level_db with noise_db (None: no
   noise), absolute octave-band levels: I_k = 10^(L_k / 10), In_k = 10^(N_k / 10), Irt_k = 10^(A_k / 10) (RECEPTION_DB), Iam_1 = 0
   and for k > 1 Iam_k = (I_{k-1} + In_{k-1}) 10^(amdB(Ltot_{k-1}) / 10), Ltot = 10 log10(I + In), amdB(L) = 0.5 L - 65 for L < 63,
   1.8 L - 146.9 for 63 <= L < 67, 0.5 L - 59.8 for 67 <= L < 100, -10 from 100 on; m' = m I_k / (I_k + In_k + Iam_k + Irt_k).
2. snr_eff = 10 log10(m' / (1 - m')) clipped to [-15, 15] (m' >= 1 gives 15, m' <= 0 gives -15); TI = (snr_eff + 15) / 30.
3. MTI_k = the mean of TI over the mask's columns of band k ("full": all; "stipa": STIPA's two per band); a band with no
   column is refused.
4. STI = sum alpha_k MTI_k - sum beta_k sqrt(MTI_k MTI_{k+1}), at most 1.  A NaN in any used m makes that response's STI NaN
   and no other.
Out of scope: the direct method (STIPA test-signal generation and the analysis of a recording of it), revision 5's changes
(IIR band filters: speech_transmission(filters="butterworth"), X6, friture_amd/sosfilter.py), absolute levels derived from an uncalibrated response, a carried state, sample rates handled
in any way other than the fs argument.  There is no CPU fallback: run() and sti_from_mtf() go to the HIP library.

speech_transmission is composition like room_acoustics: DecayBatch finds onset and truncation, ConvolveBatch applies
decay.band_filter per octave, MtfBatch reads the delayed view in place, sti_from_mtf finishes; with filters="butterworth" /
"butterworth-reversed" the seven octaves are Butterworth band-passes run as one bank by SosBatch."""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import numpy as np

from . import _batchio, _lib, decay

TILE = 4096                                 # samples per tile of the sums (frt_mtf_tile)
MAX_SAMPLES = 1 << 24
MAX_FREQS = 16
BANDS = 7

MOD_FREQS = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)
WEIGHTS = {"male": ((0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173), (0.085, 0.078, 0.065, 0.011, 0.047, 0.095)),
           "female": ((0.0, 0.117, 0.223, 0.216, 0.328, 0.250, 0.194), (0.0, 0.099, 0.066, 0.062, 0.025, 0.076))}
RECEPTION_DB = (46.0, 27.0, 12.0, 6.5, 7.5, 8.0, 12.0)
# octave-band levels of speech relative to its A-weighted level; the female spectrum has no 125 Hz band
SPEECH_SPECTRUM_DB = {"male": (2.9, 2.9, -0.8, -6.8, -12.8, -18.8, -24.8), "female": (-math.inf, 5.3, -1.9, -9.1, -15.8, -16.7, -18.0)}
_STIPA_COLUMNS = ((4, 11), (2, 9), (0, 7), (5, 12), (3, 10), (1, 8), (6, 13))         # per band, into MOD_FREQS
STIPA = np.zeros((BANDS, len(MOD_FREQS)), bool)
for _k, _columns in enumerate(_STIPA_COLUMNS):
    STIPA[_k, list(_columns)] = True
STIPA.setflags(write=False)

MtfResult = namedtuple("MtfResult", "m energy")
StiResult = namedtuple("StiResult", "sti mti ti")
SpeechResult = namedtuple("SpeechResult", "centres sti mti ti m")


def octave_bands():
    """The (f_lo, f_hi) pairs of the seven octave bands 125 Hz .. 8 kHz, as decay.band_edges takes them."""
    G = 10.0 ** 0.3
    return [(1000.0 * G ** (k - 0.5), 1000.0 * G ** (k + 0.5)) for k in range(-3, 4)]


class MtfBatch:
    """MtfBatch(freqs=MOD_FREQS, fs=48000).run(x, start=None, stop=None, scratch_bytes=1 << 28) -> MtfResult(m, energy).  x: [R, T]
    or [T], float32 or float64, numpy array or CUDA tensor (strided row views are read in place).  The results are of x's kind:
    m float64 [R, nf], energy float64 [R] ([T] in: without the R axis).  start, stop: integers [R] (host arrays are checked here;
    int64 CUDA tensors go to the kernel as they are, with CUDA input).  The rows are cut into slabs whose scratch stays within
    scratch_bytes; the result has the same bits at any slab size."""

    def __init__(self, freqs=MOD_FREQS, fs=48000):
        _batchio.check_fs(fs)
        f = np.asarray(freqs)
        if f.ndim != 1 or f.dtype.kind not in "fiu" or not 1 <= f.size <= MAX_FREQS:
            raise ValueError(f"freqs must be 1 .. {MAX_FREQS} numbers, got {freqs!r}")
        f = np.ascontiguousarray(f, np.float64)
        if not np.all(np.isfinite(f) & (f > 0) & (f < fs / 2)):
            raise ValueError(f"every modulation frequency must lie above 0 and below fs / 2 = {fs / 2!r}, got {freqs!r}")
        self.fs, self.freqs = float(fs), f
        self._handle_ = None

    def _handle(self):
        if self._handle_ is None:
            self._handle_ = _lib.Handle("mtf", self.fs, self.freqs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(self.freqs))
        return self._handle_

    def run(self, x, start=None, stop=None, scratch_bytes=1 << 28):
        x, is_np, squeeze, _ = _batchio.check_samples("MtfBatch", x, None)
        R, T = x.shape
        _batchio.check_streams(R)
        _batchio.check_row_samples(T)
        _batchio.check_scratch_bytes(scratch_bytes)
        lo = None if start is None else _batchio.row_integers("start", start, R, 0, T - 1, device=True)
        hi = None if stop is None else _batchio.row_integers("stop", stop, R, 1, T, device=True)
        on_host = all(v is None or isinstance(v, np.ndarray) for v in (lo, hi))
        if is_np and not on_host:
            raise TypeError("start and stop on the device need x on the device")
        if on_host and np.any((T if hi is None else hi) <= (0 if lo is None else lo)):
            raise ValueError("stop must lie behind start in every row")
        h = self._handle()
        x, xptr, code, row, _ = _batchio.strided_rows(x)
        vp, nf = ctypes.c_void_p, len(self.freqs)

        def call(_, m, energy):
            _lib.check(h.lib.frt_mtf_run(h.h, vp(xptr), code, R, T, row, vp(_batchio.ptr(lo)), vp(_batchio.ptr(hi)), int(scratch_bytes),
                                         vp(_batchio.ptr(m)), vp(_batchio.ptr(energy))))

        def outputs():
            return _batchio.alloc(x, (R, nf)), _batchio.alloc(x, (R,))

        m, energy = _batchio.run_call(x, is_np, outputs, h.set_stream, call, None)
        return MtfResult(m[0], energy[0]) if squeeze else MtfResult(m, energy)


def _weights(weights):
    if isinstance(weights, str):
        if weights not in WEIGHTS:
            raise ValueError(f"weights={weights!r} ('male', 'female' or (alpha [7], beta [6]))")
        weights = WEIGHTS[weights]
    try:
        alpha, beta = (np.ascontiguousarray(v, np.float64) for v in weights)
    except (TypeError, ValueError):
        raise ValueError(f"weights={weights!r} ('male', 'female' or (alpha [7], beta [6]))") from None
    if alpha.shape != (BANDS,) or beta.shape != (BANDS - 1,) or not (np.all(np.isfinite(alpha)) and np.all(np.isfinite(beta))):
        raise ValueError(f"weights must be (alpha [7], beta [6]) of finite numbers, got shapes {alpha.shape}, {beta.shape}")
    return alpha, beta


def _mask(scheme, nf):
    if isinstance(scheme, str):
        if scheme == "full":
            return np.ones((BANDS, nf), np.uint8)
        if scheme != "stipa":
            raise ValueError(f"scheme={scheme!r} ('full', 'stipa' or a boolean mask [7, {nf}])")
        if nf != len(MOD_FREQS):
            raise ValueError(f"scheme='stipa' names columns of MOD_FREQS: m must have {len(MOD_FREQS)} modulation frequencies, got {nf}")
        return np.ascontiguousarray(STIPA, np.uint8)
    mask = np.asarray(scheme)
    if mask.dtype != bool or mask.shape != (BANDS, nf):
        raise ValueError(f"scheme must be 'full', 'stipa' or a boolean mask [7, {nf}], got {mask.dtype} {mask.shape}")
    if not np.all(mask.any(axis=1)):
        raise ValueError("every band needs at least one modulation frequency in the mask")
    return np.ascontiguousarray(mask, np.uint8)


def _band_values(name, v, like, is_np, S):
    """[S, 7] float64 of m's kind from [S, 7] or [7]."""
    if is_np:
        if hasattr(v, "cpu"):
            v = v.cpu().numpy()
        v = np.asarray(v, np.float64)
    else:
        import torch
        v = torch.as_tensor(v, dtype=torch.float64, device=like.device)
    if tuple(v.shape) not in ((S, BANDS), (BANDS,)):
        raise ValueError(f"{name} must be [{S}, 7] or [7], got {tuple(v.shape)}")
    if is_np:
        return np.ascontiguousarray(np.broadcast_to(v, (S, BANDS)))
    return v.expand(S, BANDS).contiguous()


def sti_from_mtf(m, snr_db=None, level_db=None, noise_db=None, weights="male", scheme="full"):
    """StiResult(sti [S], mti [S, 7], ti [S, 7, nf]) of modulation transfer values m [S, 7, nf] or [7, nf] (then without the S
    axis), a float64 numpy array or CUDA tensor; the results are of m's kind.  snr_db, or level_db with noise_db (None: no
    noise): [S, 7] or [7], at most one of the two corrections.  weights: "male", "female" or (alpha [7], beta [6]).  scheme:
    "full", "stipa" (nf = 14, MOD_FREQS) or a boolean mask [7, nf]."""
    is_np = isinstance(m, np.ndarray)
    if not is_np and not (type(m).__module__.startswith("torch") and m.is_cuda):
        raise TypeError("sti_from_mtf takes a numpy array or a CUDA tensor")
    if str(m.dtype).split(".")[-1] != "float64":
        raise TypeError(f"m must be float64, got {m.dtype}")
    if m.ndim not in (2, 3) or m.shape[-2] != BANDS or not 1 <= m.shape[-1] <= MAX_FREQS:
        raise ValueError(f"expected m [S, 7, nf] or [7, nf] with nf in 1 .. {MAX_FREQS}, got {tuple(m.shape)}")
    squeeze = m.ndim == 2
    if squeeze:
        m = m[None]
    S, nf = m.shape[0], m.shape[2]
    if not 1 <= S <= 1 << 24:
        raise ValueError(f"expected 1 .. 2^24 responses, got {S}")
    if snr_db is not None and (level_db is not None or noise_db is not None):
        raise ValueError("snr_db and level_db / noise_db are two corrections: give at most one")
    if noise_db is not None and level_db is None:
        raise ValueError("noise_db needs level_db: both are absolute octave-band levels")
    alpha, beta = _weights(weights)
    mask = _mask(scheme, nf)
    correction, a, b = 0, None, None
    if snr_db is not None:
        correction, a = 1, _band_values("snr_db", snr_db, m, is_np, S)
    elif level_db is not None:
        correction, a = 2, _band_values("level_db", level_db, m, is_np, S)
        b = None if noise_db is None else _band_values("noise_db", noise_db, m, is_np, S)
    m = np.ascontiguousarray(m) if is_np else m.contiguous()
    lib, vp, dp = _lib.init(), ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)

    def call(_, sti, mti, ti):
        _lib.check(lib.frt_sti_run(vp(_batchio.ptr(m)), S, nf, correction, vp(_batchio.ptr(a)), vp(_batchio.ptr(b)), alpha.ctypes.data_as(dp),
                                   beta.ctypes.data_as(dp), vp(mask.ctypes.data), vp(_batchio.ptr(sti)), vp(_batchio.ptr(mti)),
                                   vp(_batchio.ptr(ti)), None))

    def outputs():
        return _batchio.alloc(m, (S,)), _batchio.alloc(m, (S, BANDS)), _batchio.alloc(m, (S, BANDS, nf))

    sti, mti, ti = _batchio.run_call(m, is_np, outputs, lambda: None, call, None)
    return StiResult(sti[0], mti[0], ti[0]) if squeeze else StiResult(sti, mti, ti)


def speech_levels(laeq, voice="male"):
    """The octave-band levels [7] in dB (125 Hz .. 8 kHz) of speech at the A-weighted level laeq: laeq + SPEECH_SPECTRUM_DB.  The
    female spectrum has no 125 Hz band: -inf there, which the female weights do not count."""
    if voice not in SPEECH_SPECTRUM_DB:
        raise ValueError(f"voice={voice!r} ('male' or 'female')")
    if not (isinstance(laeq, (int, float, np.integer, np.floating)) and math.isfinite(laeq)):
        raise ValueError(f"laeq must be a finite number of dB, got {laeq!r}")
    return float(laeq) + np.array(SPEECH_SPECTRUM_DB[voice])


def speech_transmission(ir, fs=48000, truncate="auto", filters="fir", order=3, **corrections):
    """The Speech Transmission Index of responses ir [S, T] or [T]: SpeechResult(centres [7], sti [S], mti [S, 7], ti [S, 7, 14],
    m [S, 7, 14]) at MOD_FREQS.  One broadband DecayBatch.run gives the onset and the truncation (truncate=None: the whole row
    behind the onset).  filters="fir": per octave band, ConvolveBatch(band_filter(..)).run(ir).y[..., M : M + T] is read in place
    by MtfBatch with start = onset, stop = truncation.  filters="butterworth" / "butterworth-reversed": one bank run of SosBatch
    over the seven Butterworth band-passes of `order` (sosfilter.band_sos, forward or backwards in time) gives [S, 7, T] in
    float64, whose [7 S, T] view goes through one MtfBatch.run.  Then sti_from_mtf(m, **corrections) (snr_db, level_db, noise_db,
    weights, scheme)."""
    decay.check_filters(filters)
    centres, edges = decay.band_edges(octave_bands())
    broadband = decay.DecayBatch(fs=fs).run(ir, truncate=truncate)
    mtf = MtfBatch(MOD_FREQS, fs)
    m = [mtf.run(rows, start=spread(broadband.onset), stop=spread(broadband.truncation)).m
         for rows, spread in decay.band_front(ir, edges, fs, filters, order)]
    m = decay.band_axis(ir, BANDS, filters, m)
    res = sti_from_mtf(m, **corrections)
    return SpeechResult(centres, res.sti, res.mti, res.ti, m)
