"""The spectrum widget's processing chain (friture/spectrum.py:125-184) without its Qt shell.

`SpectrumAnalyzer.handle_new_data(floatdata)` does what Spectrum_Widget's slot does per audio chunk:
push into the ring, transform every realizable frame (one batched launch of the float64 STFT kernel
over the contiguous ring window instead of a Python loop of analyzelive calls), exponential smoothing
across the new frames, dB + weighting (or the dual-channel ratio), spectral peak and the harmonic
product spectrum pitch — the last four fused in frt_spectrum_post.

`SpectrumBatch` runs the same chain over whole recordings, many streams at a time, in device calls
(frt_spectrum_batch, spectrumbatch.hip); its dB rows are what `plotcurves.CurveBatch` reads.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib, tables
from ._batchio import RecordingFront, carried, check_keep, check_samples, frame_schedule, null_stream, to_host
from .audioproc import audioproc
from .constants import SAMPLING_RATE
from .ringbuffer import RingBuffer
from .stft import StftEngine

DEFAULT_FFT_SIZE = 8192         # spectrum_settings.py:27-37
DEFAULT_RESPONSE_TIME = 0.025


def smoothing_setup(fft_size, overlap, response_time):
    """(alpha, kernel) of setresponsetime (spectrum.py:196-222)."""
    w = 0.65
    n = response_time * SAMPLING_RATE / (fft_size * (1. - overlap))
    alpha = 1. - (1. - w) ** (1. / (n + 1))
    return alpha, (1. - alpha) ** np.arange(2 * 4096 - 1, -1, -1)


def weighting_row(curves, weighting):
    """The dB row that `weighting` (0 none, 1 A, 2 B, else C) adds, from the (A, B, C) curves."""
    A, B, C = curves
    return {0: np.zeros(A.shape), 1: A, 2: B}.get(weighting, C)


class SpectrumAnalyzer:
    def __init__(self, fft_size: int = DEFAULT_FFT_SIZE, overlap: float = 3. / 4., weighting: int = 1,
                 response_time: float = DEFAULT_RESPONSE_TIME, dual_channels: bool = False):
        self._lib = _lib.init()
        self.ringbuffer = RingBuffer()
        self.proc = audioproc()
        self.overlap = overlap
        self.weighting = weighting
        self.dual_channels = dual_channels
        self.response_time = response_time
        self.old_index = 0
        self.setfftsize(fft_size)
        self.fmax = self.fpitch = 0.0
        self.dB_spectrogram = None

    # ---- configuration (names of friture/spectrum.py) ----------------------------------------------
    def setfftsize(self, fft_size):
        self.fft_size = fft_size
        self.proc.set_fftsize(fft_size)
        self.freq = self.proc.get_freq_scale()
        self.hop = int(fft_size * (1. - self.overlap))
        self._engine = StftEngine(fft_size, self.hop, 1, 64)
        self.update_weighting()
        self.dispbuffers1 = np.zeros(len(self.freq))
        self.dispbuffers2 = np.zeros(len(self.freq))
        self.setresponsetime(self.response_time)

    def setresponsetime(self, response_time):
        self.response_time = response_time
        self.alpha, self.kernel = smoothing_setup(self.fft_size, self.overlap, response_time)

    def setweighting(self, weighting):
        self.weighting = weighting
        self.update_weighting()

    def update_weighting(self):
        self.w = weighting_row(self.proc.get_freq_weighting(), self.weighting)

    # ---- the slot -------------------------------------------------------------------------------------
    def _push(self, floatdata):
        """The ring push and the frame bookkeeping of the slot: (window, realizable) with `window` the ring's samples of the
        `realizable` new frames, or None while no frame completes."""
        self.ringbuffer.push(floatdata, 0.)
        index = self.ringbuffer.offset
        available = index - self.old_index
        if available < 0:
            available = 0
            self.old_index = index
        needed = self.fft_size * (1. - self.overlap)
        realizable = int(np.floor(available / needed))
        if realizable <= 0:
            return None
        # frame i of the reference ends at old_index + i*hop: all frames form one contiguous window
        span = self.fft_size + (realizable - 1) * self.hop
        last = self.old_index + (realizable - 1) * self.hop
        window = self.ringbuffer.data_indexed(last, span)
        self.old_index += realizable * self.hop
        return window, realizable

    def handle_new_data(self, floatdata):
        new = self._push(floatdata)
        if new is None:
            return None
        window, _ = new
        sp1, db, peak, pitch = self._post(self._engine.psd(window[0:1, :].copy())[0], self.dispbuffers1, self.w, None)
        self.dispbuffers1 = sp1
        if self.dual_channels and window.shape[0] > 1:
            sp2, db, peak, _ = self._post(self._engine.psd(window[1:2, :].copy())[0], self.dispbuffers2, None, sp1)
            self.dispbuffers2 = sp2
        self.dB_spectrogram = db
        self.fmax = self.freq[peak]
        self.fpitch = max(self.freq[pitch], 1e-20)
        return self.freq, db, self.fmax, self.fpitch

    def _post(self, psd, previous, weight, ref):
        psd = np.ascontiguousarray(psd, np.float64)             # [frames, bins]
        nf, nb = psd.shape
        prev = np.ascontiguousarray(previous, np.float64)
        sm, db = np.empty(nb), np.empty(nb)
        peak, pitch = ctypes.c_int(0), ctypes.c_int(0)
        wp = None if weight is None else np.ascontiguousarray(weight, np.float64)
        rp = None if ref is None else np.ascontiguousarray(ref, np.float64)
        _lib.check(self._lib.frt_spectrum_post(
            psd.ctypes.data, 0, nf, nb, nb, self.kernel.ctypes.data, len(self.kernel), float(self.alpha), prev.ctypes.data,
            None if wp is None else wp.ctypes.data, None if rp is None else rp.ctypes.data, sm.ctypes.data, db.ctypes.data,
            ctypes.byref(peak), ctypes.byref(pitch)))
        return sm, db, peak.value, pitch.value


class SpectrumAnalyzerStream(SpectrumAnalyzer):
    """The same slot with its spectra resident in HBM.  The samples' ring stays on the host (a push is a numpy copy: the
    widget completes a frame only every few chunks, and a device call per chunk would cost more than the ring is worth);
    when frames complete, their window goes up once through page-locked memory (frt_stft_run, host samples -> device
    spectra, no wait), and smoothing, dB + weighting, peak and harmonic-product pitch (frt_spectrum_post) read and write
    device buffers — the PSD frames and the smoothed spectra never leave the device; per completed frame one window goes
    up, the dB spectrum and two indices come down, one synchronisation."""

    def __init__(self, *args, **kw):
        import torch
        self._torch = torch
        self._dev = torch.device("cuda", torch.cuda.current_device())
        super().__init__(*args, **kw)

    def setfftsize(self, fft_size):
        super().setfftsize(fft_size)
        torch = self._torch
        nb = len(self.freq)
        self._d_disp1 = torch.zeros(nb, dtype=torch.float64, device=self._dev)
        self._d_disp2 = torch.zeros(nb, dtype=torch.float64, device=self._dev)
        self._d_next = torch.zeros(nb, dtype=torch.float64, device=self._dev)       # the smoothed spectrum being written
        self._d_psd = None                                                           # [frames, bins] of the last call
        self._db = np.empty(nb)

    def update_weighting(self):
        super().update_weighting()
        self._d_w = self._torch.from_numpy(np.ascontiguousarray(self.w, np.float64)).to(self._dev)

    def handle_new_data(self, floatdata):
        new = self._push(floatdata)
        if new is None:
            return None
        window, realizable = new
        peak, pitch = self._post_dev(self._psd_dev(window[0], realizable), self._d_disp1, self._d_w, None)
        self._d_disp1, self._d_next = self._d_next, self._d_disp1
        if self.dual_channels and window.shape[0] > 1:
            peak, _ = self._post_dev(self._psd_dev(window[1], realizable), self._d_disp2, None, self._d_disp1)
            self._d_disp2, self._d_next = self._d_next, self._d_disp2
        db = self._db.copy()
        self.dB_spectrogram = db
        self.fmax = self.freq[peak]
        self.fpitch = max(self.freq[pitch], 1e-20)
        return self.freq, db, self.fmax, self.fpitch

    def _psd_dev(self, samples, n_frames):
        """PSD frames [n_frames, bins] of a host window, left on the device (enqueued on the engine's stream, not waited for).
        frt_spectrum_post launches on the null stream, which is ordered behind blocking streams only (friture_hip.h): the
        engine is put back on the null stream first, whatever a caller may have installed with frt_stft_set_stream."""
        torch = self._torch
        x = np.ascontiguousarray(samples, np.float64)
        nb = len(self.freq)
        if self._d_psd is None or self._d_psd.shape[0] < n_frames:
            self._d_psd = torch.empty((n_frames, nb), dtype=torch.float64, device=self._dev)
        nf = ctypes.c_int64(0)
        e = self._engine
        _lib.check(e._lib.frt_stft_set_stream(e._h, None))
        _lib.check(e._lib.frt_stft_run(e._h, 0, x.ctypes.data, x.shape[0], x.shape[0], ctypes.c_void_p(self._d_psd.data_ptr()),
                                       ctypes.byref(nf)))
        assert nf.value == n_frames
        return self._d_psd[:n_frames]

    def _post_dev(self, psd, disp, weight, ref):
        nf, nb = psd.shape
        peak, pitch = ctypes.c_int(0), ctypes.c_int(0)
        vp = ctypes.c_void_p
        _lib.check(self._lib.frt_spectrum_post(
            vp(psd.data_ptr()), 0, nf, nb, nb, self.kernel.ctypes.data, len(self.kernel), float(self.alpha), vp(disp.data_ptr()),
            None if weight is None else vp(weight.data_ptr()), None if ref is None else vp(ref.data_ptr()), vp(self._d_next.data_ptr()),
            self._db.ctypes.data, ctypes.byref(peak), ctypes.byref(pitch)))
        return peak.value, pitch.value


# ---- the same chain over whole recordings ---------------------------------------------------------------------------------

class SpectrumState(NamedTuple):
    """What a spectrum widget carries between two calls: its smoothed spectra, the samples it still needs and how many of them it
    has received but not consumed."""
    smoothed: object        # [S, rows, B] float64
    tail: object            # [S, rows, fft_size + pending] float64: samples [old_index - fft_size, offset), zeros before the start
    pending: int            # offset - old_index (below hop after a refresh whenever fft_size (1 - overlap) is a whole number)


class SpectrumResult(NamedTuple):
    db: object              # [S, R', B] float64 (R' = R, or 1 with keep="last"); [R', B] for one stream given without its axis
    peak_index: object      # [S, R'] int32
    pitch_index: object     # [S, R'] int32
    fmax: object            # [S, R'] float64: freq[peak_index]
    fpitch: object          # [S, R'] float64: max(freq[pitch_index], 1e-20)
    refresh_chunk: object   # [R] int64 (host): the chunk that caused each refresh
    state: SpectrumState


class SpectrumBatch:
    """S streams of a whole recording through the spectrum widget's chain in device calls, as widgets fed chunk by chunk would
    have seen it: the float64 STFT engine over the frames the schedule consumes, then frt_spectrum_batch (smoothing, dB +
    weighting or the dual-channel ratio, peak and harmonic-product pitch per refresh).  Fixed settings, no pause.
    run(x, chunk=512 | ends=..., state=None, keep="all" | "last") takes [S, T] ([S, 2, T] with dual_channels; the stream axis
    may be left out for one stream), float32 or float64, numpy array or CUDA tensor.  Results are numpy for numpy input and CUDA
    tensors for CUDA input; a CUDA `db` is what CurveBatch.run reads in place.  The PSD frames between the two stages live in at
    most `scratch_bytes` of device memory (or one refresh, if that is larger): longer recordings go through in time slabs, with
    the same bits whatever the slab size."""

    def __init__(self, fft_size: int = DEFAULT_FFT_SIZE, overlap: float = 3. / 4., weighting: int = 1,
                 response_time: float = DEFAULT_RESPONSE_TIME, dual_channels: bool = False):
        self.fft_size = int(fft_size)
        self.overlap = overlap
        self.weighting = weighting
        self.response_time = response_time
        self.dual_channels = bool(dual_channels)
        self.rows = 2 if self.dual_channels else 1
        self.needed = self.fft_size * (1. - overlap)                # a float, as in the widget
        self.hop = int(self.needed)
        if self.fft_size < 4 or self.fft_size % 2 or self.hop < 1:
            raise ValueError(f"fft_size {fft_size} with overlap {overlap}: no frame advance")
        self.freq = tables.rfft_frequencies(self.fft_size)
        self.w = weighting_row(tables.weighting_db(self.freq, floor=1e-50), weighting)
        self.n_bins = len(self.freq)
        self.alpha, self.kernel = smoothing_setup(self.fft_size, overlap, response_time)
        self._engines = {}
        self._dev_tables = {}

    # ---- host only ------------------------------------------------------------------------------------------------------------
    def schedule(self, n_samples, chunk=512, ends=None, state=None):
        """(frame_start [R + 1], refresh_chunk [R]) of a stream of n_samples seen chunk by chunk (`ends`: the chunks' end indices,
        for ragged chunks; default: the ends of `chunk`-sample chunks, a short last chunk is a short chunk).  Refresh r consumes
        the frames frame_start[r] .. frame_start[r + 1] - 1; frame j is the fft_size samples ending at j * hop - pending, zeros
        before the stream's start, so a fresh widget's frame 0 is all zeros."""
        return frame_schedule(n_samples, self.needed, self.hop, chunk, ends, 0 if state is None else state.pending)

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def _check_input(self, x, state):
        x, is_np, squeeze, pending = check_samples("SpectrumBatch", x, state, self.dual_channels)
        if state is not None:
            want_sm, want_tail = (x.shape[0], self.rows, self.n_bins), (x.shape[0], self.rows, self.fft_size + pending)
            if pending < 0 or tuple(state.smoothed.shape) != want_sm or tuple(state.tail.shape) != want_tail:
                raise ValueError(f"state of another shape: smoothed {tuple(state.smoothed.shape)} (want {want_sm}), tail "
                                 f"{tuple(state.tail.shape)} (want {want_tail}), pending {pending}")
        return x, is_np, squeeze, pending

    def run(self, x, chunk=512, ends=None, state=None, keep="all", scratch_bytes=1 << 30):
        check_keep(keep, "all", "last")
        x, is_np, squeeze, pending = self._check_input(x, state)
        frame_start, refresh_chunk = self.schedule(x.shape[-1], chunk, ends, state)
        import torch
        lib = _lib.init()
        S, rows, B, R = x.shape[0], self.rows, self.n_bins, len(refresh_chunk)
        f64, vp = torch.float64, ctypes.c_void_p
        with null_stream(x, is_np) as dev:
            front = RecordingFront(x, is_np, dev, pending, self.fft_size, self.hop, frame_start, ends)
            sm = carried(dev, None if state is None else state.smoothed, (S, rows, B))
            front.load_tail(None if state is None else state.tail)
            Ro = R if keep == "all" else min(R, 1)
            db = torch.empty((S, Ro, B), dtype=f64, device=dev)
            peak = torch.empty((S, Ro), dtype=torch.int32, device=dev)
            pitch = torch.empty((S, Ro), dtype=torch.int32, device=dev)
            if R:
                wd = None if self.dual_channels else self._table(dev, "w", self.w)
                for r0, r1, fa, fb, psd in front.transform(self._engine(S * rows), _lib.FRT_STFT_PSD, B, scratch_bytes):
                    nf, nr = fb - fa, r1 - r0
                    local = np.ascontiguousarray(frame_start[r0:r1 + 1] - fa)
                    if keep == "all":
                        pk = torch.empty((S, nr), dtype=torch.int32, device=dev)
                        pt = torch.empty((S, nr), dtype=torch.int32, device=dev)
                        dbp, ld_db = db.data_ptr() + r0 * B * 8, R * B
                    else:
                        pk, pt, dbp, ld_db = peak, pitch, db.data_ptr(), 0
                    _lib.check(lib.frt_spectrum_batch(
                        psd, 1, S, rows, nf, B, B, nf * B, local.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), nr,
                        self.kernel.ctypes.data, len(self.kernel), float(self.alpha), None if wd is None else vp(wd.data_ptr()),
                        vp(sm.data_ptr()), int(keep == "last"), vp(dbp), ld_db, vp(pk.data_ptr()), vp(pt.data_ptr())))
                    if keep == "all":
                        peak[:, r0:r1], pitch[:, r0:r1] = pk, pt
            new_tail, pending = front.new_tail()
            new_state = SpectrumState(sm, new_tail.reshape(S, rows, new_tail.shape[1]), pending)
            if is_np:
                db, peak, pitch, new_state = to_host((db, peak, pitch, new_state))
                fmax_hz, fpitch_hz = self.freq[peak], np.maximum(self.freq[pitch], 1e-20)
            else:
                fd = self._table(dev, "freq", self.freq)
                fmax_hz, fpitch_hz = fd[peak.long()], torch.clamp_min(fd[pitch.long()], 1e-20)
        if squeeze:
            db, peak, pitch, fmax_hz, fpitch_hz = db[0], peak[0], pitch[0], fmax_hz[0], fpitch_hz[0]
        return SpectrumResult(db, peak, pitch, fmax_hz, fpitch_hz, refresh_chunk, new_state)

    def _engine(self, channels):
        if channels not in self._engines:
            self._engines[channels] = StftEngine(self.fft_size, self.hop, channels, 64)
        return self._engines[channels]

    def _table(self, dev, name, values):
        import torch
        if (dev, name) not in self._dev_tables:
            self._dev_tables[(dev, name)] = torch.from_numpy(np.ascontiguousarray(values, np.float64)).to(dev)
        return self._dev_tables[(dev, name)]
