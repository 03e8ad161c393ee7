"""The spectrogram widget's processing chain (friture/spectrogram.py:131-177) without its Qt shell:
ring buffer, batched float64 STFT of every realizable frame, dB + weighting + normalisation, then the
Transform_Pipeline (frequency resampler -> online time resampler -> colour transform) to pixels.

`SpectrogramBatch` runs the same chain over whole recordings, many streams at a time, in device calls
(frt_specgram_batch, specgrambatch.hip)."""
from __future__ import annotations

from fractions import Fraction
from typing import NamedTuple

import numpy as np

from ._batchio import RecordingFront, carried, check_keep, check_samples, frame_schedule, null_stream, to_host
from .audioproc import audioproc
from .constants import SAMPLING_RATE
from .plotting import frequency_scales as fscales
from .ringbuffer import RingBuffer
from .signal.color_tranform import Color_Transform
from .signal.frequency_resampler import Frequency_Resampler
from .signal.online_linear_2D_resampler import Online_Linear_2D_resampler, advance_indices
from .signal.transform_pipeline import Transform_Pipeline
from .stft import StftEngine

DEFAULT_FFT_SIZE = 4096        # spectrogram_settings.py:27-34
DEFAULT_TIMERANGE = 10.


def _torch_device():
    """(torch, the device the HIP library is bound to) when torch with a GPU is importable, else None: the device-resident hand-over
    between the transform and the fused pipeline call needs a device allocation, which this class borrows from torch; without
    torch the frames take the host path (one more round trip per chunk, same pixels)."""
    try:
        import torch
    except ImportError:
        return None
    if not torch.cuda.is_available():
        return None
    from . import _lib
    return torch, torch.device("cuda", _lib.bound_device)


class Spectrogram:
    def __init__(self, fft_size=DEFAULT_FFT_SIZE, overlap=Fraction(3, 4), spec_min=-140., spec_max=0., weighting=0,
                 scale=fscales.Mel, minfreq=20., maxfreq=20000., screen_width=800, screen_height=400,
                 timerange_s=DEFAULT_TIMERANGE):
        self.ringbuffer = RingBuffer()
        self.proc = audioproc()
        self.overlap_frac = Fraction(overlap)
        self.spec_min, self.spec_max, self.weighting = spec_min, spec_max, weighting
        self.screen_width, self.screen_height, self.timerange_s = screen_width, screen_height, timerange_s
        self.frequency_resampler = Frequency_Resampler(scale, minfreq, maxfreq, screen_height)
        self.screen_resampler = Online_Linear_2D_resampler()
        self.audio_pipeline = Transform_Pipeline([self.frequency_resampler, self.screen_resampler, Color_Transform()])
        self.old_index = 0
        self.setfftsize(fft_size)

    def setfftsize(self, fft_size):
        self.fft_size = fft_size
        self.proc.set_fftsize(fft_size)
        self.freq = self.proc.get_freq_scale()
        self.frequency_resampler.setfreq(self.freq)
        self.hop = int(fft_size * (1. - float(self.overlap_frac)))
        self._engine = StftEngine(fft_size, self.hop, 1, 64)
        A, B, C = self.proc.get_freq_weighting()
        self.w = {0: np.zeros(A.shape), 1: A, 2: B}.get(self.weighting, C)
        self._engine.set_epilogue(self.w, self.spec_min, self.spec_max, None)
        self.sfft_rate_frac = Fraction(SAMPLING_RATE, fft_size) / (Fraction(1) - self.overlap_frac) / 1000

    def handle_new_data(self, floatdata):
        self.ringbuffer.push(floatdata, 0.)
        index = self.ringbuffer.offset
        available = index - self.old_index
        if available < 0:
            available = 0
            self.old_index = index
        needed = self.fft_size * (1. - float(self.overlap_frac))
        realizable = int(np.floor(available / needed))
        if realizable <= 0:
            return None
        span = self.fft_size + (realizable - 1) * self.hop
        last = self.old_index + (realizable - 1) * self.hop
        window = self.ringbuffer.data_indexed(last, span)
        self.old_index += realizable * self.hop
        self.screen_resampler.set_height(self.screen_height)
        screen_rate_frac = Fraction(max(self.screen_width, 1), int(self.timerange_s * 1000))
        self.screen_resampler.set_ratio(self.sfft_rate_frac, screen_rate_frac)
        self.frequency_resampler.setnsamples(self.screen_height)
        if self.audio_pipeline.fusable() and _torch_device() is not None:
            # one wait per chunk: the frames' (dB + w - min)/(max - min) stay on the device, frame-major as the kernel writes them
            # (enqueued, not waited for), and the fused pipeline call reads them there (until round 4: two host round trips)
            return self.audio_pipeline.push_frames_device(self._norm_dev(window[0], realizable), len(self.freq), realizable)
        # (dB + w - min)/(max - min) per frame, reference layout (bins, frames)
        norm_spectrogram = self._engine.norm(window[0:1, :].copy())[0].T
        return self.audio_pipeline.push(norm_spectrogram)

    def _norm_dev(self, samples, n_frames):
        """Normalised dB frames [n_frames, bins] of a host window, left on the device.  frt_screen_columns launches on the null
        stream, which is ordered behind blocking streams only (friture_hip.h): the engine is put on the null stream first."""
        import ctypes

        from . import _lib
        from ._lib import FRT_STFT_NORM
        torch, device = _torch_device()
        x = np.ascontiguousarray(samples, np.float64)
        nb = len(self.freq)
        d = getattr(self, "_d_norm", None)
        if d is None or d.shape[0] < n_frames or d.shape[1] != nb:
            d = self._d_norm = torch.empty((max(n_frames, 8), nb), dtype=torch.float64, device=device)      # the ENGINE's device
        nf = ctypes.c_int64(0)
        e = self._engine
        _lib.check(e._lib.frt_stft_set_stream(e._h, None))
        _lib.check(e._lib.frt_stft_run(e._h, FRT_STFT_NORM, x.ctypes.data, x.shape[0], x.shape[0], ctypes.c_void_p(d.data_ptr()),
                                       ctypes.byref(nf)))
        assert nf.value == n_frames
        return ctypes.c_void_p(d.data_ptr())


class SpectrogramStream:
    """The same chain as ONE device-resident object (frt_specgram_*, specgram.hip): the samples' mirror ring, the spectra,
    the frequency map, the time resampler's carried column and the LUT live in HBM; a chunk costs one upload of its own
    samples, three launches and one download of the new pixel columns.  `handle_new_data` returns the block the widget
    hands to CanvasScaledSpectrogram.addData AFTER its flip of the frequency axis (spectrogram_image.py:82-92):
    uint32 [screen_height, columns], row 0 = highest frequency, or None when the chunk completed no frame."""

    def __init__(self, fft_size=DEFAULT_FFT_SIZE, overlap=Fraction(3, 4), spec_min=-140., spec_max=0., weighting=0,
                 scale=fscales.Mel, minfreq=20., maxfreq=20000., screen_width=800, screen_height=400,
                 timerange_s=DEFAULT_TIMERANGE, ring_length=None):
        import ctypes
        from . import _lib
        self._ct, self._libmod = ctypes, _lib
        self._lib = _lib.init()
        self.proc = audioproc()
        self.overlap_frac = Fraction(overlap)
        self.spec_min, self.spec_max, self.weighting = spec_min, spec_max, weighting
        self.scale, self.minfreq, self.maxfreq = scale, minfreq, maxfreq
        self.screen_width, self.screen_height, self.timerange_s = screen_width, screen_height, timerange_s
        self._h = ctypes.c_void_p()
        self._ring_length = ring_length
        self._colors = Color_Transform().colors
        self.setfftsize(fft_size)

    def _release(self):
        if self._h.value:
            self._lib.frt_specgram_destroy(self._h)
            self._h = self._ct.c_void_p()

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def setfftsize(self, fft_size):
        ct, check = self._ct, self._libmod.check
        self._release()
        self.fft_size = fft_size
        self.proc.set_fftsize(fft_size)
        self.freq = np.ascontiguousarray(self.proc.get_freq_scale(), np.float64)
        ring = self._ring_length or max(10000, 4 * fft_size)           # ringbuffer.py:34 starts at 10000 and grows on demand
        check(self._lib.frt_specgram_create(ct.byref(self._h), fft_size, float(self.overlap_frac), int(ring)))
        A, B, C = self.proc.get_freq_weighting()
        w = np.ascontiguousarray({0: np.zeros(A.shape), 1: A, 2: B}.get(self.weighting, C), np.float64)
        lut = np.ascontiguousarray(self._colors, np.uint32)
        DP, UP = ct.POINTER(ct.c_double), ct.POINTER(ct.c_uint32)
        check(self._lib.frt_specgram_set_epilogue(self._h, w.ctypes.data_as(DP), float(self.spec_min), float(self.spec_max),
                                                  lut.ctypes.data_as(UP)))
        self.sfft_rate_frac = Fraction(SAMPLING_RATE, fft_size) / (Fraction(1) - self.overlap_frac) / 1000
        self._screen = None

    def _sync_screen(self):
        ct, check = self._ct, self._libmod.check
        key = (self.screen_height, self.scale, self.minfreq, self.maxfreq)
        if key != self._screen:
            lo, hi = self.scale.transform(self.minfreq), self.scale.transform(self.maxfreq)
            targets = np.ascontiguousarray(self.scale.inverse(np.linspace(lo, hi, self.screen_height)), np.float64)
            DP = ct.POINTER(ct.c_double)
            check(self._lib.frt_specgram_set_screen(self._h, self.freq.ctypes.data_as(DP), targets.ctypes.data_as(DP), int(self.screen_height)))
            self._screen = key
        screen_rate_frac = Fraction(max(self.screen_width, 1), int(self.timerange_s * 1000))
        # set_ratio(L, M) divides float(L) / M (online_linear_2D_resampler.py:38): the same division on the other side
        check(self._lib.frt_specgram_set_ratio(self._h, float(self.sfft_rate_frac), float(screen_rate_frac)))

    def handle_new_data(self, floatdata):
        ct = self._ct
        x = np.ascontiguousarray(np.asarray(floatdata, np.float64)[0])
        self._sync_screen()
        frames_max = x.size // max(1, int(self.fft_size * (1. - float(self.overlap_frac)))) + 2
        ratio = float(self.sfft_rate_frac) / float(Fraction(max(self.screen_width, 1), int(self.timerange_s * 1000)))
        max_cols = int(frames_max / ratio) + 4
        out = np.empty((self.screen_height, max_cols), np.uint32)
        n_cols, n_frames = ct.c_int(0), ct.c_int(0)
        self._libmod.check(self._lib.frt_specgram_push(self._h, x.ctypes.data, x.size, out.ctypes.data, max_cols, ct.byref(n_cols),
                                                        ct.byref(n_frames)))
        if n_frames.value == 0:
            return None
        return out[:, :n_cols.value]


# ---- the same chain over whole recordings ---------------------------------------------------------------------------------

class SpectrogramState(NamedTuple):
    """What a spectrogram widget carries between two calls: the samples it still needs, how many of them it has received but
    not consumed, and the time resampler's carried column and indices."""
    tail: object            # [S, fft_size + pending] float64: samples [old_index - fft_size, offset), zeros before the start
    pending: int            # offset - old_index
    old_column: object      # [S, screen_height] float64: the frequency-resampled last frame
    orig_index: float       # Online_Linear_2D_resampler.orig_index
    resampled_index: float  # Online_Linear_2D_resampler.resampled_index


class ColumnTable(NamedTuple):
    """Which frame feeds which pixel column (host arrays)."""
    src: object             # [P] int64: the source frame (index into the schedule's frames); the frame before it is the other end
    a: object               # [P] float64: pixel = frame[src] (1 - a) + frame[src - 1] a
    filler: object          # [P] bool: a column the reference allocated and never wrote (lut[0])
    column_refresh: object  # [P] int64: the refresh that emitted the column
    orig_index: float       # the resampler's indices after the last refresh
    resampled_index: float


class SpectrogramResult(NamedTuple):
    pixels: object          # [S, screen_height, P'] uint32, row 0 = highest frequency ([screen_height, P'] for one stream given without its axis)
    column_refresh: object  # [P'] int64 (host): the refresh that emitted each column
    refresh_chunk: object   # [R] int64 (host): the chunk that caused each refresh
    state: SpectrogramState


class SpectrogramBatch:
    """S streams of a whole recording through the spectrogram widget's chain in device calls, as widgets fed chunk by chunk would
    have painted it: per time slab one float64 STFT with the normalising epilogue over all streams, then frt_specgram_batch
    (specgrambatch.hip: np.interp onto the screen rows, the time resampler's lerp, clip + LUT, flipped rows).  Fixed settings, no
    pause, no resize.  run(x, chunk=512 | ends=..., state=None, keep="all" | "screen") takes [S, T] (the stream axis may be left
    out), float32 or float64, numpy array or CUDA tensor; pixels are numpy for numpy input and a CUDA tensor for CUDA input.
    keep="screen" produces only the last min(P, screen_width) columns (what the rolling canvas shows at the end) and transforms
    only the frames they need.  The normalised frames between the two stages live in at most `scratch_bytes` of device memory (or
    one refresh, if that is larger): longer recordings go through in time slabs, with the same bits whatever the slab size."""

    def __init__(self, fft_size=DEFAULT_FFT_SIZE, overlap=Fraction(3, 4), spec_min=-140., spec_max=0., weighting=0,
                 scale=fscales.Mel, minfreq=20., maxfreq=20000., screen_width=800, screen_height=400, timerange_s=DEFAULT_TIMERANGE):
        from . import palette, tables
        self.fft_size = int(fft_size)
        self.overlap_frac = Fraction(overlap)
        self.spec_min, self.spec_max, self.weighting = spec_min, spec_max, weighting
        self.scale, self.minfreq, self.maxfreq = scale, minfreq, maxfreq
        self.screen_width, self.screen_height, self.timerange_s = int(screen_width), int(screen_height), timerange_s
        self.needed = self.fft_size * (1. - float(self.overlap_frac))       # a float, as in the widget
        self.hop = int(self.needed)
        if self.fft_size < 4 or self.fft_size % 2 or self.hop < 1:
            raise ValueError(f"fft_size {fft_size} with overlap {overlap}: no frame advance")
        if self.screen_height < 1 or int(timerange_s * 1000) < 1:
            raise ValueError(f"screen height {screen_height}, time range {timerange_s} s")
        self.freq = tables.rfft_frequencies(self.fft_size)
        self.n_bins = len(self.freq)
        A, B, C = tables.weighting_db(self.freq, floor=1e-50)
        self.w = {0: np.zeros(A.shape), 1: A, 2: B}.get(weighting, C)
        self.targets = np.ascontiguousarray(scale.inverse(np.linspace(scale.transform(minfreq), scale.transform(maxfreq),
                                                                      self.screen_height)), np.float64)
        self.lut = np.ascontiguousarray(palette.cmr_lut(), np.uint32)
        sfft_rate_frac = Fraction(SAMPLING_RATE, self.fft_size) / (Fraction(1) - self.overlap_frac) / 1000
        screen_rate_frac = Fraction(max(self.screen_width, 1), int(timerange_s * 1000))
        self.ratio = float(sfft_rate_frac) / float(screen_rate_frac)        # set_ratio: float(L) / M (online_linear_2D_resampler.py:38)
        self._engines = {}

    # ---- host only ------------------------------------------------------------------------------------------------------------
    def schedule(self, n_samples, chunk=512, ends=None, state=None):
        """(frame_start [R + 1], refresh_chunk [R]): SpectrumBatch.schedule's, the two widgets keep the same bookkeeping.  Refresh r
        consumes the frames frame_start[r] .. frame_start[r + 1] - 1; frame j is the fft_size samples ending at j * hop - pending."""
        return frame_schedule(n_samples, self.needed, self.hop, chunk, ends, 0 if state is None else state.pending)

    def columns(self, n_samples, chunk=512, ends=None, state=None):
        """The ColumnTable of the recording: the time resampler's scalar recurrence replayed refresh by refresh (the widget pushes the
        frames of one refresh at once).  The reference sizes a push's block from processable(m) and fills it frame by frame; in
        float arithmetic the two counts can differ by one: a column allocated and not written is a `filler`, a refresh that would
        write more columns than were allocated raises ValueError (the reference raises there too)."""
        frame_start, _ = self.schedule(n_samples, chunk, ends, state)
        orig, res = (0., 0.) if state is None else (float(state.orig_index), float(state.resampled_index))
        src, a, filler, col_refresh = [], [], [], []
        for r in range(len(frame_start) - 1):
            f0, m = int(frame_start[r]), int(frame_start[r + 1] - frame_start[r])
            total, s, w, orig, res = advance_indices(orig, res, self.ratio, m)
            if len(s) > total:
                raise ValueError(f"refresh {r}: the time resampler emits {len(s)} columns for {m} frames where the reference "
                                 f"allocates {total}")
            src += [f0 + j for j in s] + [f0 + m - 1] * (total - len(s))
            a += w + [0.] * (total - len(s))
            filler += [False] * len(s) + [True] * (total - len(s))
            col_refresh += [r] * total
        return ColumnTable(np.array(src, np.int64), np.array(a, np.float64), np.array(filler, bool), np.array(col_refresh, np.int64),
                           orig, res)

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def _check_input(self, x, state):
        x, is_np, squeeze, pending = check_samples("SpectrogramBatch", x, state)
        S = x.shape[0]
        if S < 1:
            raise ValueError("no stream")
        if state is not None:
            want_tail, want_old = (S, self.fft_size + pending), (S, self.screen_height)
            if pending < 0 or tuple(state.tail.shape) != want_tail or tuple(state.old_column.shape) != want_old:
                raise ValueError(f"state of another shape: tail {tuple(state.tail.shape)} (want {want_tail}), old_column "
                                 f"{tuple(state.old_column.shape)} (want {want_old}), pending {pending}")
        return x, is_np, squeeze, pending

    def run(self, x, chunk=512, ends=None, state=None, keep="all", scratch_bytes=1 << 30):
        check_keep(keep, "all", "screen")
        x, is_np, squeeze, pending = self._check_input(x, state)
        S, T = x.shape
        frame_start, refresh_chunk = self.schedule(T, chunk, ends, state)
        table = self.columns(T, chunk, ends, state)                 # raises before anything is enqueued
        import ctypes

        import torch

        from . import _lib
        lib = _lib.init()
        B, H = self.n_bins, self.screen_height
        R, F, P = len(refresh_chunk), int(frame_start[-1]), len(table.src)
        c_lo = 0 if keep == "all" else max(0, P - self.screen_width)                 # the first column produced
        f_lo = 0 if keep == "all" else (max(0, int(table.src[c_lo]) - 1) if c_lo < P else max(0, F - 1))   # the first frame transformed
        Po = P - c_lo
        col_start = np.searchsorted(table.column_refresh, np.arange(R + 1))          # the columns of each refresh
        src = np.where(table.filler, -1, table.src)
        vp = ctypes.c_void_p
        with null_stream(x, is_np) as dev:
            front = RecordingFront(x, is_np, dev, pending, self.fft_size, self.hop, frame_start, ends)
            front.load_tail(None if state is None else state.tail)
            old = carried(dev, None if state is None else state.old_column, (S, H))
            pixels = torch.empty((S, H, Po), dtype=torch.int32, device=dev)          # uint32 words (torch has no uint32 arithmetic)
            if R:
                old_next = torch.empty_like(old)
                for r0, r1, fa, fb, norm in front.transform(self._engine(S), _lib.FRT_STFT_NORM, B, scratch_bytes, f_lo):
                    ca, cb = max(int(col_start[r0]), c_lo), max(int(col_start[r1]), c_lo)
                    nf, nc = fb - fa, cb - ca
                    local = np.ascontiguousarray(np.where(src[ca:cb] < 0, -1, src[ca:cb] - fa), np.int32)
                    weights = np.ascontiguousarray(table.a[ca:cb])
                    _lib.check(lib.frt_specgram_batch(
                        norm, S, nf, B, B, nf * B, self.freq.ctypes.data, self.targets.ctypes.data, H,
                        local.ctypes.data if nc else None, weights.ctypes.data if nc else None, nc, vp(old.data_ptr()),
                        vp(old_next.data_ptr()), self.lut.ctypes.data, vp(pixels.data_ptr()) if nc else None, ca - c_lo, Po))
                    old, old_next = old_next, old
            new_tail, pending = front.new_tail()
            new_state = SpectrogramState(new_tail, pending, old, table.orig_index, table.resampled_index)
            if is_np:
                pixels, new_state = to_host((pixels, new_state))
                pixels = pixels.view(np.uint32)
            else:
                pixels = pixels.view(torch.uint32) if hasattr(torch, "uint32") else pixels
        if squeeze:
            pixels = pixels[0]
        return SpectrogramResult(pixels, table.column_refresh[c_lo:], refresh_chunk, new_state)

    def _engine(self, streams):
        if streams not in self._engines:
            eng = StftEngine(self.fft_size, self.hop, streams, 64)
            eng.set_epilogue(self.w, self.spec_min, self.spec_max, None)
            self._engines[streams] = eng
        return self._engines[streams]
