"""friture/pitch_tracker.py:160-428 on the GPU: `PitchTracker`, `calcCosineKernel`,
`fastParabolicInterp`, plus the batch engine `PitchEngine`.

The tracker matches each frame's log-frequency spectrum against SWIPE-style harmonic kernels; the
table construction below (one-off, host side) produces the same numbers as the reference's loop over
harmonics, the per-frame work — spectrum, log-grid interpolation, the [candidates x grid] product,
peak refinement and the voiced/unvoiced gate — runs in the kernels of csrc/pitch.hip (frt_pitch_*).
The Qt widget around it (PitchTrackerWidget, :57-158) is out of scope, except for what it shows of whole
recordings: `PitchBatch` (the refresh schedule, the latest estimate and the curve of handle_new_data / update_curve, :109-119).
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import numpy as np

from . import _lib
from ._batchio import carried, check_keep, check_samples, checked_ends, null_stream, source, to_host
from .audioproc import audioproc
from .constants import SAMPLING_RATE
from .ringbuffer import RingBuffer

# defaults of friture/pitch_tracker_settings.py:27-34
DEFAULT_FFT_SIZE = 4096
DEFAULT_MIN_FREQ = 65
DEFAULT_MAX_FREQ = 1047
DEFAULT_DURATION = 10
DEFAULT_MIN_DB = -50.0
DEFAULT_C_RES = 10
DEFAULT_P_CONF = 0.50
DEFAULT_P_DELTA = 2

_HARMONICS = np.array([1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 13, 17, 19, 23])
_PEAK_WIDTH = 0.15
_VALLEY_WIDTH = 1 - _PEAK_WIDTH


def fastParabolicInterp(y1, y2, y3):
    """Vertex (offset from the centre sample, height) of the parabola through three neighbouring
    pitch strengths (pitch_tracker.py:160-193)."""
    curvature = (y1 - 2 * y2 + y3) / 2
    tilt = (y3 - y1) / 2
    vx = -tilt / (2 * curvature + np.finfo(np.float64).eps)
    return vx, curvature * vx ** 2 + tilt * vx + y2


def calcCosineKernel(f, freqList):
    """Kernel of candidate `f` over the frequency grid (pitch_tracker.py:195-264).

    Around every integer multiple i <= 23 of f, the grid points with -0.85 < freq/f - i < 0.15 carry a
    lobe: a cosine peak of half-width 0.15 (full height at the harmonics in use, a quarter elsewhere)
    preceded by a negative half-height cosine valley.  The intervals of different i do not overlap, so
    every grid point is classified once instead of sweeping the grid per harmonic."""
    freqList = np.asarray(freqList, np.float64)
    in_use = min(int(freqList[-1] / f), len(_HARMONICS))
    used = np.zeros(_HARMONICS[-1] + 2, bool)
    used[_HARMONICS[:in_use]] = True

    ratio = freqList / f
    # the multiple whose interval (-0.85, 0.15) can contain this point, and the distance from it
    mult = np.clip(np.ceil(ratio - _PEAK_WIDTH), 0, _HARMONICS[-1] + 1).astype(int)
    k = np.zeros_like(freqList)
    for cand in (mult, mult + 1):            # ceil() sits on the boundary for points exactly 0.15 above a multiple
        cand = np.minimum(cand, _HARMONICS[-1] + 1)
        a = ratio - cand
        live = (cand >= 1) & (cand <= _HARMONICS[-1])
        sel = used[cand]
        in_peak = live & (np.abs(a) < _PEAK_WIDTH)
        in_valley = live & (-_VALLEY_WIDTH < a) & (a < np.where(sel, -_PEAK_WIDTH, _PEAK_WIDTH)) & ~in_peak
        k[in_valley] = -np.cos((a[in_valley] + 0.5) / ((_VALLEY_WIDTH - _PEAK_WIDTH) / 2) * (np.pi / 2)) / 2
        k[in_peak] = np.cos(a[in_peak] / _PEAK_WIDTH * (np.pi / 2)) / np.where(sel[in_peak], 1, 4)

    knee = f * (2 + _PEAK_WIDTH)             # flat up to harmonic 2.15, then 1/sqrt(freq)
    k *= np.where(freqList <= knee, np.sqrt(1.0 / knee), np.sqrt(1.0 / freqList)) / np.sqrt(1.0 / knee)
    k /= np.sum(k[k > 0])
    k /= in_use / len(_HARMONICS)
    return k


def swipe_tables(sample_rate=SAMPLING_RATE, min_freq=DEFAULT_MIN_FREQ, max_freq=DEFAULT_MAX_FREQ, cres=DEFAULT_C_RES):
    """(log-spaced grid up to Nyquist, candidates = grid below max_freq, kernel matrix) — _init_swipe, :334-355."""
    count = int(np.log2(sample_rate / (2 * min_freq)) * (1200 / cres))
    grid = np.logspace(np.log2(min_freq), np.log2(sample_rate // 2), num=count, base=2)
    candidates = grid[:np.searchsorted(grid, max_freq)]
    kernels = np.zeros((len(candidates), len(grid)))
    for row, f in enumerate(candidates):
        kernels[row] = calcCosineKernel(f, grid)
    return grid, candidates, kernels


class PitchEngine:
    """Batch driver of frt_pitch_*: every complete frame of x[C][T] -> one estimate (NaN = unvoiced)."""

    def __init__(self, fft_size=DEFAULT_FFT_SIZE, hop=None, n_channels=1, sample_rate=SAMPLING_RATE, grid=None, kernels=None,
                 min_db=DEFAULT_MIN_DB, conf=DEFAULT_P_CONF, p_delta=DEFAULT_P_DELTA):
        self._lib = _lib.init()
        if grid is None or kernels is None:
            grid, _, kernels = swipe_tables(sample_rate)
        self.fft_size, self.hop = int(fft_size), int(hop if hop is not None else fft_size // 4)
        self.n_channels = int(n_channels)
        self.grid = np.ascontiguousarray(grid, np.float64)
        kernels = np.ascontiguousarray(kernels, np.float64)
        if kernels.ndim != 2 or kernels.shape[1] != self.grid.size:
            raise ValueError("kernels must be [candidates, len(grid)]")
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.frt_pitch_create(ctypes.byref(self._h), self.fft_size, self.hop, self.n_channels, float(sample_rate),
                                              self.grid.ctypes.data, self.grid.size, kernels.ctypes.data, kernels.shape[0],
                                              float(min_db), float(conf), float(p_delta)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.frt_pitch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def frames_for(self, n_samples: int) -> int:
        return int(self._lib.frt_pitch_frames_for(self._h, int(n_samples)))

    def reset(self):
        _lib.check(self._lib.frt_pitch_reset(self._h))

    def set_scratch_limit(self, n_bytes: int):
        _lib.check(self._lib.frt_pitch_set_scratch_limit(self._h, int(n_bytes)))

    def set_gate(self, min_db, conf, p_delta):
        _lib.check(self._lib.frt_pitch_set_gate(self._h, float(min_db), float(conf), float(p_delta)))

    @property
    def previous(self):
        p = np.empty(self.n_channels, np.float64)
        _lib.check(self._lib.frt_pitch_get_previous(self._h, p.ctypes.data))
        return p

    @previous.setter
    def previous(self, values):
        p = np.ascontiguousarray(np.broadcast_to(np.asarray(values, np.float64), (self.n_channels,)))
        _lib.check(self._lib.frt_pitch_set_previous(self._h, p.ctypes.data))

    def track(self, x, with_raw: bool = False):
        """x: [C, T] float64 (numpy, or a torch CUDA tensor: the result stays in HBM).
        Returns f0 [C, F]; with_raw adds [3, C, F] = (estimate before gating, confidence, dBFS)."""
        if type(x).__module__.startswith("torch"):
            import torch
            if not (x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()):
                raise ValueError("expected a contiguous float64 CUDA tensor")
            if x.dim() == 1:
                x = x[None, :]
            if x.shape[0] != self.n_channels:
                raise ValueError(f"expected {self.n_channels} channels, got {x.shape[0]}")
            F = self.frames_for(x.shape[1])
            f0 = torch.empty((self.n_channels, F), dtype=torch.float64, device=x.device)
            raw = torch.empty((3, self.n_channels, F), dtype=torch.float64, device=x.device) if with_raw else None
            _lib.check(self._lib.frt_pitch_set_stream(self._h, ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
            if F:
                _lib.check(self._lib.frt_pitch_track(self._h, ctypes.c_void_p(x.data_ptr()), x.shape[1], x.stride(0),
                                                     ctypes.c_void_p(f0.data_ptr()),
                                                     ctypes.c_void_p(raw.data_ptr()) if with_raw else None, None))
            return (f0, raw) if with_raw else f0
        x = np.ascontiguousarray(x, np.float64)
        if x.ndim == 1:
            x = x[None, :]
        if x.shape[0] != self.n_channels:
            raise ValueError(f"expected {self.n_channels} channels, got {x.shape[0]}")
        F = self.frames_for(x.shape[1])
        f0 = np.empty((self.n_channels, F), np.float64)
        raw = np.empty((3, self.n_channels, F), np.float64) if with_raw else None
        if F:
            _lib.check(self._lib.frt_pitch_track(self._h, x.ctypes.data, x.shape[1], x.shape[1], f0.ctypes.data,
                                                 raw.ctypes.data if with_raw else None, None))
        return (f0, raw) if with_raw else f0


class PitchTracker:
    """Streaming tracker over a ring buffer, with the reference's interface (pitch_tracker.py:266-428)."""

    def __init__(self, input_buf: RingBuffer, fft_size: int = DEFAULT_FFT_SIZE, overlap: float = 0.75,
                 sample_rate: int = SAMPLING_RATE, min_freq: float = DEFAULT_MIN_FREQ, max_freq: float = DEFAULT_MAX_FREQ,
                 min_db: float = DEFAULT_MIN_DB, cres: int = DEFAULT_C_RES, conf: float = DEFAULT_P_CONF,
                 p_delta: int = DEFAULT_P_DELTA):
        self.fft_size = fft_size
        self.overlap = overlap
        self.sample_rate = sample_rate
        self.min_freq = min_freq
        self.max_freq = max_freq
        self.min_db = min_db
        self.cres = cres
        self.conf = conf
        self.p_delta = p_delta
        self.prev_f0 = None

        self.input_buf = input_buf
        self.input_buf.grow_if_needed(fft_size)
        self.next_in_offset = self.input_buf.offset

        self.out_buf = RingBuffer()
        self.out_offset = self.out_buf.offset

        self.proc = audioproc()
        self.proc.set_fftsize(self.fft_size)
        self._engine = None
        self._init_swipe()

    def set_input_buffer(self, new_buf: RingBuffer) -> None:
        self.input_buf = new_buf
        self.input_buf.grow_if_needed(self.fft_size)
        self.next_in_offset = self.input_buf.offset

    def _init_swipe(self):
        self.logSpacedFreqs, self.pitchCandidates, self.kernels = swipe_tables(self.sample_rate, self.min_freq, self.max_freq,
                                                                               self.cres)
        self._engine = None                   # tables changed: the device plan is rebuilt at the next estimate

    def _step(self) -> int:
        return math.floor(self.fft_size * (1.0 - self.overlap))

    def _plan(self) -> PitchEngine:
        if self._engine is None:
            self._engine = PitchEngine(self.fft_size, max(1, self._step()), 1, self.sample_rate, self.logSpacedFreqs, self.kernels,
                                       self.min_db, self.conf, self.p_delta)
        # thresholds and the previous estimate are plain attributes upstream (the widget writes them, :142-146)
        self._engine.set_gate(self.min_db, self.conf, self.p_delta)
        self._engine.previous = np.nan if self.prev_f0 is None else self.prev_f0
        return self._engine

    def _run(self, samples):
        """All complete frames of one contiguous float64 run ([T] or [rows, T]) -> estimates; keeps prev_f0 in step.
        The spectrum is row 0's; the level of the gate is the RMS over EVERY row of the frame (pitch_tracker.py:404-407:
        `np.sqrt(np.mean(frame**2))` on the 2-D frame, two rows when the shared ring buffer is in dual-channel mode)."""
        samples = np.asarray(samples, np.float64)
        if samples.ndim == 1 or samples.shape[0] == 1:
            est = self._plan().track(np.ascontiguousarray(samples.reshape(-1)))[0]
        else:
            # dual-channel frames: estimate, confidence on the device from row 0; the gate (one comparison chain per frame,
            # sequential in prev_f0) on the host with the all-rows level
            eng = self._plan()
            _, raw = eng.track(np.ascontiguousarray(samples[0]), with_raw=True)
            f0_raw, conf = raw[0, 0], raw[1, 0]
            step, n = max(1, self._step()), self.fft_size
            csum = np.concatenate([[0.0], np.cumsum(np.sum(samples * samples, axis=0))])
            est = np.empty_like(f0_raw)
            prev = self.prev_f0
            for f in range(f0_raw.size):
                rms = np.sqrt((csum[f * step + n] - csum[f * step]) / (samples.shape[0] * n))
                dbfs = 20 * np.log10(rms + np.finfo(np.float64).eps)
                f0 = f0_raw[f]
                jump = 12 * np.abs(np.log2(f0 / prev)) if prev is not None else 0
                if (dbfs < self.min_db) or (conf[f] < self.conf) or (jump > self.p_delta) or np.isnan(f0):
                    prev, est[f] = None, np.nan
                else:
                    prev, est[f] = float(f0), f0
        if est.size:
            self.prev_f0 = None if np.isnan(est[-1]) else float(est[-1])
        return est

    def estimate_pitch(self, frame: np.ndarray):
        """frame: [rows, fft_size]: spectrum from row 0, level from every row.  Hz, or nan if unvoiced."""
        frame = np.asarray(frame, np.float64)
        if frame.shape[-1] != self.fft_size:
            raise ValueError(f"estimate_pitch expects {self.fft_size} samples, got {frame.shape[-1]}")
        return float(self._run(frame)[0])

    def new_frames(self):
        assert self.input_buf.offset >= self.next_in_offset
        while self.next_in_offset + self.fft_size <= self.input_buf.offset:
            yield self.input_buf.data_indexed(self.next_in_offset + self.fft_size, self.fft_size)
            self.next_in_offset += self._step()

    def update(self) -> bool:
        """Estimates for every frame completed since the last call, as ONE batch: consecutive frames are
        a contiguous run of the ring (the reference estimates them one by one, :313-317)."""
        assert self.input_buf.offset >= self.next_in_offset
        step = self._step()
        avail = self.input_buf.offset - self.next_in_offset
        count = 0 if avail < self.fft_size else (avail - self.fft_size) // step + 1 if step > 0 else 0
        new = []
        if count:
            span = self.fft_size + (count - 1) * step
            run = self.input_buf.data_indexed(self.next_in_offset + span, span)
            new = list(self._run(np.ascontiguousarray(run)))
            self.next_in_offset += count * step
        self.out_buf.push(np.array([new]), 0)
        self.out_offset = self.out_buf.offset
        return len(new) != 0

    def get_estimates(self, time_s: float) -> np.ndarray:
        num_results = math.floor(time_s / (self._step() / self.sample_rate)) + 1
        return self.out_buf.data_indexed(self.out_offset, num_results)[0, :]

    def get_latest_estimate(self) -> float:
        return self.out_buf.data_indexed(self.out_offset, 1)[0, 0]


# ---- the widget's chain over whole recordings -----------------------------------------------------------------------------

def pitch_schedule(n_samples, fft_size, step, chunk=512, ends=None, pending=0):
    """(frame_start [R + 1], refresh_chunk [R]) of a stream of n_samples seen chunk by chunk by the pitch widget (update /
    new_frames, pitch_tracker.py:313-332; handle_new_data, :109-112).  Frame g is the fft_size samples from g * step on, counted
    from the first of the `pending` samples received and not consumed before this stream; it completes in the first chunk whose
    end e has pending + e >= g * step + fft_size, and a chunk refreshes iff it completes at least one frame.  `ends`: the
    chunks' end indices, for ragged chunks; default: the ends of `chunk`-sample chunks, a short last chunk is a short chunk."""
    have = checked_ends(n_samples, chunk, ends) + int(pending)
    done = np.where(have >= fft_size, (have - fft_size) // step + 1, 0)          # frames complete after each chunk
    fresh = np.diff(done, prepend=0) > 0
    return np.concatenate([[0], done[fresh]]).astype(np.int64), np.flatnonzero(fresh).astype(np.int64)


class PitchState(NamedTuple):
    """What a pitch widget carries between two calls."""
    tail: object            # [S, rows, pending] float64 (float32 input widened exactly): the samples from the next frame's first on
    pending: int            # received and not consumed (below fft_size)
    previous: object        # [S] float64: the gate's previous estimate, NaN = none
    history: object         # [S, M] float64: the last M estimates (NaN = unvoiced), zeros before the first


class PitchResult(NamedTuple):
    estimates: object       # [S, F] float64, NaN = unvoiced; [F] for one stream given without its axis (likewise below)
    raw: object             # [3, S, F] float64 (estimate before the gate, confidence, dBFS) with with_raw, else None
    frame_start: object     # [R + 1] int64 (host): refresh r completes the frames frame_start[r] .. frame_start[r + 1] - 1
    refresh_chunk: object   # [R] int64 (host): the chunk that caused each refresh
    pitch: object           # [S, R] float64: the latest estimate at each refresh
    curve: object           # [S, M] (keep="last": the curve after the last refresh) or [S, R, M] (keep="all"), within [0, 1]
    times: object           # [M] float64 (host): linspace(0, 1, M)
    state: PitchState


class PitchBatch:
    """S streams of a whole recording through the pitch tracker widget's chain in device calls, as widgets fed chunk by chunk
    would have seen it: the kernels of PitchEngine on row 0 of every frame, the gate's level as the RMS over every row of the
    frame (one row, or two with dual_channels: pitch_tracker.py:370, 404-407), the gate, and per refresh the latest estimate
    and the curve of update_curve (:114-119: the last M = floor(duration / (step / sample_rate)) + 1 estimates on the OctaveC
    axis between min_freq and max_freq, flipped and clipped; unvoiced estimates and the zeros before the first frame sit at 1).
    Fixed settings, no pause.

    run(x, chunk=512 | ends=..., state=None, keep="last" | "all", with_raw=False) takes [S, T] ([S, 2, T] with dual_channels;
    the stream axis may be left out for one stream), float32 or float64, numpy array or CUDA tensor.  Results are numpy for numpy
    input and CUDA tensors for CUDA input.  Spectra, grid spectra and strengths of the frames live in at most `scratch_bytes` of
    device memory: longer recordings go through in slabs of frames, with the same bits whatever the slab size; the number of
    launches and copies of a run depends on the number of slabs only, not on frames or refreshes.

    The chain is defined on the true samples: what the reference shows as long as chunk + fft_size stays within the 10000
    samples of its ring (ringbuffer.py:34), beyond which its frames read samples the ring has already overwritten.  For one
    row, `estimates` equals PitchEngine.track on the same float64 samples, bit for bit, where track's rows start on 16-byte
    boundaries (an even number of samples per row): the transform has another instance for rows that do not, which from fft_size
    2048 on rounds differently (4e-16 relative in the estimates), and PitchBatch always uses the aligned one, so that a
    recording cut at any sample gives the bits of the recording fed whole."""

    def __init__(self, fft_size: int = DEFAULT_FFT_SIZE, overlap: float = 0.75, sample_rate: int = SAMPLING_RATE,
                 min_freq: float = DEFAULT_MIN_FREQ, max_freq: float = DEFAULT_MAX_FREQ, min_db: float = DEFAULT_MIN_DB,
                 cres: int = DEFAULT_C_RES, conf: float = DEFAULT_P_CONF, p_delta: int = DEFAULT_P_DELTA,
                 duration: float = DEFAULT_DURATION, dual_channels: bool = False):
        self.fft_size = int(fft_size)
        self.overlap = overlap
        self.sample_rate = sample_rate
        self.min_freq, self.max_freq = min_freq, max_freq
        self.min_db, self.cres, self.conf, self.p_delta = min_db, cres, conf, p_delta
        self.duration = duration
        self.dual_channels = bool(dual_channels)
        self.rows = 2 if self.dual_channels else 1
        self.step = math.floor(self.fft_size * (1.0 - overlap))
        if self.step < 1:
            raise ValueError(f"fft_size {fft_size} with overlap {overlap}: no frame advance")
        if not 0 < min_freq < max_freq:
            raise ValueError(f"axis range [{min_freq}, {max_freq}]")
        self.n_history = math.floor(duration / (self.step / sample_rate)) + 1          # get_estimates, :325-327
        if self.n_history < 1:
            raise ValueError(f"duration {duration}")
        self.times = np.linspace(0, 1.0, self.n_history)
        self.grid, self.candidates, self.kernels = swipe_tables(sample_rate, min_freq, max_freq, cres)
        self._engines = {}

    # ---- host only ------------------------------------------------------------------------------------------------------------
    def schedule(self, n_samples, chunk=512, ends=None, state=None):
        """pitch_schedule for this widget's frame size and step, from a carried state's pending samples on."""
        return pitch_schedule(n_samples, self.fft_size, self.step, chunk, ends, 0 if state is None else state.pending)

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def _check_input(self, x, state):
        x, is_np, squeeze, pending = check_samples("PitchBatch", x, state, self.dual_channels)
        S, M = x.shape[0], self.n_history
        if state is not None:
            want = {"tail": (S, self.rows, pending), "previous": (S,), "history": (S, M)}
            got = {name: tuple(getattr(state, name).shape) for name in want}
            if not 0 <= pending < self.fft_size or got != want:
                raise ValueError(f"state of another shape: {got} (want {want}), pending {pending} (below {self.fft_size})")
        return x.reshape(S, self.rows, x.shape[-1]), is_np, squeeze, pending

    def _engine(self, streams):
        if streams not in self._engines:
            self._engines[streams] = PitchEngine(self.fft_size, self.step, streams, self.sample_rate, self.grid, self.kernels,
                                                 self.min_db, self.conf, self.p_delta)
        return self._engines[streams]

    def run(self, x, chunk=512, ends=None, state=None, keep="last", with_raw=False, scratch_bytes=1 << 30):
        check_keep(keep, "all", "last")
        x, is_np, squeeze, pending = self._check_input(x, state)
        frame_start, refresh_chunk = self.schedule(x.shape[-1], chunk, ends, state)
        if ends is not None:                                         # the widgets were pushed ends[-1] samples
            x = x[..., :int(np.asarray(ends).reshape(-1)[-1]) if np.size(ends) else 0]
        import torch
        lib = _lib.init()
        S, rows, T, M = x.shape[0], self.rows, x.shape[-1], self.n_history
        F, R, L = int(frame_start[-1]), len(refresh_chunk), pending + x.shape[-1]
        f64, vp = torch.float64, ctypes.c_void_p
        tail, previous, history = (None, None, None) if state is None else (state.tail, state.previous, state.history)
        with null_stream(x, is_np) as dev:
            xd, x_ptr, code, strides = source(torch.from_numpy(np.ascontiguousarray(x)).to(dev) if is_np else x, True)
            tail = carried(dev, tail, (S, rows, pending))
            eng = self._engine(S)
            est = torch.empty((S, F), dtype=f64, device=dev)
            raw = torch.empty((3, S, F), dtype=f64, device=dev) if with_raw else None
            previous = carried(dev, previous, (S,), math.nan)
            if F:
                # The transform picks its instance by the alignment of its rows (16-byte row starts: an even stride from an
                # aligned address), and the instances round differently from fft_size 2048 on.  Row 0 is therefore always handed
                # over aligned, whatever the length of this piece, so that a recording in pieces gives the bits of the whole.
                even = L + (L & 1)
                if pending == 0 and code == 1 and x_ptr % 16 == 0 and (S == 1 or strides[0] % 2 == 0):
                    row0, row0_stride = xd[:, 0, :], strides[0] if S > 1 else even          # row 0 as it lies
                else:
                    row0, row0_stride = torch.empty((S, even), dtype=f64, device=dev), even
                    row0[:, :pending] = tail[:, 0, :]
                    row0[:, pending:L] = xd[:, 0, :]
                    row0[:, L:] = 0.0                                # the pad: never part of a frame
                eng.set_scratch_limit(scratch_bytes)
                _lib.check(lib.frt_pitch_set_stream(eng._h, None))
                _lib.check(lib.frt_pitch_set_previous(eng._h, vp(previous.data_ptr())))
                _lib.check(lib.frt_pitch_track_rows(eng._h, vp(row0.data_ptr()), row0_stride, vp(x_ptr), code, rows, T, strides[0],
                                                    strides[1], vp(tail.data_ptr()) if pending else None, pending,
                                                    vp(est.data_ptr()), vp(raw.data_ptr()) if with_raw else None, None))
                _lib.check(lib.frt_pitch_get_previous(eng._h, vp(previous.data_ptr())))
            history_in = carried(dev, history, (S, M))
            history = torch.empty((S, M), dtype=f64, device=dev)
            pitch = torch.empty((S, R), dtype=f64, device=dev)
            curve = torch.empty((S, 1 if keep == "last" else R, M), dtype=f64, device=dev)
            if R or keep == "last":
                _lib.check(lib.frt_pitch_refresh(vp(est.data_ptr()) if F else None, S, F,
                                                 frame_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), R,
                                                 vp(history_in.data_ptr()), M, float(self.min_freq), float(self.max_freq),
                                                 int(keep == "last"), vp(history.data_ptr()), vp(pitch.data_ptr()),
                                                 vp(curve.data_ptr())))
            if not R:
                history = history_in
            if keep == "last":
                curve = curve[:, 0]
            # behind the last frame: samples F * step .. L of tail || x, widened
            used = F * self.step
            new_tail = torch.cat([tail[:, :, min(used, pending):], xd[:, :, max(used - pending, 0):].to(f64)], dim=2)
            new_state = PitchState(new_tail, L - used, previous, history)
            if is_np:
                est, raw, pitch, curve, new_state = to_host((est, raw, pitch, curve, new_state))
        if squeeze:
            est, pitch, curve = est[0], pitch[0], curve[0]
            raw = raw[:, 0] if with_raw else None
        return PitchResult(est, raw, frame_start, refresh_chunk, pitch, curve, self.times, new_state)


# ---- the live chain on the device -----------------------------------------------------------------------------------------

class PitchTrackerStream(PitchTracker):
    """PitchTracker with its chain resident on the device (csrc/pitchstream.hip, frt_pitch_live_*): the reference's interface —
    the shared host RingBuffer, set_input_buffer, update, get_estimates, get_latest_estimate, estimate_pitch, and min_db / conf /
    p_delta as plain attributes read at every update — with the gate's previous estimate, the estimate history and the curve
    kept in HBM.  An update() that completes frames is ONE device call: the span of the ring that completes them goes up (one
    row, or two when the ring is in dual-channel mode: the gate's level is the RMS over both), the new estimates, the latest
    estimate and the curve of update_curve come back, behind one synchronisation; an update() that completes none makes no
    device call.  The estimates still go into out_buf; `pitch`, `curve` and `times` are what handle_new_data / update_curve
    (:109-119) leave in the view model, as of the last refresh.  duration, min_freq and max_freq are fixed at construction, as
    in PitchBatch.  The device objects are created at the first completed frame: construction and updates before it need no GPU.

    Estimates, `pitch` and `curve` equal PitchBatch.run on the same samples and chunk ends bit for bit, and get_state() /
    set_state() exchange a PitchState of one stream with it: a recording can be started in PitchBatch and continued live, or
    the other way round."""

    def __init__(self, input_buf: RingBuffer, fft_size: int = DEFAULT_FFT_SIZE, overlap: float = 0.75,
                 sample_rate: int = SAMPLING_RATE, min_freq: float = DEFAULT_MIN_FREQ, max_freq: float = DEFAULT_MAX_FREQ,
                 min_db: float = DEFAULT_MIN_DB, cres: int = DEFAULT_C_RES, conf: float = DEFAULT_P_CONF,
                 p_delta: int = DEFAULT_P_DELTA, duration: float = DEFAULT_DURATION):
        # PitchTracker.__init__ without its audioproc, which is a device object: nothing here touches the GPU
        self.fft_size = int(fft_size)
        self.overlap = overlap
        self.sample_rate = sample_rate
        self.min_freq, self.max_freq = min_freq, max_freq
        self.min_db, self.cres, self.conf, self.p_delta = min_db, cres, conf, p_delta
        self.duration = duration
        self.step = self._step()
        if self.step < 1:
            raise ValueError(f"fft_size {fft_size} with overlap {overlap}: no frame advance")
        if not 0 < min_freq < max_freq:
            raise ValueError(f"axis range [{min_freq}, {max_freq}]")
        self.n_history = math.floor(duration / (self.step / sample_rate)) + 1          # get_estimates, :325-327
        if self.n_history < 1:
            raise ValueError(f"duration {duration}")
        self.times = np.linspace(0, 1.0, self.n_history)
        self.curve = np.ones(self.n_history)                 # the ring's zeros on the axis
        self.pitch = math.nan                                # no refresh yet

        self.input_buf = input_buf
        self.input_buf.grow_if_needed(self.fft_size)
        self.next_in_offset = self.input_buf.offset
        self.out_buf = RingBuffer()
        self.out_offset = self.out_buf.offset

        self._engine, self._live = None, None
        self._carry = None                                   # [rows, n] float64 handed over by set_state, ahead of the ring's samples
        self._previous = np.full(1, np.nan)                  # the state while there is no device object
        self._history = np.zeros(self.n_history)
        self._init_swipe()

    # ---- host only ------------------------------------------------------------------------------------------------------------
    def set_input_buffer(self, new_buf: RingBuffer) -> None:
        super().set_input_buffer(new_buf)
        self._carry = None

    def _init_swipe(self):
        if getattr(self, "_live", None) is not None:         # new tables: the plan is rebuilt, the state stays
            self._previous, self._history = self._device_state()
        self.close()
        super()._init_swipe()

    def pending(self) -> int:
        """Samples received that no frame has consumed."""
        carried_over = 0 if self._carry is None else self._carry.shape[1]
        return carried_over + self.input_buf.offset - self.next_in_offset

    def plan_update(self):
        """(frames, span) of the next update(): the frames the pending samples complete and the samples that hold them."""
        avail = self.pending()
        count = 0 if avail < self.fft_size else (avail - self.fft_size) // self.step + 1
        return count, self.fft_size + (count - 1) * self.step if count else 0

    def _take(self, count, span):
        """The span that completes `count` frames, [rows, span]; the stream advances by count steps."""
        used = count * self.step
        if self._carry is None:
            run = self.input_buf.data_indexed(self.next_in_offset + span, span)
            self.next_in_offset += used
            return run
        carried_over = self._carry.shape[1]
        rest = self.input_buf.data_indexed(self.next_in_offset + span - carried_over, span - carried_over)
        if rest.shape[0] != self._carry.shape[0]:
            raise ValueError(f"a state of {self._carry.shape[0]} rows ahead of a ring of {rest.shape[0]}")
        run = np.concatenate([self._carry, rest], axis=1)
        if used >= carried_over:
            self.next_in_offset += used - carried_over
            self._carry = None
        else:
            self._carry = self._carry[:, used:]
        return run

    def update(self) -> bool:
        assert self.input_buf.offset >= self.next_in_offset
        count, span = self.plan_update()
        new = []
        if count:
            new = list(self._push(self._take(count, span)))
        self.out_buf.push(np.array([new]), 0)
        self.out_offset = self.out_buf.offset
        return len(new) != 0

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_live", None) is not None:
            _lib.load().frt_pitch_live_destroy(self._live)
        self._live = None
        if getattr(self, "_engine", None) is not None:
            self._engine.close()
        self._engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _device(self):
        if self._live is None:
            lib = _lib.init()
            self._engine = PitchEngine(self.fft_size, self.step, 1, self.sample_rate, self.logSpacedFreqs, self.kernels,
                                       self.min_db, self.conf, self.p_delta)
            live = ctypes.c_void_p()
            _lib.check(lib.frt_pitch_live_create(ctypes.byref(live), self._engine._h, self.n_history, float(self.min_freq),
                                                 float(self.max_freq)))
            self._live = live
            _lib.check(lib.frt_pitch_live_set_state(live, self._previous.ctypes.data, self._history.ctypes.data))
        return self._live

    @property
    def crossover(self) -> int:
        """Frames per update up to which the few-frames product kernel runs; above it the tiled kernel of PitchEngine."""
        return int(_lib.load().frt_pitch_live_crossover(self._live))

    @crossover.setter
    def crossover(self, frames):
        _lib.check(_lib.load().frt_pitch_live_set_crossover(self._device(), int(frames)))

    def _push(self, samples):
        """[rows, fft_size + (F - 1) * step] host samples -> the F gated estimates; leaves pitch and curve."""
        x = np.asarray(samples)
        if x.ndim == 1:
            x = x[None, :]
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float64)
        if x.ndim != 2 or x.shape[0] not in (1, 2):
            raise ValueError(f"samples of shape {x.shape}: one stream is [rows, n] with one row, or two for dual channels")
        if x.strides[1] != x.itemsize or x.strides[0] % x.itemsize or (x.shape[0] == 2 and x.strides[0] < x.shape[1] * x.itemsize):
            x = np.ascontiguousarray(x)
        span = x.shape[1]
        if span < self.fft_size or (span - self.fft_size) % self.step:
            raise ValueError(f"{span} samples complete no whole number of frames of {self.fft_size} every {self.step}")
        frames = (span - self.fft_size) // self.step + 1
        est, curve, latest = np.empty(frames), np.empty(self.n_history), ctypes.c_double()
        _lib.check(_lib.load().frt_pitch_live_push(self._device(), x.ctypes.data, int(x.dtype == np.float64), x.shape[0], span,
                                                   x.strides[0] // x.itemsize, float(self.min_db), float(self.conf),
                                                   float(self.p_delta), est.ctypes.data, ctypes.byref(latest), curve.ctypes.data,
                                                   None))
        self.pitch, self.curve = latest.value, curve
        return est

    def estimate_pitch(self, frame: np.ndarray):
        """frame: [rows, fft_size]: spectrum from row 0, level from every row.  Hz, or nan if unvoiced.  As upstream, the gate's
        previous estimate moves on; history, pitch and curve belong to update() and stay."""
        frame = np.asarray(frame)
        if frame.shape[-1] != self.fft_size:
            raise ValueError(f"estimate_pitch expects {self.fft_size} samples, got {frame.shape[-1]}")
        self._device()
        (_, history), shown = self._device_state(), (self.pitch, self.curve)
        est = float(self._push(frame)[0])
        self._set_device_state(np.full(1, est), history)
        self.pitch, self.curve = shown
        return est

    def _device_state(self):
        previous, history = np.empty(1), np.empty(self.n_history)
        _lib.check(_lib.load().frt_pitch_live_get_state(self._live, previous.ctypes.data, history.ctypes.data))
        return previous, history

    def _set_device_state(self, previous, history):
        _lib.check(_lib.load().frt_pitch_live_set_state(self._live, previous.ctypes.data, history.ctypes.data))

    @property
    def prev_f0(self):
        previous = self._previous if self._live is None else self._device_state()[0]
        return None if np.isnan(previous[0]) else float(previous[0])

    @prev_f0.setter
    def prev_f0(self, value):
        previous = np.full(1, np.nan if value is None else float(value))
        if self._live is None:
            self._previous = previous
        else:
            self._set_device_state(previous, self._device_state()[1])

    def get_state(self) -> PitchState:
        """The PitchState of this one stream (numpy): PitchBatch.run(rest, state=...) continues where the stream stands."""
        previous, history = (self._previous.copy(), self._history.copy()) if self._live is None else self._device_state()
        in_ring = self.input_buf.offset - self.next_in_offset
        tail = np.array(self.input_buf.data_indexed(self.input_buf.offset, in_ring), np.float64)
        if self._carry is not None:
            if in_ring and tail.shape[0] != self._carry.shape[0]:
                raise ValueError(f"a state of {self._carry.shape[0]} rows ahead of a ring of {tail.shape[0]}")
            tail = np.concatenate([self._carry, tail], axis=1) if in_ring else self._carry.copy()
        return PitchState(tail[None], tail.shape[1], previous, history[None])

    def set_state(self, state: PitchState) -> None:
        """Continue from a PitchState of one stream (PitchBatch's, or another stream's): its tail stands ahead of whatever the
        ring receives from now on; what the ring holds at this moment is not part of the stream."""
        tail, previous, history = (np.asarray(to_host(v), np.float64) for v in (state.tail, state.previous, state.history))
        pending = int(state.pending)
        want = {"tail": (1, tail.shape[1] if tail.ndim == 3 else 0, pending), "previous": (1,), "history": (1, self.n_history)}
        got = {"tail": tail.shape, "previous": previous.shape, "history": history.shape}
        if not 0 <= pending < self.fft_size or got != want or tail.shape[1] not in (1, 2):
            raise ValueError(f"state of another shape: {got} (want {want}, one or two rows), pending {pending} (below {self.fft_size})")
        self._carry = tail[0].copy() if pending else None
        self.next_in_offset = self.input_buf.offset
        self._previous, self._history = previous.copy(), np.ascontiguousarray(history[0])
        if self._live is not None:
            self._set_device_state(self._previous, self._history)
