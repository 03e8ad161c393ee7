"""The delay estimator's processing chain (friture/delay_estimator.py:87-176) without its Qt shell.

`DelayEstimator.handle_new_data(floatdata)` does what the widget's slot does for a two-channel
chunk: two chained IIR decimations per channel with carried state (kernel K2 via
friture_amd.signal.decimate), private ring buffers of the 12 kHz signals, 50 %-overlapped windows of
2 * delayrange * 12000 samples, GCC-PHAT per window (kernel K5), exponential smoothing of the
correlation, peak pick and the delay / polarity / confidence read-out (frt_gcc_readout).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import filter_design
from ._batchio import carried, check_keep, check_samples, checked_ends, null_stream, to_host
from .constants import SAMPLING_RATE
from .ringbuffer import RingBuffer
from .signal.correlation import GccPhat, generalized_cross_correlation
from .signal.decimate import decimate_multiple, decimate_multiple_channels, decimate_multiple_filtic

DEFAULT_DELAYRANGE = 1      # default delay range is 1 second (delay_estimator.py:31)


class DelayEstimator:
    def __init__(self, delayrange_s: float = DEFAULT_DELAYRANGE):
        t = filter_design.load_tables()
        self.Ndec = 2
        self.subsampled_sampling_rate = SAMPLING_RATE / 2 ** self.Ndec
        self.bdec, self.adec = np.array(t["bdec"]), np.array(t["adec"])
        self.zfs0 = decimate_multiple_filtic(self.Ndec, self.bdec, self.adec)
        self.zfs1 = decimate_multiple_filtic(self.Ndec, self.bdec, self.adec)
        self.ringbuffer0, self.ringbuffer1 = RingBuffer(), RingBuffer()
        self.delayrange_s = delayrange_s
        self.old_Xcorr = None
        self.old_index = 0
        self.two_channels = False
        self.delay_ms = 0.
        self.distance_m = 0.
        self.correlation = 0.
        self.Xcorr_extremum = 0.
        self._gcc = None

    def set_delayrange(self, delay_s):
        self.delayrange_s = delay_s

    def handle_new_data(self, floatdata):
        if floatdata.shape[0] == 1:
            self.two_channels = False
            return
        self.two_channels = True
        # both channels in one device call (the reference decimates them one after the other, delay_estimator.py:97-98; the
        # channels are independent slots of the same launches: bit for bit the two separate calls)
        xdec, (self.zfs0, self.zfs1) = decimate_multiple_channels(self.Ndec, self.bdec, self.adec, floatdata[0:2, :], [self.zfs0, self.zfs1])
        x0_dec, x1_dec = xdec[0], xdec[1]
        self.ringbuffer0.push(x0_dec.reshape(1, -1), 0)
        self.ringbuffer1.push(x1_dec.reshape(1, -1), 0)

        index = self.ringbuffer0.offset
        available = index - self.old_index
        if available < 0:
            available = 0
            self.old_index = index
        time = 2 * self.delayrange_s
        length = int(time * self.subsampled_sampling_rate)
        needed = int(0.5 * length)
        for _ in range(int(available / needed)):
            self.old_index += needed
            d0 = self.ringbuffer0.data_indexed(self.old_index, length).reshape(-1)     # views into the rings
            d1 = self.ringbuffer1.data_indexed(self.old_index, length).reshape(-1)
            if np.std(d0) > 0. and np.std(d1) > 0.:
                Xcorr = generalized_cross_correlation(d0, d1)                            # de-means the views in place
                if self._gcc is None or self._gcc.length != length:
                    self._gcc = GccPhat(length, 1)
                old = self.old_Xcorr if self.old_Xcorr is not None and self.old_Xcorr.shape == Xcorr.shape else None
                smoothed, ro = self._gcc.readout(Xcorr, old, self.subsampled_sampling_rate, self.delayrange_s, 0.3)
                self.old_Xcorr = smoothed[0]
                self.Xcorr_extremum = ro[0].extremum
                self.delay_ms = ro[0].delay_ms
                self.distance_m = ro[0].distance_m
                self.correlation = ro[0].correlation_pct
            else:
                self.delay_ms = 0.
                self.Xcorr_extremum = 0.
                self.distance_m = 0.
                self.correlation = 0


class DelayEstimatorStream(DelayEstimator):
    """The same chain with its signals resident in HBM, on one C object (frt_delay_*, include/friture_hip.h): per chunk the
    new samples go up through a pinned slot, the two decimation stages (filter states on the device) and one ring-write
    launch are enqueued on the object's stream and the call returns — nothing comes back.  Once per `needed` decimated
    samples a window of both rings (device pointers, same indices / mirror layout / growth as RingBuffer) goes to GCC-PHAT
    and the read-out on the same stream; the in-place mean removal the reference applies to its ring views
    (correlation.py:27-28) is applied to the same samples.  Per window two scalars (the std test of
    delay_estimator.py:127-129) and the read-out come down.  The gate treats a window whose samples are all equal as silent
    (std = 0): numpy's std of a constant non-zero window is 0 or rounding noise depending on the value and the summation
    order, so the reference's own behaviour there is not defined by its arithmetic."""

    def __init__(self, delayrange_s: float = DEFAULT_DELAYRANGE):
        super().__init__(delayrange_s)
        import ctypes

        import torch

        from . import _lib
        self._torch, self._ct, self._libmod = torch, ctypes, _lib
        self._lib = _lib.init()
        # the rings live inside the C object; ringbuffer0 / ringbuffer1 stay inspectable (offset, data_indexed) as on the
        # reference widget (friture/delay_estimator.py:52-53)
        self.ringbuffer0, self.ringbuffer1 = _DeviceRingProxy(self, 0), _DeviceRingProxy(self, 1)
        self._h = ctypes.c_void_p()
        DP = ctypes.POINTER(ctypes.c_double)
        b, a = np.ascontiguousarray(self.bdec, np.float64), np.ascontiguousarray(self.adec, np.float64)
        _lib.check(self._lib.frt_delay_create(ctypes.byref(self._h), b.ctypes.data_as(DP), a.ctypes.data_as(DP), self.Ndec, 10000))
        self._stream = ctypes.c_void_p(self._lib.frt_delay_stream(self._h))
        self._dev = torch.device("cuda", torch.cuda.current_device())
        self._offset = ctypes.c_int64(0)
        self._push = self._lib.frt_delay_push
        self.offset = 0

    def __del__(self):
        try:
            if self._h.value:
                self._lib.frt_delay_destroy(self._h)
        except Exception:
            pass

    def handle_new_data(self, floatdata):
        if floatdata.shape[0] == 1:
            self.two_channels = False
            return
        self.two_channels = True
        x = floatdata[:2]
        if x.dtype != np.float64 or not x.flags.c_contiguous:
            x = np.ascontiguousarray(x, np.float64)
        rc = self._push(self._h, x.ctypes.data, x.shape[1], self._offset)
        if rc:
            self._libmod.check(rc)
        index = self.offset = self._offset.value
        available = index - self.old_index
        if available < 0:
            available = 0
            self.old_index = index
        time = 2 * self.delayrange_s
        length = int(time * self.subsampled_sampling_rate)
        needed = int(0.5 * length)
        if available >= needed:
            self._windows(int(available / needed), length, needed)

    def _windows(self, count, length, needed):
        torch, ct, check, lib = self._torch, self._ct, self._libmod.check, self._lib
        for _ in range(count):
            self.old_index += needed
            p0, p1 = ct.c_void_p(), ct.c_void_p()
            check(lib.frt_delay_window(self._h, self.old_index, length, ct.byref(p0), ct.byref(p1)))
            stds = (ct.c_double * 2)()
            check(lib.frt_delay_window_std(self._h, p0, p1, length, stds))
            if stds[0] > 0. and stds[1] > 0.:
                if self._gcc is None or self._gcc.length != length:
                    self._gcc = GccPhat(length, 1)
                Xcorr = self._gcc.correlate_windows(p0, p1, self._dev, self._stream)
                check(lib.frt_delay_demean(self._h, p0, p1, length, ct.c_void_p(self._gcc.means.data_ptr()), None))
                old = self.old_Xcorr if self.old_Xcorr is not None and self.old_Xcorr.shape == Xcorr.shape else None
                smoothed, ro = self._gcc.readout(Xcorr, old, self.subsampled_sampling_rate, self.delayrange_s, 0.3, stream=self._stream)
                self.old_Xcorr = smoothed
                self.Xcorr_extremum = ro[0].extremum
                self.delay_ms = ro[0].delay_ms
                self.distance_m = ro[0].distance_m
                self.correlation = ro[0].correlation_pct
            else:
                self.delay_ms = 0.
                self.Xcorr_extremum = 0.
                self.distance_m = 0.
                self.correlation = 0

    def window(self, end, length):
        """Host copy [2, length] of the two windows that end at absolute index `end` (tests, inspection)."""
        torch, ct, check = self._torch, self._ct, self._libmod.check
        p0, p1 = ct.c_void_p(), ct.c_void_p()
        check(self._lib.frt_delay_window(self._h, end, length, ct.byref(p0), ct.byref(p1)))
        stds = (ct.c_double * 2)()
        check(self._lib.frt_delay_window_std(self._h, p0, p1, length, stds))                 # waits for the pushes in flight
        return np.stack([torch.as_tensor(_DeviceView(p.value, length), device=self._dev).cpu().numpy() for p in (p0, p1)])


class _DeviceRingProxy:
    """Read-only stand-in for one of DelayEstimatorStream's rings with the two members of friture/ringbuffer.py callers
    inspect: `offset` (absolute index of the next sample) and `data_indexed(start, length)` (the `length` samples that end at
    `start`, as a host array [1, length]; ringbuffer.py:87-99)."""

    def __init__(self, owner, channel):
        self._owner, self._channel = owner, channel

    @property
    def offset(self):
        return self._owner.offset

    def data_indexed(self, start, length):
        if length <= 0:
            raise ArithmeticError("negative or null length")
        return self._owner.window(start, length)[self._channel:self._channel + 1]


class _DeviceView:
    """`length` float64 values at a device address, for torch.as_tensor (CUDA array interface)."""

    def __init__(self, ptr, length):
        self.__cuda_array_interface__ = {"shape": (length,), "typestr": "<f8", "data": (ptr, False), "version": 2}


# ---- the chain over whole recordings -------------------------------------------------------------------------------------------

DELAY_NDEC = 2                  # decimations by 2 in front of the rings (delay_estimator.py:45)
DELAY_RING = 10000              # a fresh RingBuffer's length (ringbuffer.py:30)
DELAY_RUNS = 8                  # runs per window in the table


def delay_lengths(delayrange_s):
    """(length, needed) of the windows at a delay range (delay_estimator.py:113-117)."""
    length = int(2 * delayrange_s * (SAMPLING_RATE / 2 ** DELAY_NDEC))
    return length, int(0.5 * length)


class DelayRing(NamedTuple):
    """A delay estimator's ring as integers: where every position's sample came from, and which window's mean was subtracted there."""
    buffer_length: int
    offset: int                 # decimated samples pushed so far (RingBuffer.offset)
    old_index: int              # the last window's end (delay_estimator.py:104-123)
    n_windows: int              # windows so far: a window's id is its count from the widget's start
    cells: np.ndarray           # [3, 2 * buffer_length] int64: source index + 1 (0: a zero), window id + 1 (0: none), means subtracted
    length: int                 # the windows' length: the delay range cannot change under a state


class DelaySchedule(NamedTuple):
    window_end: np.ndarray      # [W] int64: each window's old_index, counted in decimated samples from the widget's start
    window_start: np.ndarray    # [R + 1] int64: refresh r completed windows window_start[r] .. window_start[r + 1] - 1
    refresh_chunk: np.ndarray   # [R] int64: the chunks after which at least one window completed
    runs: np.ndarray            # [W, 8, 4] int64: (first source index counted from the carried tail, length, 1 = zeros, earlier window)
    ring: DelayRing             # after the last chunk
    length: int
    needed: int
    tail: int                   # decimated samples in front of this call's: length + pending
    n_dec: int                  # decimated samples of this call


class _IndexRing:
    """RingBuffer (friture/ringbuffer.py:28-130) on index cells instead of samples: the same writes, growth and views."""

    def __init__(self, state: DelayRing):
        self.buffer_length, self.offset, self.buffer = int(state.buffer_length), int(state.offset), np.array(state.cells, np.int64)

    def push(self, first, n):
        self.grow_if_needed(n)
        data = np.zeros((3, n), np.int64)
        data[0] = np.arange(first + 1, first + n + 1)
        L = self.buffer_length
        o = self.offset % L
        self.buffer[:, o:o + n] = data
        direct = min(n, L - o)
        self.buffer[:, o + L:o + L + direct] = data[:, :direct]
        self.buffer[:, :n - direct] = data[:, direct:]
        self.offset += n

    def data_indexed(self, start, length):
        self.grow_if_needed(length + self.offset - start)
        stop0 = start % self.buffer_length + self.buffer_length
        start0 = stop0 - length
        if start0 < 0 or start0 > 2 * self.buffer_length:
            raise ArithmeticError("Start index is wrong %d %d" % (start0, self.buffer_length))
        return self.buffer[:, start0:stop0]

    def grow_if_needed(self, length):
        if length <= self.buffer_length:
            return
        old, new = self.buffer_length, int(1.5 * length)
        nb = np.zeros((3, 2 * new), np.int64)
        shift = (self.offset % new - self.offset % old) % new
        nb[:, shift:shift + old] = self.buffer[:, :old]
        direct = min(old, new - shift)
        nb[:, new + shift:new + shift + direct] = self.buffer[:, :direct]
        nb[:, :old - direct] = self.buffer[:, direct:old]
        self.buffer, self.buffer_length = nb, new


def fresh_ring(length):
    return DelayRing(DELAY_RING, 0, 0, 0, np.zeros((3, 2 * DELAY_RING), np.int64), int(length))


def delay_schedule(n_samples, delayrange_s=DEFAULT_DELAYRANGE, chunk=512, ends=None, state=None):
    """The windows of a delay estimator fed n_samples two-channel samples chunk by chunk (`ends`: the chunks' end indices), from
    a carried ring state on (a DelayRing, or a DelayState; None: a fresh widget), planned on indices alone: RingBuffer's push,
    grow_if_needed and data_indexed are replayed on cells that hold, per ring position, where its sample came from and which
    window's in-place mean removal (correlation.py:27-28) it has seen.  Every window then is a few runs of (a range of the
    decimated stream | zeros, the earlier window whose mean was subtracted there | none): row [w, r] of `runs` is (first source
    index, length, 1 for zeros, earlier window: its index in this call, -1 none, -2 the last window before this call).  Source
    indices count from the start of the carried tail, the `length + pending` decimated samples in front of this call's.

    Every chunk holds a multiple of 2 ** Ndec = 4 samples, and at least 4: the reference restarts the [::2] phase of both
    decimations in every chunk, so only then is the decimated stream the same for every chunking.  The chunks cover the
    recording (ends[-1] == n_samples).  More than 8 runs in a window, a position that carries two means when it is read, or one
    whose mean belongs to a window before the state's last are NotImplementedError (none occurs with 50 % overlap)."""
    length, needed = delay_lengths(delayrange_s)
    if length < 4 or length % 2:
        raise ValueError(f"delay range {delayrange_s} s: windows of {length} samples (GCC-PHAT takes even lengths from 4 on)")
    ring = getattr(state, "ring", state)
    if ring is None:
        ring = fresh_ring(length)
    if not isinstance(ring, DelayRing) or np.shape(ring.cells) != (3, 2 * ring.buffer_length) or ring.old_index > ring.offset:
        raise ValueError("state of another shape: not a DelayRing with cells [3, 2 * buffer_length]")
    if ring.length != length:
        raise ValueError(f"the state was made with windows of {ring.length} samples, this delay range has {length}")
    ends = checked_ends(n_samples, chunk, ends)
    sizes = np.diff(ends, prepend=0)
    if ends.size and (np.any(sizes < 4) or np.any(sizes % 4) or ends[-1] != int(n_samples)):
        raise ValueError("every chunk holds a multiple of 4 samples (4 at least) and the chunks cover the recording")
    if not ends.size and int(n_samples):
        raise ValueError("the chunks cover the recording")
    r = _IndexRing(ring)
    offset0, old_index, count0 = r.offset, int(ring.old_index), int(ring.n_windows)
    tail = length + (offset0 - old_index)
    base = offset0 - tail
    window_end, window_start, refresh_chunk, runs = [], [0], [], []
    k = count0
    for c, m in enumerate((sizes // 4).tolist()):
        r.push(r.offset, m)
        available = r.offset - old_index
        done = int(available / needed)
        for _ in range(done):
            old_index += needed
            view = r.data_indexed(old_index, length)
            src, wid, depth = view
            if depth.max() > 1:
                raise NotImplementedError("a ring position carries the means of two windows")
            cont = (wid[1:] == wid[:-1]) & (((src[1:] == src[:-1] + 1) & (src[:-1] > 0)) | ((src[1:] == 0) & (src[:-1] == 0)))
            starts = np.concatenate([[0], np.flatnonzero(~cont) + 1, [length]])
            if len(starts) - 1 > DELAY_RUNS:
                raise NotImplementedError(f"a window of {len(starts) - 1} runs")
            row = np.zeros((DELAY_RUNS, 4), np.int64)
            row[:, 3] = -1
            for j, (a, b) in enumerate(zip(starts[:-1].tolist(), starts[1:].tolist())):
                prior = int(wid[a]) - 1 - count0 if wid[a] else -1
                if wid[a] and prior < -1:
                    raise NotImplementedError("a mean of a window before the state's last one")
                first = int(src[a]) - 1 - base
                if src[a] and first < 0:
                    raise NotImplementedError("a sample older than the carried tail")
                row[j] = (first if src[a] else 0, b - a, int(src[a] == 0), -2 if wid[a] and prior == -1 else prior)
            runs.append(row)
            window_end.append(old_index)
            view[1] = k + 1                       # the view is de-meaned in place (a gated window's mean counts as 0)
            view[2] += 1
            k += 1
        if done:
            window_start.append(window_start[-1] + done)
            refresh_chunk.append(c)
    out = DelayRing(r.buffer_length, r.offset, old_index, k, r.buffer, length)
    return DelaySchedule(np.array(window_end, np.int64), np.array(window_start, np.int64), np.array(refresh_chunk, np.int64),
                         np.array(runs, np.int64).reshape(-1, DELAY_RUNS, 4), out, length, needed, tail, r.offset - offset0)


class DelayState(NamedTuple):
    """What a delay estimator carries between two calls."""
    zi: object                  # [S, 2, Ndec, 12] float64: the decimators' DF2T states, decimate_multiple's order
    samples: object             # [S, 2, 0]: the undecimated remainder (none: every chunk is a multiple of 4 samples)
    tail: object                # [S, 2, length + pending] float64: the last raw decimated samples
    pending: int                # decimated samples behind the last window's end
    ring: DelayRing             # the ring as integers (host)
    means: object               # [S, 2] float64: the last window's means (0 where it was gated)
    gated: object               # [S] int32: the last window's gate
    smoothed: object            # [S, length] float64: the smoothed correlation (old_Xcorr)
    present: object             # [S] int32: 1 where a correlation is carried
    readout: object             # [S, 4] float64: delay_ms, distance_m, extremum, correlation as the widget shows them
    seen: int                   # samples per channel so far: anchors the decimator's cell grid


class DelayResult(NamedTuple):
    window_end: object          # [W] int64 (host)
    window_start: object        # [R + 1] int64 (host)
    refresh_chunk: object       # [R] int64 (host)
    delay_ms: object            # [S, W] float64 per window
    distance_m: object
    extremum: object
    correlation: object         # [S, W] int32
    gated: object               # [S, W] int32
    argmax: object              # [S, W] int32: the lag of the extremum (0 where gated)
    shown_delay_ms: object      # [S, R] ([S] with keep="last"): what the widget shows after each refresh chunk
    shown_distance_m: object
    shown_extremum: object
    shown_correlation: object   # int32
    xcorr: object               # [S, W, L] with with_xcorr (zeros where gated), else None
    state: DelayState


class DelayEstimatorBatch:
    """S two-channel streams of a whole recording through the delay estimator's chain in a few device calls, as widgets fed
    chunk by chunk would have seen it: both channels through the two chained decimations in a time-parallel form
    (frt_delaybatch_decimate), every window of the widgets' rings rebuilt from delay_schedule's run table, GCC-PHAT of all of
    them in slabs (frt_delaybatch_windows, frt_gcc_phat), smoothing and read-out in window order (frt_delaybatch_readout).

    run(x, chunk=512 | ends=..., state=None, keep="last" | "all", with_xcorr=False, scratch_bytes=1 << 30) takes [S, 2, T]
    (the stream axis may be left out), float32 or float64, a numpy array or a CUDA tensor; results are of the same kind.

    What is reproduced, because the reference widget and DelayEstimatorStream both show it at the default settings:
      * the windows are views of the ring, and GCC-PHAT subtracts their means in place (correlation.py:27-28): the overlap half
        of the next window holds this window's samples minus this window's mean where both views lie at the same ring
        positions, and the untouched mirror copy where the view wrapped or the ring grew in between;
      * the ring starts at 10000 samples and grows only on request (ringbuffer.py:102-130): with windows longer than that (any
        range above about 0.41 s) the first windows hold zeros where samples had been overwritten before the growth.
    Both are functions of indices, planned on the host.  The gate is DelayEstimatorStream's: a window is silent (reads 0, keeps
    the smoothed correlation, subtracts nothing) where every effective sample of a channel is equal; numpy.std of a constant
    non-zero window is 0 or rounding noise depending on the value and the summation order, so the reference's own behaviour
    there is not defined by its arithmetic.  Every chunk holds a multiple of 4 samples.  Fixed delay range, no pause.

    The correlations of all windows ([S, W, L] float64) are held on the device whether with_xcorr asks for them or not; the
    effective windows go to GCC-PHAT in slabs of pairs that fit scratch_bytes (a pair at least).  The caller's state is never
    written to.  A recording in pieces equals the whole to rounding.  The GCC-PHAT handles are pinned to one workgroup per pair,
    so that a pair's bits do not depend on the slab size."""

    def __init__(self, delayrange_s: float = DEFAULT_DELAYRANGE):
        t = filter_design.load_tables()
        self.delayrange_s = delayrange_s
        self.Ndec = DELAY_NDEC
        self.subsampled_sampling_rate = SAMPLING_RATE / 2 ** self.Ndec
        self.bdec, self.adec = np.ascontiguousarray(t["bdec"], np.float64), np.ascontiguousarray(t["adec"], np.float64)
        self.length, self.needed = delay_lengths(delayrange_s)
        self.last_slabs = 0
        self._gcc = {}

    def schedule(self, n_samples, chunk=512, ends=None, state=None):
        return delay_schedule(n_samples, self.delayrange_s, chunk, ends, state)

    def _plan(self, n_pairs):
        """The GCC-PHAT handle of a slab size: one workgroup per pair whatever the slab's size, so that a pair's bits do not
        depend on how many ride along."""
        if n_pairs not in self._gcc:
            self._gcc[n_pairs] = GccPhat(self.length, n_pairs, one_workgroup=True)
        return self._gcc[n_pairs]

    def _check_input(self, x, state):
        x, is_np, squeeze, pending = check_samples("DelayEstimatorBatch", x, state, dual=True)
        if state is not None:
            S, L = x.shape[0], self.length
            if not isinstance(state.ring, DelayRing) or state.ring.length != L:
                raise ValueError(f"the state belongs to another delay range (windows of {getattr(state.ring, 'length', None)} samples, not {L})")
            want = {"zi": (S, 2, self.Ndec, 12), "samples": (S, 2, 0), "tail": (S, 2, L + pending), "means": (S, 2), "gated": (S,),
                    "smoothed": (S, L), "present": (S,), "readout": (S, 4)}
            got = {name: tuple(getattr(state, name).shape) for name in want}
            if pending < 0 or pending != state.ring.offset - state.ring.old_index or got != want:
                raise ValueError(f"state of another shape: {got} (want {want}), pending {pending}")
        return x, is_np, squeeze, pending

    def run(self, x, chunk=512, ends=None, state=None, keep="last", with_xcorr=False, scratch_bytes=1 << 30):
        import ctypes

        from . import _lib
        check_keep(keep, "last", "all")
        x, is_np, squeeze, pending = self._check_input(x, state)
        plan = self.schedule(x.shape[-1], chunk, ends, state)
        import torch
        lib = _lib.init()
        S, T, L, W, R = x.shape[0], x.shape[-1], self.length, len(plan.window_end), len(plan.refresh_chunk)
        f64, i32, vp = torch.float64, torch.int32, ctypes.c_void_p
        DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
        seen = 0 if state is None else int(state.seen)
        with null_stream(x, is_np) as dev:
            xd = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) if is_np else x).reshape(2 * S, T)
            if T and xd.stride(1) != 1:
                xd = xd.contiguous()
            st = state
            zi = carried(dev, None if st is None else st.zi, (2 * S, self.Ndec, 12))
            zf = torch.empty_like(zi)
            n_all = plan.tail + plan.n_dec
            dec = torch.empty((2 * S, n_all), dtype=f64, device=dev)
            dec[:, :plan.tail] = carried(dev, None if st is None else st.tail, (2 * S, plan.tail), copy=False)
            n_out = ctypes.c_int64(0)
            _lib.check(lib.frt_delaybatch_decimate(
                self.bdec.ctypes.data_as(DP), self.adec.ctypes.data_as(DP), len(self.bdec), self.Ndec, vp(xd.data_ptr()),
                int(xd.dtype == f64), 2 * S, T, xd.stride(0) if T else 0, seen, vp(zi.data_ptr()),
                vp(dec.data_ptr() + 8 * plan.tail), n_all, vp(zf.data_ptr()), ctypes.byref(n_out)))
            assert n_out.value == plan.n_dec
            means_in = carried(dev, None if st is None else st.means, (S, 2))
            sm_in = carried(dev, None if st is None else st.smoothed, (S, L), copy=False)
            present_in = (torch.zeros(S, dtype=i32, device=dev) if st is None
                          else torch.as_tensor(st.present).to(device=dev, dtype=i32).reshape(S).clone())
            shown_in = carried(dev, None if st is None else st.readout, (S, 4))
            sm_out, present_out = torch.empty((S, L), dtype=f64, device=dev), torch.empty(S, dtype=i32, device=dev)
            xcorr = torch.empty((S, W, L), dtype=f64, device=dev)
            means = torch.empty((S, W, 2), dtype=f64, device=dev)
            gated, argmax, corr = (torch.empty((S, W), dtype=i32, device=dev) for _ in range(3))
            delay, dist, ext = (torch.empty((S, W), dtype=f64, device=dev) for _ in range(3))
            self.last_slabs = 0
            if W:
                per = int(min(S * W, 65535, max(1, int(scratch_bytes) // (2 * L * 8))))
                runs = np.ascontiguousarray(plan.runs, np.int64)
                slabs = ctypes.c_int(0)
                full, last = self._plan(per), self._plan((S * W) % per or per)
                for g in (full, last):
                    _lib.check(lib.frt_gcc_set_stream(g._h, None))
                _lib.check(lib.frt_delaybatch_windows(
                    vp(dec.data_ptr()), n_all, n_all, S, L, W, runs.ctypes.data_as(IP), vp(means_in.data_ptr()), full._h, per, last._h,
                    vp(xcorr.data_ptr()), vp(means.data_ptr()), vp(gated.data_ptr()), ctypes.byref(slabs)))
                self.last_slabs = slabs.value
            _lib.check(lib.frt_delaybatch_readout(
                vp(xcorr.data_ptr()), vp(gated.data_ptr()), S, W, L, vp(sm_in.data_ptr()), vp(present_in.data_ptr()), 0.3,
                float(self.subsampled_sampling_rate), float(self.delayrange_s), vp(sm_out.data_ptr()), vp(present_out.data_ptr()),
                vp(argmax.data_ptr()), vp(delay.data_ptr()), vp(dist.data_ptr()), vp(ext.data_ptr()), vp(corr.data_ptr())))
            if W and with_xcorr:                                      # gated pairs rode along: what came of them is not a correlation
                xcorr.masked_fill_(gated.bool()[..., None], 0.0)
            if R:
                at = torch.from_numpy(plan.window_start[1:] - 1).to(dev)
                shown = [delay[:, at], dist[:, at], ext[:, at], corr[:, at]]
            else:
                shown = [shown_in[:, k:k + 1] for k in range(3)] + [shown_in[:, 3:4].to(i32)]
            readout = torch.stack([v[:, -1].to(f64) for v in shown], dim=1)
            if keep == "last":
                shown = [v[:, -1] for v in shown]
            elif not R:
                shown = [v[:, :0] for v in shown]
            pending_out = plan.ring.offset - plan.ring.old_index
            new_state = DelayState(zf.reshape(S, 2, self.Ndec, 12), torch.empty((S, 2, 0), dtype=f64, device=dev),
                                   dec[:, n_all - (L + pending_out):].reshape(S, 2, L + pending_out).clone(), pending_out, plan.ring,
                                   means[:, -1].clone() if W else means_in, gated[:, -1].clone() if W else
                                   (torch.zeros(S, dtype=i32, device=dev) if st is None else torch.as_tensor(st.gated).to(device=dev, dtype=i32).reshape(S).clone()),
                                   sm_out, present_out, readout, seen + T)
            fields = [delay, dist, ext, corr, gated, argmax, *shown, xcorr if with_xcorr else None]
            if squeeze:
                fields = [None if v is None else v[0] for v in fields]
            if is_np:
                ring = new_state.ring
                fields, new_state = to_host(tuple(fields)), to_host(new_state._replace(ring=None))._replace(ring=ring)
        return DelayResult(plan.window_end, plan.window_start, plan.refresh_chunk, *fields, new_state)
