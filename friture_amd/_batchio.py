"""What the batch classes share.  All of them (LevelsBatch, ScopeBatch, CurveBatch, SpectrumBatch, SpectrogramBatch, PitchBatch,
OctaveSpectrumBatch, DelayEstimatorBatch, Resampler, LoudnessBatch, TransferBatch, ConvolveBatch, DecayBatch, DeconvolveBatch, MtfBatch, SosBatch, SoundLevelBatch): their input is a float32/float64
numpy array or CUDA tensor and their results are of the same kind (ptr, source, alloc).  The widget batches: a recording is seen
in chunks (chunk_ends, checked_ends, frame_schedule); for the five chains over recordings, the host side of run(): the input
checks (check_keep, check_samples; `dual` for two rows per stream), the hand-over to the null stream, the device copy of a
carried state (carried) and the way back to numpy (to_host); for the two STFT chains, the sample front (RecordingFront).  The
recording chains (Resampler, LoudnessBatch, TransferBatch, ConvolveBatch, DecayBatch, DeconvolveBatch, MtfBatch, SosBatch, SoundLevelBatch): the checks of the stream count and of scratch_bytes,
the rows read in place (strided_rows) and the numpy / CUDA fork of run() (run_call).  The chains over rows of samples (DecayBatch,
MtfBatch; rowfront.h is their library side): the checks of fs and of the samples per row (check_fs, check_row_samples) and the
per-row integers of onset / truncate / start / stop (row_integers)."""
from __future__ import annotations

import ctypes
import math
from contextlib import contextmanager

import numpy as np

from . import _lib


def chunk_ends(T, chunk=512):
    """The stream ends at which a widget fed `chunk`-sample chunks refreshes (a short last chunk is a short chunk)."""
    return np.minimum(np.arange(1, -(-T // chunk) + 1, dtype=np.int64) * chunk, T)


def checked_ends(n_samples, chunk=512, ends=None):
    """The chunks' end indices as an int64 vector: `ends`, sorted and within [0, n_samples], or the ends of `chunk`-sample chunks."""
    n_samples = int(n_samples)
    if ends is None:
        if chunk < 1:
            raise ValueError(f"chunk {chunk}")
        return chunk_ends(n_samples, chunk)
    ends = np.asarray(ends, np.int64).reshape(-1)
    if ends.size and (ends[0] < 0 or ends[-1] > n_samples or np.any(np.diff(ends) < 0)):
        raise ValueError(f"ends must be sorted and within [0, {n_samples}]")
    return ends


def frame_schedule(n_samples, needed, hop, chunk=512, ends=None, pending=0):
    """(frame_start [R + 1], refresh_chunk [R]) of a stream of n_samples seen chunk by chunk by a widget that transforms
    realizable = floor(available / needed) frames per chunk and advances by hop = int(needed) per frame (friture/spectrum.py:
    133-155, friture/spectrogram.py:131-160); `pending`: samples received and not consumed before the first one.  `ends`: the
    chunks' end indices, for ragged chunks; default: the ends of `chunk`-sample chunks, a short last chunk is a short chunk."""
    old_index = -int(pending)
    frame_start, refresh_chunk = [0], []
    for c, e in enumerate(checked_ends(n_samples, chunk, ends).tolist()):
        realizable = int(np.floor((e - old_index) / needed))
        if realizable > 0:
            frame_start.append(frame_start[-1] + realizable)
            refresh_chunk.append(c)
            old_index += realizable * hop
    return np.array(frame_start, np.int64), np.array(refresh_chunk, np.int64)


def ptr(a):
    """The address of a numpy array or tensor; None stays None."""
    if a is None:
        return None
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def source(x, strided):
    """(x, address, dtype code 0 float32 / 1 float64, strides in elements) of a kernel's input.  strided: the leading axes are
    read in place and only a last axis that is not unit-stride (numpy: or a negative or unaligned stride) costs a copy;
    otherwise x is made contiguous as a whole."""
    if isinstance(x, np.ndarray):
        assert x.dtype in (np.float32, np.float64)
        if not strided or x.strides[-1] != x.itemsize or any(st % x.itemsize or st < 0 for st in x.strides):
            x = np.ascontiguousarray(x)
        return x, x.ctypes.data, int(x.dtype == np.float64), tuple(st // x.itemsize for st in x.strides)
    import torch
    assert x.is_cuda and x.dtype in (torch.float32, torch.float64)
    if not strided or x.stride(-1) != 1:
        x = x.contiguous()
    return x, x.data_ptr(), int(x.dtype == torch.float64), x.stride()


def alloc(like, shape, dtype=np.float64, zero=False):
    """A new array of the kind of `like` (numpy for a numpy array, on its device for a CUDA tensor), uninitialised or zeros."""
    name = "zeros" if zero else "empty"
    if isinstance(like, np.ndarray):
        return getattr(np, name)(shape, dtype)
    import torch
    return getattr(torch, name)(shape, dtype=getattr(torch, np.dtype(dtype).name), device=like.device)


# ---- the host side of run() of the chains over recordings ----------------------------------------------------------------------

def check_keep(keep, *allowed):
    if keep not in allowed:
        raise ValueError(f"keep={keep!r} ({' or '.join(repr(a) for a in allowed)})")


def check_samples(who, x, state, dual=False):
    """(x with its stream axis, is_np, squeeze, pending) of a recording x [S, T] ([S, 2, T] with `dual`; the stream axis may be
    left out) and a carried state (None: a fresh widget)."""
    is_np = isinstance(x, np.ndarray)
    if not is_np and not (type(x).__module__.startswith("torch") and x.is_cuda):
        raise TypeError(f"{who}.run takes a numpy array or a CUDA tensor")
    full = 3 if dual else 2
    if x.ndim not in (full - 1, full):
        raise ValueError(f"expected [S, {'2, ' if dual else ''}T] (the stream axis may be left out), got {tuple(x.shape)}")
    if str(x.dtype).split(".")[-1] not in ("float32", "float64"):
        raise TypeError(f"samples must be float32 or float64, got {x.dtype}")
    squeeze = x.ndim == full - 1
    if squeeze:
        x = x[None]
    if dual and x.shape[1] != 2:
        raise ValueError(f"dual channels need two rows per stream, got {x.shape[1]}")
    return x, is_np, squeeze, 0 if state is None else int(state.pending)


def check_streams(S):
    if not 1 <= S <= 65535:
        raise ValueError(f"expected 1 .. 65535 streams, got {S}")


def check_scratch_bytes(scratch_bytes):
    if isinstance(scratch_bytes, bool) or not isinstance(scratch_bytes, (int, np.integer)) or scratch_bytes < 0:
        raise ValueError(f"scratch_bytes must be an integer >= 0, got {scratch_bytes!r}")


def check_row_samples(T):
    if not 1 <= T <= 1 << 24:
        raise ValueError(f"expected 1 .. 2^24 samples per row, got {T}")


def check_fs(fs):
    if not (isinstance(fs, (int, float, np.integer, np.floating)) and math.isfinite(fs) and 100 <= fs <= 1e7):
        raise ValueError(f"fs must lie in 100 .. 1e7, got {fs!r}")


def row_integers(name, v, R, lo, hi, device=False):
    """[R] int64 on the host from integers [R] or a scalar (a tensor comes to the host), every value within lo .. hi.
    device=True: an int64 CUDA tensor passes as it is, unchecked: a bad value makes its row dead in the kernel."""
    if device and getattr(v, "is_cuda", False):
        import torch
        if v.dtype != torch.int64 or tuple(v.shape) not in ((R,), ()) or v.numel() != R:
            raise ValueError(f"{name} must be int64 [{R}], got {v.dtype} {tuple(v.shape)}")
        return v.reshape(R).contiguous()
    if hasattr(v, "cpu"):
        v = v.cpu().numpy()
    v = np.asarray(v)
    if v.dtype.kind not in "iu" or v.shape not in ((R,), ()):
        raise ValueError(f"{name} must be integers [{R}], got {v.dtype} {v.shape}")
    v = np.ascontiguousarray(np.broadcast_to(v, (R,)), np.int64)
    if v.size and (v.min() < lo or v.max() > hi):
        raise ValueError(f"{name} must lie in {lo} .. {hi}, got {int(v.min())} .. {int(v.max())}")
    return v


def strided_rows(x, dual=False):
    """(x, address, dtype code, row stride, pair stride) of the rows x [S, T] ([S, 2, T] with `dual`) of a recording chain, strides
    in elements: read in place where source(x, strided=True) can, from a contiguous copy when the rows overlap (a broadcast
    view).  The row stride is at least max(T, 1), whatever a single row's own says; the pair stride is 0 without `dual` and for
    S = 1."""
    S, T = x.shape[0], x.shape[-1]
    for strided in (True, False):
        x, address, code, strides = source(x, strided)
        row = strides[-2] if dual or S > 1 else T
        pair = strides[0] if dual and S > 1 else 0
        if not T or (row >= T and pair >= 0):
            break
    return x, address, code, max(row, T, 1), pair


@contextmanager
def null_stream(x, is_np):
    """The batch kernels launch on the null stream (friture_hip.h): inside, everything is enqueued there, after whatever the
    caller's stream still has to do to x; afterwards the caller's stream may read the results.  Yields the device."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if is_np else x.device
    mine, null = torch.cuda.current_stream(dev), torch.cuda.default_stream(dev)
    if mine != null:
        mine.synchronize()
    with torch.cuda.device(dev), torch.cuda.stream(null):
        yield dev
    if mine != null:
        null.synchronize()


def carried(dev, value, shape, fill=0.0, copy=True):
    """A float64 copy on `dev` of an array that a state carries: what run() writes to must not be the caller's state.  None, a
    fresh widget: `fill`.  copy=False is for RecordingFront's tail alone, which is only read: a contiguous CUDA float64 tail is
    then taken as it is, as it always was, and a call with a carried state is spared one device copy of [C, fft_size + pending]."""
    import torch
    if value is None:
        return torch.full(shape, fill, dtype=torch.float64, device=dev) if fill else torch.zeros(shape, dtype=torch.float64, device=dev)
    value = torch.as_tensor(value).to(device=dev, dtype=torch.float64).reshape(shape)
    return value.clone() if copy else value.contiguous()


def run_call(x, is_np, outputs, set_stream, call, state, device_state=None):
    """The numpy / CUDA fork of a recording chain's run(): call(state_in, *outputs()) and the outputs.  outputs() makes the new
    arrays of x's kind.  numpy: the carried `state` goes in as a host float64 array (None: a fresh stream).  CUDA: everything
    happens inside null_stream, the outputs are made there, set_stream() points the handle at the null stream, and the state
    goes in as device_state(dev, state); default: None for a fresh stream, otherwise the state as it is when it is a
    contiguous float64 tensor on dev (it is only read)."""
    if is_np:
        outs = outputs()
        call(None if state is None else np.ascontiguousarray(to_host(state), np.float64), *outs)
        return outs
    with null_stream(x, is_np) as dev:
        outs = outputs()
        set_stream()
        if device_state is not None:
            state = device_state(dev, state)
        elif state is not None:
            state = carried(dev, state, tuple(state.shape), copy=False)
        call(state, *outs)
    return outs


def to_host(value):
    """`value` with its tensors as numpy arrays: a (named) tuple field by field, anything else as it is.  EVERY tensor field
    comes to the host: a state that is to keep a field on the device for numpy input must not go through here whole."""
    if isinstance(value, tuple):
        fields = [to_host(v) for v in value]
        return type(value)(*fields) if hasattr(value, "_fields") else tuple(fields)
    return value.cpu().numpy() if hasattr(value, "cpu") else value


class RecordingFront:
    """The samples of a recording x [S, (rows,) T] behind a carried tail, as C = S * rows device rows, and the frames of a
    schedule transformed from them slab by slab.  To be made and used inside null_stream: making it stages x, load_tail the
    tail (a step of its own, so that each class keeps the order in which its state reaches the stream)."""

    def __init__(self, x, is_np, dev, pending, fft_size, hop, frame_start, ends=None):
        import torch
        self.torch, self.dev, self.N, self.hop, self.frame_start = torch, dev, fft_size, hop, frame_start
        self.C, self.L, self.F, self.T = math.prod(x.shape[:-1]), fft_size + pending, int(frame_start[-1]), x.shape[-1]
        if ends is not None:                                        # the widgets were pushed ends[-1] samples
            self.T = int(np.asarray(ends).reshape(-1)[-1]) if np.size(ends) else 0
        self.x = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) if is_np else x).reshape(self.C, x.shape[-1])
        if self.x.stride(1) != 1:
            self.x = self.x.contiguous()

    def load_tail(self, tail):
        """The carried tail (None: zeros); it is only read."""
        self.tail = carried(self.dev, tail, (self.C, self.L), copy=False)

    def window(self, a, b):
        """Samples [a, b) of tail || x per row as float64 (float32 widens exactly), unit stride along time."""
        x, L = self.x, self.L
        if a >= L and x.dtype == self.torch.float64:
            return x[:, a - L:b - L]
        out = self.torch.empty((self.C, b - a), dtype=self.torch.float64, device=self.dev)
        if a < L:
            out[:, :min(b, L) - a] = self.tail[:, a:min(b, L)]
        if b > L:
            out[:, max(a, L) - a:] = x[:, max(a, L) - L:b - L]
        return out

    def transform(self, eng, kind, n_bins, scratch_bytes, f_lo=0):
        """The frames from f_lo on, in time slabs of whole refreshes r0 .. r1 - 1, at most scratch_bytes of float64 frames each
        (one refresh if it alone has more; slabs that end at or before f_lo drop out).  Per slab: one frt_stft_run of `kind` over
        its frames fa .. fb - 1 on the null stream into a scratch buffer [C, fb - fa, n_bins] (sized for the largest slab, freed
        when the loop ends), then yields (r0, r1, fa, fb, the buffer's address)."""
        lib, vp, fs = _lib.init(), ctypes.c_void_p, self.frame_start
        _lib.check(lib.frt_stft_set_stream(eng._h, None))
        fmax = max(1, int(scratch_bytes) // (self.C * n_bins * 8))
        slabs, r0 = [], 0
        while r0 < len(fs) - 1:
            r1 = max(r0 + 1, int(np.searchsorted(fs, fs[r0] + fmax, "right")) - 1)
            if fs[r1] > f_lo:
                slabs.append((r0, r1, max(int(fs[r0]), f_lo), int(fs[r1])))
            r0 = r1
        out = self.torch.empty(self.C * n_bins * max(fb - fa for _, _, fa, fb in slabs), dtype=self.torch.float64, device=self.dev)
        nfo = ctypes.c_int64(0)
        for r0, r1, fa, fb in slabs:
            seg = self.window(fa * self.hop, (fb - 1) * self.hop + self.N)
            _lib.check(lib.frt_stft_run(eng._h, kind, vp(seg.data_ptr()), seg.shape[1], seg.stride(0) if self.C > 1 else seg.shape[1],
                                        vp(out.data_ptr()), ctypes.byref(nfo)))
            assert nfo.value == fb - fa
            yield r0, r1, fa, fb, vp(out.data_ptr())

    def new_tail(self):
        """(tail [C, fft_size + pending] float64, pending) behind the schedule's last frame: what the next call carries in."""
        return self.window(self.F * self.hop, self.L + self.T).clone(), self.L + self.T - self.F * self.hop - self.N
