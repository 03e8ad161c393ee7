"""What the batch classes (LevelsBatch, ScopeBatch, CurveBatch, SpectrumBatch, SpectrogramBatch) share: their input is a float32/float64 numpy
array or CUDA tensor, their results are of the same kind, and a recording is seen in chunks."""
from __future__ import annotations

import numpy as np


def chunk_ends(T, chunk=512):
    """The stream ends at which a widget fed `chunk`-sample chunks refreshes (a short last chunk is a short chunk)."""
    return np.minimum(np.arange(1, -(-T // chunk) + 1, dtype=np.int64) * chunk, T)


def frame_schedule(n_samples, needed, hop, chunk=512, ends=None, pending=0):
    """(frame_start [R + 1], refresh_chunk [R]) of a stream of n_samples seen chunk by chunk by a widget that transforms
    realizable = floor(available / needed) frames per chunk and advances by hop = int(needed) per frame (friture/spectrum.py:
    133-155, friture/spectrogram.py:131-160); `pending`: samples received and not consumed before the first one.  `ends`: the
    chunks' end indices, for ragged chunks; default: the ends of `chunk`-sample chunks, a short last chunk is a short chunk."""
    n_samples = int(n_samples)
    if ends is None:
        if chunk < 1:
            raise ValueError(f"chunk {chunk}")
        ends = chunk_ends(n_samples, chunk)
    else:
        ends = np.asarray(ends, np.int64).reshape(-1)
        if ends.size and (ends[0] < 0 or ends[-1] > n_samples or np.any(np.diff(ends) < 0)):
            raise ValueError(f"ends must be sorted and within [0, {n_samples}]")
    old_index = -int(pending)
    frame_start, refresh_chunk = [0], []
    for c, e in enumerate(ends.tolist()):
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
