"""What the batch classes (LevelsBatch, ScopeBatch, CurveBatch, SpectrumBatch) share: their input is a float32/float64 numpy
array or CUDA tensor, their results are of the same kind, and a recording is seen in chunks."""
from __future__ import annotations

import numpy as np


def chunk_ends(T, chunk=512):
    """The stream ends at which a widget fed `chunk`-sample chunks refreshes (a short last chunk is a short chunk)."""
    return np.minimum(np.arange(1, -(-T // chunk) + 1, dtype=np.int64) * chunk, T)


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
