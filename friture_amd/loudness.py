"""How loud a recording is and whether it clips between the samples: programme loudness per ITU-R BS.1770-4 / EBU R 128
(momentary, short-term, integrated with both gates, loudness range per EBU Tech 3342) and true peak, on the GPU
(loudness.hip, frt_loudness_*; the definition: L2 in include/friture_hip.h).

Samples are at SAMPLING_RATE, the one rate for which BS.1770 states its filter (resample first: Resampler, to_48k).  A stream
is K-weighted (two biquads, float64), its energy summed per sub-block of SUB_BLOCK = 4800 samples on the absolute grid, and
its sample peak max |x| and true peak max |u| taken per sub-block, u being the output of Resampler(48000, 192000,
zeros=tp_zeros) — the interpolator is that converter's own prototype, not a second design.  P programmes of C channels with
weights G: a 400 ms block every 100 ms is z400[j] = sum_c G[c] (e[j] + .. + e[j + 3]) / 19200, a 3 s block the same over 30
sub-blocks; loudness l(z) = -0.691 + 10 log10 z.  After N samples a stream that is not flushed has emitted
max(0, (N - tp_zeros) // 4800) sub-blocks (the last true-peak tap of a sub-block arrives tp_zeros samples past its end), a
flushed one N // 4800 energies and ceil(N / 4800) peak entries.  There is no CPU fallback: run() goes to the HIP library."""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import numpy as np

from . import _batchio, _lib
from .constants import SAMPLING_RATE
from .resample import Resampler

SUB_BLOCK = 4800                            # samples per sub-block: 100 ms
ENERGY_TAIL = 29                            # sub-block energies a state carries: a 3 s block spans 30
ABSOLUTE_GATE = -70.0
MAX_TP_ZEROS = 512                          # frt_loudness_create refuses more
PRESETS = {"mono": (1.0,), "stereo": (1.0, 1.0), "5.0": (1.0, 1.0, 1.0, 1.41, 1.41), "5.1": (1.0, 1.0, 1.0, 0.0, 1.41, 1.41)}

# data: one float64 array (its layout: state_layout); streams; samples taken; peak entries emitted
LoudnessState = namedtuple("LoudnessState", "data streams n_in n_blocks")
LoudnessResult = namedtuple("LoudnessResult", "momentary short_term integrated loudness_range true_peak_db sample_peak_db energy "
                                              "true_peak sample_peak state")


def channel_weights(channels):
    """The weights G[c] of a preset name or of an explicit sequence."""
    if isinstance(channels, str):
        if channels not in PRESETS:
            raise ValueError(f"channels={channels!r} ({', '.join(repr(k) for k in PRESETS)} or a sequence of weights)")
        return PRESETS[channels]
    w = tuple(float(v) for v in channels)
    if not 1 <= len(w) <= 64 or any(not math.isfinite(v) or v < 0 for v in w):
        raise ValueError(f"channel weights {channels!r} (1 .. 64 finite values, none negative)")
    return w


def emitted(n_in, tp_zeros, flush):
    """(sub-blocks with an energy, sub-blocks with peaks) after n_in samples in total."""
    n_in = int(n_in)
    if flush:
        return n_in // SUB_BLOCK, -(-n_in // SUB_BLOCK)
    e = max(0, (n_in - tp_zeros) // SUB_BLOCK)
    return e, e


def n_blocks_400ms(energies):
    return max(0, energies - 3)


def n_blocks_3s(energies):
    return max(0, energies - ENERGY_TAIL)


def state_layout(S, P, tp_zeros, n_in, energies):
    """name -> (offset, shape) of the parts of a state's data after n_in samples and `energies` sub-blocks, and its length."""
    parts = (("filter", (S, 4)), ("samples", (S, n_in - energies * SUB_BLOCK + tp_zeros)), ("energy_tail", (S, min(ENERGY_TAIL, energies))),
             ("z400", (P, n_blocks_400ms(energies))), ("z3s", (P, n_blocks_3s(energies))))
    out, at = {}, 0
    for name, shape in parts:
        out[name] = (at, shape)
        at += shape[0] * shape[1]
    return out, at


def _lkfs(z):
    """-0.691 + 10 log10 z, -inf where z == 0; numpy array or tensor."""
    if isinstance(z, (np.ndarray, np.generic)):
        with np.errstate(divide="ignore"):
            return -0.691 + 10.0 * np.log10(z)
    import torch
    return -0.691 + 10.0 * torch.log10(z)


def _db(v):
    if isinstance(v, np.ndarray):
        with np.errstate(divide="ignore"):
            return 20.0 * np.log10(v)
    import torch
    return 20.0 * torch.log10(v)


def loudness_range(short_term_power):
    """LRA per EBU Tech 3342 of the 3 s block powers z3s [n] or [P, n] (numpy array or tensor), one value per row, of the same
    kind: of the short-term values l > -70, Gamma = l(mean of their z3s) - 20; those above Gamma sorted ascending as v[0 .. n - 1];
    LRA = v[floor((n - 1) 0.95 + 0.5)] - v[floor((n - 1) 0.10 + 0.5)], 0 for n < 2."""
    z = short_term_power
    rows = z.reshape(1, -1) if z.ndim == 1 else z
    if rows.shape[1] == 0:
        out = _batchio.alloc(z, (rows.shape[0],), zero=True)
        return out[0] if z.ndim == 1 else out
    # every programme at once and nothing that waits for the device: the rejected values sort to the end as +inf
    if isinstance(z, np.ndarray):
        xp, sort, take = np, (lambda a: np.sort(a, axis=1)), (lambda a, i: np.take_along_axis(a, i[:, None], 1)[:, 0])
        real, index = np.float64, np.int64
    else:
        import torch as xp
        sort, take = (lambda a: a.sort(dim=1).values), (lambda a, i: a.gather(1, i[:, None])[:, 0])
        real, index = xp.float64, xp.int64
    l = _lkfs(rows)
    keep = l > ABSOLUTE_GATE
    count = keep.sum(1)
    mean = xp.where(keep, rows, xp.zeros_like(rows)).sum(1) / xp.where(count > 0, count, xp.ones_like(count))
    gamma = _lkfs(mean) - 20.0                                      # -inf for a programme with nothing above the absolute gate
    keep = keep & (l > gamma[:, None])
    v = sort(xp.where(keep, l, xp.full_like(l, math.inf)))
    n = keep.sum(1)
    last = xp.where(n > 0, n - 1, xp.zeros_like(n)).astype(real) if xp is np else xp.where(n > 0, n - 1, xp.zeros_like(n)).to(real)
    hi, lo = xp.floor(last * 0.95 + 0.5), xp.floor(last * 0.10 + 0.5)
    hi, lo = (hi.astype(index), lo.astype(index)) if xp is np else (hi.to(index), lo.to(index))
    v = xp.where(xp.isinf(v), xp.zeros_like(v), v)                 # never read where n >= 2; keeps inf - inf out of the other rows
    out = xp.where(n >= 2, take(v, hi) - take(v, lo), xp.zeros_like(mean))
    return out[0] if z.ndim == 1 else out


class LoudnessBatch:
    """run(x, state=None, flush=True) -> LoudnessResult.  x: [S, T] (S a multiple of the channels of a programme, programme p
    being rows p C .. p C + C - 1) or [P, C, T] ([T]: one mono stream), float32 or float64, numpy array or CUDA tensor (rows read
    in place).  channels: "mono", "stereo", "5.0", "5.1" (the LFE, fourth, at weight 0) or a sequence of weights.  Results are
    float64 and of x's kind: momentary [P, new 400 ms blocks] and short_term [P, new 3 s blocks] in LUFS, integrated [P] and
    loudness_range [P] over the whole stream so far, energy [S, new sub-blocks], true_peak / sample_peak [S, new sub-blocks]
    (linear) and their dBTP / dBFS values; true_peak=False skips the interpolator (true_peak and true_peak_db are None).
    flush=False keeps the sub-blocks whose last true-peak tap has not arrived for the next call, which continues with `state`; a
    recording cut into calls at any points gives the bits of one call.  After flush=True a partial last sub-block has peak
    entries (zeros behind the end) and no energy, and the state is final."""

    def __init__(self, channels="stereo", tp_zeros=16, true_peak=True):
        self.weights = channel_weights(channels)
        self.channels = len(self.weights)
        if isinstance(tp_zeros, bool) or not isinstance(tp_zeros, (int, np.integer)) or not 1 <= tp_zeros <= MAX_TP_ZEROS:
            raise ValueError(f"tp_zeros must be an integer in 1 .. {MAX_TP_ZEROS}, got {tp_zeros!r}")
        self.tp_zeros = int(tp_zeros)
        self.true_peak = bool(true_peak)
        self.prototype = Resampler(SAMPLING_RATE, 4 * SAMPLING_RATE, zeros=self.tp_zeros).prototype
        self._handles = {}

    # ---- host only ------------------------------------------------------------------------------------------------------------
    def emitted(self, n_in, flush=True):
        """(sub-blocks with an energy, sub-blocks with peaks) after n_in samples in total."""
        return emitted(n_in, self.tp_zeros, flush)

    def state_parts(self, state):
        """The parts of a state as views of its data: filter [S, 4], samples, energy_tail, z400 [P, n], z3s [P, n]."""
        S = state.streams
        n_in, peaks = int(state.n_in), int(state.n_blocks)
        energies = peaks if peaks == self.emitted(n_in, False)[0] else n_in // SUB_BLOCK
        layout, _ = state_layout(S, S // self.channels, self.tp_zeros, n_in, energies)
        return {name: state.data[at:at + shape[0] * shape[1]].reshape(shape) for name, (at, shape) in layout.items()}

    def _check_state(self, state, S):
        if state is None:
            return None, 0, 0
        data, streams, n_in, n_blocks = state
        n_in, n_blocks = int(n_in), int(n_blocks)
        if int(streams) != S:
            raise ValueError(f"state of another shape: {streams} streams (want {S})")
        if n_in < 0 or n_blocks != self.emitted(n_in, False)[0]:
            if n_in >= 0 and n_blocks == self.emitted(n_in, True)[1]:
                raise ValueError("the state is final: it was flushed")
            raise ValueError(f"state of another stream: {n_blocks} sub-blocks after {n_in} samples")
        want = state_layout(S, S // self.channels, self.tp_zeros, n_in, n_blocks)[1]
        if data.ndim != 1 or data.shape[0] != want:
            raise ValueError(f"state of another shape: data {tuple(data.shape)} (want {(want,)})")
        return data, n_in, n_blocks

    def _rows(self, x):
        """(x as [S, T] rows, whether the programme axis is to be put back, squeeze)"""
        is_np = isinstance(x, np.ndarray)
        if not is_np and not (type(x).__module__.startswith("torch") and x.is_cuda):
            raise TypeError("LoudnessBatch.run takes a numpy array or a CUDA tensor")
        if str(x.dtype).split(".")[-1] not in ("float32", "float64"):
            raise TypeError(f"samples must be float32 or float64, got {x.dtype}")
        C = self.channels
        if x.ndim == 1:
            if C != 1:
                raise ValueError(f"expected [S, T] or [P, {C}, T] for programmes of {C} channels, got {tuple(x.shape)}")
            return x[None], is_np, True
        if x.ndim == 2:
            if x.shape[0] < 1 or x.shape[0] % C:
                raise ValueError(f"expected whole programmes of {C} channels, got {x.shape[0]} streams")
            return x, is_np, False
        if x.ndim == 3:
            if x.shape[0] < 1 or x.shape[1] != C:
                raise ValueError(f"expected [P, {C}, T], got {tuple(x.shape)}")
            x, _, _, st = _batchio.source(x, strided=True)
            P, T = x.shape[0], x.shape[2]
            step = st[0] if C == 1 else st[1] if P == 1 or st[0] == C * st[1] else None
            if step is None:                                         # the rows of all programmes are not evenly spaced: one copy
                x = np.ascontiguousarray(x) if is_np else x.contiguous()
                return x.reshape(P * C, T), is_np, False
            if is_np:
                return np.lib.stride_tricks.as_strided(x, (P * C, T), (step * x.itemsize, x.itemsize), writeable=False), is_np, False
            return x.as_strided((P * C, T), (step, 1), x.storage_offset()), is_np, False
        raise ValueError(f"expected [S, T] or [P, {C}, T], got {tuple(x.shape)}")

    # ---- device ---------------------------------------------------------------------------------------------------------------
    def _handle(self, S):
        if S not in self._handles:
            dp = ctypes.POINTER(ctypes.c_double)
            weights = np.ascontiguousarray(self.weights, np.float64)
            self._handles[S] = _lib.Handle("loudness", S, self.channels, weights.ctypes.data_as(dp), self.tp_zeros, self.prototype.ctypes.data_as(dp))
        return self._handles[S]

    def run(self, x, state=None, flush=True):
        x, is_np, squeeze = self._rows(x)
        S, T = x.shape
        P, R = S // self.channels, self.tp_zeros
        data, n_in, e0 = self._check_state(state, S)
        N = n_in + T
        e1, k1 = self.emitted(N, flush)
        ne, npk = e1 - e0, k1 - e0
        n_mom, n_st = n_blocks_400ms(e1) - n_blocks_400ms(e0), n_blocks_3s(e1) - n_blocks_3s(e0)
        layout, state_len = state_layout(S, P, R, N, e1)
        parts = (("energy", (S, ne)), ("true_peak", (S, npk)), ("sample_peak", (S, npk)), ("momentary", (P, n_mom)), ("short_term", (P, n_st)),
                 ("integrated", (P, 1)))
        out_len = sum(a * b for _, (a, b) in parts)
        h = self._handle(S)
        x, xptr, code, ld, _ = _batchio.strided_rows(x)
        vp = ctypes.c_void_p

        def call(state_in, state_out, out):
            _lib.check(h.lib.frt_loudness_run(h.h, vp(xptr) if T else None, code, T, ld, vp(_batchio.ptr(state_in)), vp(_batchio.ptr(state_out)),
                                              n_in, int(bool(flush)), int(self.true_peak), vp(_batchio.ptr(out))))

        new, out = _batchio.run_call(x, is_np, lambda: (_batchio.alloc(x, (state_len,)), _batchio.alloc(x, (out_len,))), h.set_stream, call, data)
        res, at = {}, 0
        for name, (a, b) in parts:
            res[name] = out[at:at + a * b].reshape(a, b)
            at += a * b
        z3s_at, z3s_shape = layout["z3s"]
        lra = loudness_range(new[z3s_at:z3s_at + z3s_shape[0] * z3s_shape[1]].reshape(z3s_shape))
        res["integrated"] = res["integrated"][:, 0]
        tp = res["true_peak"] if self.true_peak else None
        fields = [res["momentary"], res["short_term"], res["integrated"], lra, None if tp is None else _db(tp), _db(res["sample_peak"]),
                  res["energy"], tp, res["sample_peak"]]
        if squeeze:
            fields = [None if f is None else f[0] for f in fields]
        return LoudnessResult(*fields, LoudnessState(new, S, N, k1))


def loudness(x, channels="stereo"):
    """The integrated loudness in LUFS of the recording x (LoudnessBatch(channels, true_peak=False).run(x).integrated)."""
    return LoudnessBatch(channels, true_peak=False).run(x).integrated
