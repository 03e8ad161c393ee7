"""The delay estimator widget replayed in numpy from oracle.dsp as it stands (decimate_multiple, MirrorRing, gcc_phat,
delay_readout), and the seeded cases that the delay-batch tests and oracle/golden_delaybatch.py share.

replay() does what Delay_Estimator_Widget.handle_new_data does (friture/delay_estimator.py:87-176) chunk by chunk on one
two-channel stream: the windows are views of the rings and GCC-PHAT's mean removal is written back into them.
"""
from __future__ import annotations

import functools

import numpy as np

from . import dsp
from .cases import chunk_ends

NDEC, RATE = 2, 12000.0

# name -> (delay range in s, samples, seed, streams); the shapes of the GPU tests
CASES = {"r0.1": (0.1, 1 << 16, 11, 2), "r0.5": (0.5, 1 << 17, 12, 2), "r1.0": (1.0, 1 << 18, 13, 2), "r2.0": (2.0, 1 << 19, 14, 2)}
# what the reference widget is recorded on: one stream of a case, or its own ragged chunks (multiples of 4, one long push)
GOLDEN = {"r0.1": ("r0.1", 1, None), "r0.5": ("r0.5", 0, None),
          "ragged": ("r0.1", 0, [512, 1024, 1028, 4100, 4612, 44612, 45124, 60000, 65024, 65536])}


COLUMNS = ("delay_ms", "distance_m", "extremum", "correlation")


def golden_ends(name):
    case, _, ends = GOLDEN[name]
    return chunk_ends(CASES[case][1]) if ends is None else np.array(ends, np.int64)


def signal(name):
    """[S, 2, T] float64: seeded noise with a DC offset of 0.01; channel 1 is channel 0 rolled by 4 * 31 samples plus 1 % noise;
    the last stream's channel 1 has a stretch of exact zeros long enough to gate windows."""
    delayrange, T, seed, S = CASES[name]
    rng = np.random.default_rng(seed)
    x = np.empty((S, 2, T))
    for s in range(S):
        a = 0.25 * rng.standard_normal(T) + 0.01
        x[s, 0] = a
        x[s, 1] = np.roll(a, 4 * 31) + 0.0025 * rng.standard_normal(T)
    # exact zeros from the start, through the end of the third window: only from the zero state do the decimators return exact
    # zeros (their tails take thousands of samples per decade to die), so these are the windows that the reference gates
    x[S - 1, 1, :4 * 3 * int(0.5 * int(2 * delayrange * RATE))] = 0.0
    return x


def ends_with_cut(T, cut, chunk=512):
    """The ends of `chunk`-sample chunks and one more end at `cut` (a multiple of 4)."""
    return np.unique(np.concatenate([chunk_ends(T, chunk), [cut]]))


def tables():
    t = dsp.load_filter_tables()
    return np.array(t["bdec"], np.float64), np.array(t["adec"], np.float64)


def replay(x, delayrange, ends, carry=None):
    """x [2, T] float64 fed in chunks that end at `ends`.  Returns a dict: per chunk `shown` [chunks, 4] (delay_ms, distance_m,
    extremum, correlation); per window delay_ms, distance_m, extremum, correlation, gated, argmax, pct (the percentage before
    int()), margin (the two largest |smoothed| apart), xcorr and views (the effective windows [W, 2, L]); `smoothed`, `window_end`,
    `window_chunk`, `dec` [2, n] the decimated signals and `zf`; `carry` to go on from."""
    bdec, adec = tables()
    length = int(2 * delayrange * RATE)
    needed = int(0.5 * length)
    if carry is None:
        carry = dict(z=[dsp.decimate_multiple_filtic(NDEC, bdec, adec) for _ in range(2)], rings=[dsp.MirrorRing(), dsp.MirrorRing()],
                     old_index=0, old=None, shown=(0.0, 0.0, 0.0, 0))
    z, rings, old_index, old, shown = carry["z"], carry["rings"], carry["old_index"], carry["old"], carry["shown"]
    per = {k: [] for k in ("delay_ms", "distance_m", "extremum", "correlation", "gated", "argmax", "pct", "margin", "xcorr", "views",
                           "window_end", "window_chunk", "silent")}
    rows, decs, start = [], [[], []], 0
    for c, e in enumerate(np.asarray(ends).tolist()):
        for ch in range(2):
            d, z[ch] = dsp.decimate_multiple(NDEC, bdec, adec, np.ascontiguousarray(x[ch, start:e], np.float64), z[ch])
            decs[ch].append(d)
            rings[ch].push(d.reshape(1, -1))
        start = e
        available = rings[0].offset - old_index
        for _ in range(int(available / needed)):
            old_index += needed
            d0 = rings[0].data_indexed(old_index, length).reshape(-1)
            d1 = rings[1].data_indexed(old_index, length).reshape(-1)
            per["views"].append(np.stack([d0, d1]).copy())
            per["window_end"].append(old_index)
            per["window_chunk"].append(c)
            per["silent"].append(bool(d0.min() == d0.max() or d1.min() == d1.max()))      # the stream object's gate
            if np.std(d0) > 0. and np.std(d1) > 0.:
                xc, a0, a1 = dsp.gcc_phat(d0, d1)
                d0[...] = a0                                                 # the reference's in-place side effect on the ring views
                d1[...] = a1
                ro = dsp.delay_readout(xc, old, RATE, delayrange)
                old = sm = ro["smoothed"]
                top = np.sort(np.abs(sm))[-2:]
                xx = abs(sm[ro["argmax"]]) / (3 * np.std(sm))
                xx = (0.12 * ((xx > 1.0) * (xx - 1.0))) ** 3
                shown = (ro["delay_ms"], ro["distance_m"], ro["extremum"], ro["correlation_pct"])
                for k, v in (("gated", 0), ("argmax", ro["argmax"]), ("pct", xx / (1.0 + xx) * 100), ("margin", float(top[1] - top[0])),
                             ("xcorr", xc)):
                    per[k].append(v)
            else:
                shown = (0.0, 0.0, 0.0, 0)
                for k, v in (("gated", 1), ("argmax", 0), ("pct", 0.0), ("margin", np.inf), ("xcorr", np.zeros(length))):
                    per[k].append(v)
            for k, v in zip(("delay_ms", "distance_m", "extremum", "correlation"), shown):
                per[k].append(v)
        rows.append(shown)
    out = {k: np.array(v) for k, v in per.items()}
    out["shown"] = np.array(rows, np.float64).reshape(-1, 4)
    out["smoothed"] = old
    out["dec"] = np.stack([np.concatenate(d) if d else np.zeros(0) for d in decs])
    out["zf"] = np.array(z)
    out["carry"] = dict(z=z, rings=rings, old_index=old_index, old=old, shown=shown)
    return out


def doubtful(r, w):
    """A window whose correlation or arg-max the replay itself decides by less than rounding can move."""
    return bool(not r["gated"][w] and (abs(r["pct"][w] - np.round(r["pct"][w])) < 1e-6 or r["margin"][w] < 1e-9))


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """(x [S, 2, T] of `dtype`, the replay of every stream of it): computed once per session, never written to."""
    delayrange, T, _, S = CASES[name]
    x = signal(name).astype(dtype)
    x.setflags(write=False)
    return x, tuple(replay(x[s].astype(np.float64), delayrange, chunk_ends(T)) for s in range(S))
