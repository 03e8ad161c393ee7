"""The level meters' cases and CPU restatement, shared by oracle/golden_levels.py and the level tests: the fixture's input signals (regenerated from seeds, never
stored) and a numpy restatement of the long-level path as raw-input tap sums — the form the kernels compute
(friture_amd/csrc/levels.hip): y[n] = ((x[n-10] b10 + x[n-9] b9) + ...) + x[n] b0, elementwise IEEE operations."""
from __future__ import annotations

import numpy as np

from .cases import CHUNK, FS, chunk_ends

SUBSAMPLER_PUSHES = [0, 5, 1, 11, 3, 1000, 0, 7, 513, 2049, 10, 1, 4096, 9, 8191, 2, 333, 16384, 1, 0, 77]
IRREGULAR_CHUNKS = [512, 0, 7, 1, 10, 513, 2048, 0, 300, 4099, 1, 8192, 65, 11, 9000, 512, 0, 3, 20000, 255]
CURVE_STEPS = [("push", 40), ("setduration", 10), ("push", 20), ("setmin", -50), ("push", 20), ("setmax", -10), ("push", 20),
               ("setresptime", 1), ("push", 30), ("setresptime", 20), ("push", 40)]       # pushes in chunks of CHUNK


def sine(n, f, amp, start=0):
    t = np.arange(start, start + n) / FS
    return amp * np.sin(2 * np.pi * f * t)


def signal(name):
    """[channels, T] float64 of one fixture case."""
    if name == "noise":                    # white noise at -20 dBFS RMS
        return 0.1 * np.random.default_rng(1).standard_normal((1, 1 << 19))
    if name == "bursts":                   # 1 kHz bursts at changing levels with silences: follow, hold, decay, re-follow
        parts, pos = [], 0
        for db, secs in [(-6, 0.5), (None, 1.2), (-30, 0.4), (-12, 0.3), (None, 1.5), (-40, 0.6), (-3, 0.2), (None, 2.0),
                         (-20, 0.5)]:
            n = int(secs * FS)
            parts.append(np.zeros(n) if db is None else sine(n, 1000., 10 ** (db / 20), pos))
            pos += n
        return np.concatenate(parts)[None, :]
    if name == "impulse":                  # silence, then an impulse
        x = np.zeros((1, 2 * FS))
        x[0, FS + 123] = 1.0
        return x
    if name == "stereo":                   # unequal channels
        rng = np.random.default_rng(2)
        T = 3 * FS
        return np.stack([0.3 * rng.standard_normal(T), sine(T, 440., 0.05)])
    if name == "irregular":
        return 0.05 * np.random.default_rng(3).standard_normal((1, sum(IRREGULAR_CHUNKS)))
    if name == "subsampler":               # squared noise: the Subsampler's input in the widget
        return (0.2 * np.random.default_rng(4).standard_normal(sum(SUBSAMPLER_PUSHES))) ** 2
    if name == "curve":
        return 0.02 * np.random.default_rng(5).standard_normal((1, CHUNK * sum(v for k, v in CURVE_STEPS if k == "push")))
    raise KeyError(name)


def chunks(T, sizes=None):
    """[(start, length)] of a case: CHUNK-sample chunks (short last one), or the given sizes."""
    ends = chunk_ends(T) if sizes is None else np.cumsum(sizes)
    return [(int(e - n), int(n)) for e, n in zip(ends, np.diff(ends, prepend=0))]


def gauss(n=11, sigma=1):
    r = range(-int(n/2), int(n/2)+1)
    return [1 / (sigma * np.sqrt(2*np.pi)) * np.exp(-float(x)**2/(2*sigma**2)) for x in r]


def tapsum(b, x, tail):
    """FIR with a = [1, 0, ...] over x with the previous len(b)-1 raw inputs `tail` in front, as left-to-right tap sums."""
    L = len(b) - 1
    xp = np.concatenate([tail, x])
    n = x.shape[0]
    acc = xp[0:n] * b[L]
    for k in range(1, L + 1):
        acc = acc + xp[k:k + n] * b[L - k]
    return acc, xp[-L:].copy()


class SubsamplerCPU:
    """Subsampler.push restated: per stage tapsum then [::2] from index 0 of the push; state = last 10 raw stage inputs."""

    def __init__(self, ndec):
        self.b = np.array(gauss(11, 2.))
        self.tails = [np.zeros(10) for _ in range(ndec)]

    def push(self, x):
        if x.size == 0:
            return x
        for s in range(len(self.tails)):
            y, self.tails[s] = tapsum(self.b, x, self.tails[s])
            x = y[::2]
        return x


class LongLevelsCPU:
    """The long-level chain per complete block of 2^Ndec squared samples: subsampler, 41-tap FIR, dB."""

    def __init__(self, ndec):
        self.ndec = ndec
        self.sub = SubsamplerCPU(ndec)
        self.b41 = np.array(gauss(41, 8.))
        self.tail41 = np.zeros(40)
        self.pending = np.zeros(1 << 13)       # the samples before old_index (zeros before the stream's start), then new ones

    def push(self, x):
        """x: raw samples of channel 0; returns [(level, dB)] of the blocks consumed.  As the widget: a block is the 2^Ndec
        samples ending at old_index (data_indexed), so it is one block behind the stream."""
        self.pending = np.concatenate([self.pending, x])
        B = 1 << self.ndec
        H = 1 << 13
        nb = (self.pending.shape[0] - H) // B
        out = []
        if nb:
            u = self.sub.push(self.pending[H - B:H - B + nb * B] ** 2)
            lev, self.tail41 = tapsum(self.b41, u, self.tail41)
            for v in lev:
                out.append((v, 10. * np.log10(max(v, 1e-150))))
            self.pending = self.pending[nb * B:]
        return out
