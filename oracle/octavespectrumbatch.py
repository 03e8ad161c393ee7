"""What the OctaveSpectrumBatch tests and their recorder (oracle/golden_octavespectrumbatch.py) share: a numpy replay of the
octave-spectrum widget's chain (oracle.dsp: OlaBank, band_smoothing_setup, band_energies, band_db) fed chunk by chunk at given ends with a carried state, the same chain walked in
256-sample sub-blocks, and seeded inputs.  tests/golden/octavespectrumbatch.npz pins the replay to the reference widget.  Nothing
here touches the GPU."""
import functools

import numpy as np

from . import dsp
from .cases import synth

LENGTHS = (256, 512, 768, 1024)
GOLDEN_CASES = [(bpo, weighting) for bpo in (1, 3) for weighting in (0, 1)]      # on golden_input(), chunks at golden_ends()


def sweep(n, seed):
    """Seeded float32 PCM: a 20 Hz - 20 kHz sine sweep plus noise at amplitude 0.25, so that every octave responds."""
    return (0.5 * synth("chirp", n, seed) + synth("noise", n, seed)).astype(np.float32)


def golden_input():
    return sweep(16384, 5).astype(np.float64)


def golden_ends():
    return mixed_ends(16384, 9)


def streams(S, n, seed):
    return np.stack([sweep(n, seed + s) for s in range(S)])


def mixed_ends(T, seed, pending=0):
    """Chunk ends from a seeded draw over {256, 512, 768, 1024}, counted from -pending, the last one before T."""
    ends = np.cumsum(np.random.default_rng(seed).choice(LENGTHS, size=(T + pending) // 256 + 1)) - pending
    return ends[ends < T].astype(np.int64)


def band_weight(bpo, weighting):
    fi, _, _ = dsp.octave_frequencies(dsp.NOCTAVE * bpo, bpo)
    A, B, C = dsp.band_weighting(fi)
    return {0: np.zeros(len(fi)), 1: A, 2: B}.get(weighting, C)


class WidgetReplay:
    """One widget: Octave_Filters.filter, the per-band smoothing of y^2 and the dB read-out of every chunk it is pushed."""

    def __init__(self, bpo=3, weighting=1, response_time=1.0):
        self.bank = dsp.OlaBank(bpo)
        self.alphas, self.kernels = dsp.band_smoothing_setup(bpo, response_time)
        self.decs = dsp.get_decs(bpo)
        self.w = band_weight(bpo, weighting)
        self.sp = [0.0] * (dsp.NOCTAVE * bpo)

    def push(self, chunk):
        y, _ = self.bank.filter(np.asarray(chunk, np.float64))
        self.sp = dsp.band_energies(y, self.kernels, self.alphas, self.sp)
        return np.array(self.sp), dsp.band_db(self.sp, self.w)

    def push_subblocks(self, chunk):
        """The same chunk with the smoothing walked over its 256-sample sub-blocks: sp = E_b + sp (1 - alpha)^m, m = 256 / dec,
        E_b = alpha sum_i (1 - alpha)^(m-1-i) y_i^2 (what the device computes)."""
        y, _ = self.bank.filter(np.asarray(chunk, np.float64))
        assert len(chunk) % 256 == 0
        for k, (band, kernel, alpha, dec) in enumerate(zip(y, self.kernels, self.alphas, self.decs)):
            m = 256 // dec
            for b in range(len(chunk) // 256):
                e = alpha * np.dot(kernel[len(kernel) - m:], band[b * m:(b + 1) * m] ** 2)
                self.sp[k] = float(e + self.sp[k] * (1.0 - alpha) ** m)
        return np.array(self.sp), dsp.band_db(self.sp, self.w)


def replay(x, ends, bpo=3, weighting=1, response_time=1.0, pending=0, widgets=None, subblocks=False):
    """dict(energy [S, R, 9 bpo], db [S, R, 9 bpo], widgets) of the streams x [S, T] (float64 of what the device is given) whose
    chunks end at `ends`, counted from -pending; `widgets`: the carried replays of an earlier call."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    widgets = widgets or [WidgetReplay(bpo, weighting, response_time) for _ in range(x.shape[0])]
    nb = dsp.NOCTAVE * bpo
    energy, db = np.empty((x.shape[0], len(ends), nb)), np.empty((x.shape[0], len(ends), nb))
    for s, widget in enumerate(widgets):
        start = -pending
        for r, e in enumerate(np.asarray(ends).tolist()):
            push = widget.push_subblocks if subblocks else widget.push
            energy[s, r], db[s, r] = push(x[s, start + pending:e + pending])
            start = e
    return dict(energy=energy, db=db, widgets=widgets)


@functools.lru_cache(maxsize=None)
def case(S, T, bpo, weighting, seed, chunk=None):
    """(x float32 [S, T], ends, replay of the float64 of x): computed once, shared, left unchanged."""
    x = streams(S, T, seed)
    ends = mixed_ends(T, seed + 100) if chunk is None else np.arange(chunk, T + 1, chunk, dtype=np.int64)
    ref = replay(x.astype(np.float64), ends, bpo, weighting)
    for a in (ends, ref["energy"], ref["db"]):
        a.setflags(write=False)
    return x, ends, ref


def energy_close(got, want):
    """The bank's own bar (tests/test_ola_gpu.py, measured agreement 1e-12): |got - want| <= 1e-10 want + 1e-20 max(want) per
    refresh; returns the largest |got - want| / (1e-10 want + 1e-20 max) seen (<= 1 passes)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    bound = 1e-10 * want + 1e-20 * want.max(axis=-1, keepdims=True)
    return float(np.max(np.abs(got - want) / bound))


def db_of(energy, w):
    return 10 * np.log10(np.asarray(energy) + 1e-30) + w
