"""Shared by the SpectrumBatch tests and tools/bench_spectrumbatch.py: the spectrum widget's body replayed with the oracle (the loop of
test_widgets_gpu.test_spectrum_analyzer_stream, over streams, dual channels and ragged chunk ends, every refresh kept), seeded
inputs, and the check that an oracle result decides its own arg-max indices."""
from __future__ import annotations

import numpy as np

from . import dsp
from .cases import FS, chunk_ends

NK = 8192


def settings(fft_size, overlap, weighting, response_time):
    """(hop, needed, alpha, kernel, weight, freq) as Spectrum_Widget sets them (friture/spectrum.py:196-222, audioproc.py:86-96)."""
    needed = fft_size * (1. - overlap)
    n = response_time * FS / (fft_size * (1. - overlap))
    alpha = 1. - (1. - 0.65) ** (1. / (n + 1))
    freq = dsp.frequency_axis(fft_size)
    curves = dsp.weighting_curves(freq)
    weight = np.zeros(freq.shape) if weighting == 0 else curves[min(weighting, 3) - 1]
    return int(needed), needed, alpha, dsp.smoothing_kernel(alpha, NK), weight, freq


def replay_schedule(fft_size, overlap, ends, pending=0):
    """The widget's bookkeeping alone: (frames per refresh, chunk index of every refresh), old_index starting `pending` samples
    behind the first sample."""
    needed = fft_size * (1. - overlap)
    hop = int(needed)
    old_index, frames, chunks = -pending, [], []
    for c, e in enumerate(ends):
        available = int(e) - old_index
        realizable = int(np.floor(available / needed))
        if realizable > 0:
            frames.append(realizable)
            chunks.append(c)
            old_index += realizable * hop
    return frames, chunks


def readouts(spn_rows, kernel, alpha, previous, weight, freq):
    """One refresh of one stream: spn_rows is [(bins, frames)] per row, previous [rows][bins].  Returns (smoothed [rows, B], last)
    with `last` the read-out the widget shows (dual: the ratio against row 0's smoothed spectrum, pitch from row 0)."""
    first = dsp.spectrum_readout(spn_rows[0], kernel, alpha, previous[0], weight, freq)
    if len(spn_rows) == 1:
        return first["smoothed"][None], first
    second = dsp.spectrum_readout(spn_rows[1], kernel, alpha, previous[1], None, freq, ref_smoothed=first["smoothed"])
    return np.stack([first["smoothed"], second["smoothed"]]), second


def _collect(per_stream, refresh_chunk, freq):
    keys = ("db", "smoothed", "peak_index", "pitch_index", "fmax", "fpitch")
    out = {k: np.array([[r[k] for r in rs] for rs in per_stream]) for k in keys}
    B = len(freq)
    if not len(refresh_chunk):
        out["db"], out["smoothed"] = out["db"].reshape(len(per_stream), 0, B), out["smoothed"].reshape(len(per_stream), 0, 1, B)
    out["refresh_chunk"] = np.array(refresh_chunk, np.int64)
    return out


def replay(x, fft_size=8192, overlap=0.75, weighting=1, response_time=0.025, chunk=512, ends=None):
    """x: [S, rows, T] float64 (rows 1, or 2 for dual channels).  Every stream through the widget's frame loop
    (dsp.widget_frames) -> psd_frame -> spectrum_readout chunk by chunk.  Returns dict(db [S, R, B], smoothed [S, R, rows, B],
    peak_index, pitch_index, fmax, fpitch [S, R], refresh_chunk [R])."""
    x = np.asarray(x, np.float64)
    S, rows, T = x.shape
    _, needed, alpha, kernel, weight, freq = settings(fft_size, overlap, weighting, response_time)
    ends = chunk_ends(T, chunk) if ends is None else np.asarray(ends, np.int64)
    window = dsp.hann_symmetric(fft_size)
    per_stream, refresh_chunk = [], []
    for s in range(S):
        prev = np.zeros((rows, len(freq)))
        got, chunks = [], []
        for c, frames in dsp.widget_frames(x[s], ends, fft_size, needed):
            spn = [np.stack([dsp.psd_frame(f[r], window) for f in frames], axis=1) for r in range(rows)]
            prev, last = readouts(spn, kernel, alpha, prev, weight, freq)
            got.append(dict(last, smoothed=prev))
            chunks.append(c)
        per_stream.append(got)
        refresh_chunk = chunks
    return _collect(per_stream, refresh_chunk, freq)


def readout_loop(psd, frame_start, kernel, alpha, previous, weight, freq):
    """The kernel's contract on given PSD frames: psd [S, rows, F, B], previous [S, rows, B]; a loop of dsp.spectrum_readout over
    the refresh table.  Same dict as replay(), plus `state` [S, rows, B]."""
    S, rows, F, B = psd.shape
    per_stream, state = [], np.array(previous, np.float64, copy=True)
    for s in range(S):
        got = []
        for r in range(len(frame_start) - 1):
            a, b = int(frame_start[r]), int(frame_start[r + 1])
            state[s], last = readouts([np.asarray(psd[s, q, a:b], np.float64).T for q in range(rows)], kernel, alpha, state[s],
                                      weight, freq)
            got.append(dict(last, smoothed=state[s].copy()))
        per_stream.append(got)
    out = _collect(per_stream, list(range(len(frame_start) - 1)), freq)
    out["state"] = state
    return out


def assert_decisive(ref):
    """On the oracle's values alone: every refresh of every stream decides its two indices by a margin far above the 1e-8 dB of
    the end-to-end comparison.  A signal refresh: the top two dB values differ by more than 1e-6 dB and the top two harmonic
    products by more than 1e-6 relative.  A silent refresh (every smoothed row all zero): dB is the same constant plus the
    weighting on both sides, so the top two differ by more than 1e-10 dB or are exactly equal (the first index wins), and the
    harmonic product is all zeros (index 0).  No refresh is left out."""
    db, sm = ref["db"], ref["smoothed"]
    S, R, B = db.shape
    for s in range(S):
        for r in range(R):
            top = np.sort(db[s, r])[-2:]
            gap = top[1] - top[0]
            if not np.any(sm[s, r]):
                assert gap > 1e-10 or gap == 0.0, (s, r, gap)
                assert ref["pitch_index"][s, r] == 0
                continue
            assert gap > 1e-6, ("dB", s, r, gap)
            hps = np.sort(dsp.harmonic_product_spectrum(sm[s, r, 0]))[-2:]
            assert hps[1] > 0 and (hps[1] - hps[0]) > 1e-6 * hps[1], ("hps", s, r, hps)


# ---- inputs (float32 PCM, as captured audio) ----------------------------------------------------------------------------------

def sine_noise(T, seed, f=440.0):
    """A sine plus noise 40 dB below it."""
    rng = np.random.default_rng(seed)
    return (0.5 * np.sin(2 * np.pi * f * np.arange(T) / FS) + 0.005 * rng.standard_normal(T)).astype(np.float32)


def two_tone(T, seed):
    """Two tones plus noise 40 dB below the weaker one.  The noise floor is part of the input on purpose: the float64 transform
    differs from pocketfft by about 1e-16 of a frame's largest bin amplitude (test_widgets_gpu.test_spectrogram_chain), so a bin
    150 dB below the tones, as between two float32-quantised pure tones, moves by 2 * 1e-16 * 10^(150 / 20) * 4.34 = 2.7e-8 dB, above
    the chain's 1e-8 dB tolerance for a reason that lies in the transform and not in what is tested here."""
    rng = np.random.default_rng(seed)
    f1, f2 = 300.0 + 50.0 * rng.random(), 1900.0 + 200.0 * rng.random()
    t = np.arange(T) / FS
    tones = 0.4 * np.sin(2 * np.pi * f1 * t) + 0.25 * np.sin(2 * np.pi * f2 * t + 1.0)
    return (tones + 0.0025 * rng.standard_normal(T)).astype(np.float32)


def silence(T, seed=0):
    return np.zeros(T, np.float32)


def half_silent(T, seed):
    x = sine_noise(T, seed, 660.0)
    x[:T // 2] = 0
    return x


MAKERS = [sine_noise, two_tone, silence, half_silent]


def streams(S, rows, T, seed=0):
    """[S, rows, T] float32: stream s is MAKERS[s % 4]; the second row of a dual stream is the same kind from another seed (a
    silent stream is silent on both rows, so that its refreshes are silent refreshes)."""
    return np.stack([np.stack([MAKERS[s % 4](T, seed + 10 * s + 5 * q) for q in range(rows)]) for s in range(S)])
