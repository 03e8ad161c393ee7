"""numpy replay of the pitch tracker widget's chain (PitchTrackerWidget.handle_new_data / update_curve, friture/pitch_tracker.py:
109-119, around PitchTracker.update / new_frames / estimate_pitch, :312-428), driven chunk by chunk as the widget is: the
candidate of oracle.dsp on row 0 of every frame, the level over ALL rows of the frame (:407), oracle.dsp.PitchGate, the
estimate ring (friture_amd.ringbuffer.RingBuffer, as out_buf) and the OctaveC axis of coordinateTransform.py:73-83 with length 1
and borders 0.  The frames are cut from the true samples: what the reference's input ring hands out while chunk + fft_size stays
within its 10000 samples.  Shared by the PitchBatch tests and their recorder (oracle/golden_pitchbatch.py), which pins this
replay to the reference's PitchTracker in tests/golden/pitchbatch.npz.  Nothing here touches the GPU.
"""
import functools
import math

import numpy as np

from friture_amd.ringbuffer import RingBuffer

from . import dsp
from .cases import chunk_ends

EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def tables(sample_rate=48000, min_freq=65, max_freq=1047, cres=10):
    return dsp.swipe_tables(sample_rate, min_freq, max_freq, cres)


def axis_curve(pitches, min_freq=65, max_freq=1047):
    """update_curve, :114-117: 1 - toScreen(pitches) on the OctaveC scale (log2(fmax(x, 1e-20))), clipped to [0, 1]."""
    trans = np.log2(np.fmax(np.asarray(pitches, np.float64), 1e-20))
    trans_min, trans_max = np.log2(float(min_freq)), np.log2(float(max_freq))
    return np.clip(1.0 - ((trans - trans_min) * 1.0 / (trans_max - trans_min) + 0.0), 0, 1)


def level_db(frame):
    """dBFS of a [rows, N] (or [N]) frame: the RMS over every row (:407-408)."""
    return float(20 * np.log10(np.sqrt(np.mean(np.asarray(frame, np.float64) ** 2)) + EPS))


class WidgetReplay:
    """One stream.  push(chunk [rows, n]) is AudioBuffer.push + handle_new_data; the lists hold what each call left."""

    def __init__(self, fft_size=4096, overlap=0.75, sample_rate=48000, min_freq=65, max_freq=1047, min_db=-50.0, cres=10, conf=0.5,
                 p_delta=2, duration=10):
        self.fft_size, self.sample_rate, self.min_freq, self.max_freq, self.duration = fft_size, sample_rate, min_freq, max_freq, duration
        self.step = math.floor(fft_size * (1.0 - overlap))
        self.freqs, self.kernels = tables(sample_rate, min_freq, max_freq, cres)
        self.window = dsp.hann_symmetric(fft_size)
        self.gate = dsp.PitchGate(min_db, conf, p_delta)
        self.samples = None                     # every sample pushed so far, [rows, offset]
        self.next_in_offset = 0                 # set_buffer pins it to the ring's offset: 0 for a fresh stream
        self.out_buf = RingBuffer()
        self.out_offset = self.out_buf.offset
        self.estimates, self.raw, self.row0_db = [], [], []
        self.chunks = 0
        self.frame_start, self.refresh_chunk, self.pitch, self.curves = [0], [], [], []

    @property
    def n_history(self):
        return math.floor(self.duration / (self.step / self.sample_rate)) + 1           # get_estimates, :318-321

    def get_estimates(self):
        return self.out_buf.data_indexed(self.out_offset, self.n_history)[0, :]

    def curve(self):
        return axis_curve(self.get_estimates(), self.min_freq, self.max_freq)

    def push(self, chunk):
        chunk = np.atleast_2d(np.asarray(chunk, np.float64))
        self.samples = chunk if self.samples is None else np.concatenate([self.samples, chunk], axis=1)
        new = []
        while self.next_in_offset + self.fft_size <= self.samples.shape[1]:             # new_frames, :326-332
            frame = self.samples[:, self.next_in_offset:self.next_in_offset + self.fft_size]
            f0, confidence, db0 = dsp.pitch_candidate(frame[0], self.window, self.freqs, self.kernels, self.sample_rate)
            db = level_db(frame)
            new.append(self.gate.step(f0, confidence, db))
            self.raw.append((f0, confidence, db))
            self.row0_db.append(db0)
            self.next_in_offset += self.step
        self.out_buf.push(np.array([new], np.float64).reshape(1, len(new)), 0)          # update, :312-316
        self.out_offset = self.out_buf.offset
        self.estimates += new
        if new:                                                                         # handle_new_data, :109-112
            self.frame_start.append(len(self.estimates))
            self.refresh_chunk.append(self.chunks)
            self.curves.append(self.curve().copy())
            self.pitch.append(self.out_buf.data_indexed(self.out_offset, 1)[0, 0])
        self.chunks += 1
        return bool(new)


def replay(x, ends, **settings):
    """x: [rows, T] (or [T]) of one stream fed as the chunks that end at `ends` -> dict of arrays."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    w = WidgetReplay(**settings)
    start = 0
    for e in np.asarray(ends, np.int64).tolist():
        w.push(x[:, start:e])
        start = e
    M = w.n_history
    return {"estimates": np.array(w.estimates, np.float64), "raw": np.array(w.raw, np.float64).reshape(-1, 3).T,
            "row0_db": np.array(w.row0_db, np.float64), "frame_start": np.array(w.frame_start, np.int64),
            "refresh_chunk": np.array(w.refresh_chunk, np.int64), "pitch": np.array(w.pitch, np.float64),
            "curves": np.array(w.curves, np.float64).reshape(-1, M), "last_curve": w.curve().copy(), "n_history": M}


def close(a, b, tol):
    """The voiced pattern identical, the rest within tol relative (absolute below 1): tests/test_pitch_gpu.py's rule."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return bool(np.all(np.abs(a[m] - b[m]) <= tol * np.maximum(1.0, np.abs(b[m]))))


def tone(n, f0, dbfs, seed, partials=(1.0, 0.5), noise_db=-90.0, fs=48000.0):
    """A seeded harmonic tone of the given RMS level with a little noise, float64."""
    t = np.arange(n)
    x = sum(a * np.sin(2 * np.pi * f0 * (h + 1) * t / fs) for h, a in enumerate(partials))
    x = x / np.sqrt(np.mean(x ** 2)) * 10 ** (dbfs / 20)
    return x + 10 ** (noise_db / 20) * np.random.default_rng(seed).standard_normal(n)


def dual_inputs(n):
    """The two inputs a level from row 0 alone gets wrong (tests/test_pitchbatch_gpu.py; the margins: tests/test_pitchbatch_cpu.py): [2, rows, n]."""
    loud = tone(n, 330.0, -20.0, 11, partials=(1.0,), noise_db=-32.0)
    one = np.stack([tone(n, 220.0, -56.0, 12), loud])               # pooled above min_db: voiced
    two = np.stack([tone(n, 220.0, -48.5, 13), np.zeros(n)])        # pooled below min_db: unvoiced
    return np.stack([one, two])


def ragged(T, seed, largest=3000):
    rng = np.random.default_rng(seed)
    ends = np.unique(np.concatenate([np.cumsum(rng.integers(0, largest, 4 * T // largest + 8)), [T]]))
    return ends[ends <= T]


# ---- what tests/golden/pitchbatch.npz records: the reference's PitchTracker behind a reference RingBuffer, chunk by chunk --------

GOLDEN_SETTINGS = dict(fft_size=1024, overlap=0.75, duration=0.1)
GOLDEN_CHUNKINGS = {"chunk512": lambda T: chunk_ends(T, 512), "ragged": lambda T: ragged(T, 5, largest=2500)}
GOLDEN_KEYS = {"steady220": "N1024_steady220_x", "jump": "N1024_jump_x", "quiet": "N1024_quiet_x"}      # inputs that lie in pitch.npz


def golden_inputs(pitch_npz):
    """{case: x [rows, n] float64}: the three one-row cases are arrays of pitch.npz (GOLDEN_KEYS), the three two-row cases stand
    `jump` beside a seeded tone and take the two dual_inputs."""
    one = {name: pitch_npz[key].astype(np.float64)[None] for name, key in GOLDEN_KEYS.items()}
    n = one["jump"].shape[1]
    return {**one, "jump_tone": np.stack([one["jump"][0], tone(n, 330.0, -30.0, 21)]), "dual_one": dual_inputs(n)[0],
            "dual_two": dual_inputs(n)[1]}
