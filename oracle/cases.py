"""What the widgets' case definitions share: the audio backend's constants, the chunk schedule of a stream and seeded inputs."""
import numpy as np

FS = 48000              # friture/audiobackend.py: SAMPLING_RATE
CHUNK = 512             # FRAMES_PER_BUFFER


def chunk_ends(T, chunk=CHUNK):
    """The stream ends after each `chunk`-sample chunk of T samples (a short last chunk is a short chunk)."""
    return np.minimum(np.arange(1, -(-T // chunk) + 1, dtype=np.int64) * chunk, T)


def ragged_ends(T, seed):
    """Seeded chunk ends of T samples with chunks of 1 to 20000 samples."""
    rng = np.random.default_rng(seed)
    steps = rng.choice([1, 7, 100, 512, 512, 512, 640, 3000, 20000], size=400)
    ends = np.cumsum(steps)
    return np.concatenate([ends[ends < T], [T]]).astype(np.int64)


def synth(kind, n, seed):
    """Seeded float32 PCM: `noise`, `tone` (1 kHz plus a little noise) or `chirp` (20 Hz to 20 kHz, exponential).  The tests'
    conftest.synth, here for the recorders, which run without pytest; a test keeps the two equal."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "noise":
        x = 0.25 * rng.standard_normal(n)
    elif kind == "tone":
        x = 0.5 * np.sin(2 * np.pi * 1000.0 * t / 48000.0) + 1e-3 * rng.standard_normal(n)
    elif kind == "chirp":
        dur = n / 48000.0
        k = np.log(20000.0 / 20.0) / dur
        x = 0.5 * np.sin(2 * np.pi * 20.0 * (np.exp(k * t / 48000.0) - 1.0) / k)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)
