"""What the widgets' case definitions share: the audio backend's constants and the chunk schedule of a stream."""
import numpy as np

FS = 48000              # friture/audiobackend.py: SAMPLING_RATE
CHUNK = 512             # FRAMES_PER_BUFFER


def chunk_ends(T, chunk=CHUNK):
    """The stream ends after each `chunk`-sample chunk of T samples (a short last chunk is a short chunk)."""
    return np.minimum(np.arange(1, -(-T // chunk) + 1, dtype=np.int64) * chunk, T)
