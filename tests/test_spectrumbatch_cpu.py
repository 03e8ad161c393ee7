"""SpectrumBatch without a GPU: the refresh schedule against the widget's bookkeeping replayed, the oracle replay's own
properties the GPU tests lean on, and the new entry point in the header, the ctypes table and the library."""
import numpy as np
import pytest

from oracle import spectrumbatch as H
from oracle.cases import ragged_ends as _ragged
from friture_amd.spectrum import SpectrumBatch, SpectrumState


def _check(sb, T, ends, pending):
    state = None if not pending else SpectrumState(None, None, pending)
    fs, rc = sb.schedule(T, ends=ends, state=state)
    frames, chunks = H.replay_schedule(sb.fft_size, sb.overlap, ends, pending)
    assert fs.dtype == np.int64 and rc.dtype == np.int64 and fs[0] == 0
    assert np.diff(fs).tolist() == frames and rc.tolist() == chunks
    return fs, rc


@pytest.mark.parametrize("fft_size", [32, 1024, 8192, 16384])
@pytest.mark.parametrize("overlap", [0.75, 0.5, 0.0])
def test_schedule_equals_the_widgets_bookkeeping(fft_size, overlap):
    sb = SpectrumBatch(fft_size, overlap)
    assert sb.hop == int(fft_size * (1. - overlap))
    T = 100000
    fs, rc = sb.schedule(T)                                          # 512-sample chunks, a short last one
    frames, chunks = H.replay_schedule(fft_size, overlap, H.chunk_ends(T, 512))
    assert np.diff(fs).tolist() == frames and rc.tolist() == chunks and len(chunks) > 0
    assert fs[-1] == T // sb.hop                                     # every frame ending at or before the last sample, frame 0 included
    _check(sb, T, H.chunk_ends(T, 5 * sb.hop + 3), 0)                # one chunk larger than several hops
    _check(sb, T, _ragged(T, fft_size), 0)
    for pending in (1, sb.hop - 1, sb.hop + 700):                    # carried in from an earlier call
        _check(sb, T, _ragged(T, fft_size + pending), pending)
    fs1, rc1 = sb.schedule(T, ends=[T])                              # the whole recording as one chunk: one refresh
    assert fs1.tolist() == [0, T // sb.hop] and rc1.tolist() == [0]
    assert sb.schedule(0)[0].tolist() == [0] and sb.schedule(0)[1].size == 0


def test_schedule_rejects_bad_ends():
    sb = SpectrumBatch(1024)
    for ends in ([600, 500], [-1], [1001]):
        with pytest.raises(ValueError):
            sb.schedule(1000, ends=ends)


@pytest.mark.parametrize("fft_size,overlap", [(32, 0.75), (1024, 0.75), (8192, 0.5), (1024, 0.0)])
def test_schedule_of_a_whole_equals_its_halves_with_the_state_carried(fft_size, overlap):
    sb = SpectrumBatch(fft_size, overlap)
    T = 512 * 90
    fs, rc = sb.schedule(T)
    for c in (512, 512 * 3, 512 * 44, 512 * 89):
        fa, ra = sb.schedule(c)
        pending = c - int(fa[-1]) * sb.hop                           # offset - old_index after the first half
        fb, rb = sb.schedule(T - c, state=SpectrumState(None, None, pending))
        assert np.array_equal(np.concatenate([fa, fb[1:] + fa[-1]]), fs)
        assert np.array_equal(np.concatenate([ra, rb + c // 512]), rc)


def test_replay_first_refresh_is_the_all_zero_frame_and_decides_its_indices():
    """Frame 0 ends at sample 0: fed one hop per chunk, a fresh widget's first refresh holds only zeros, whatever the input
    (reference behaviour)."""
    x = H.streams(4, 1, 256 * 24, seed=3).astype(np.float64)
    ref = H.replay(x, fft_size=1024, weighting=1, chunk=256)
    w = H.settings(1024, 0.75, 1, 0.025)[4]
    assert ref["refresh_chunk"][0] == 0 and not np.any(ref["smoothed"][:, 0])
    assert np.array_equal(ref["db"][:, 0], np.broadcast_to(10 * np.log10(1e-30) + w, (4, 513)))
    assert 10 * np.log10(1e-30) == -300.0
    assert np.all(ref["peak_index"][:, 0] == np.argmax(w)) and np.all(ref["pitch_index"][:, 0] == 0)
    H.assert_decisive(ref)
    assert np.all(ref["peak_index"][2] == np.argmax(w))              # the silent stream stays silent
    sb = SpectrumBatch(1024)
    assert np.array_equal(sb.schedule(256 * 24, chunk=256)[1], ref["refresh_chunk"])
    assert sb.alpha == H.settings(1024, 0.75, 1, 0.025)[2] and np.array_equal(sb.kernel, H.settings(1024, 0.75, 1, 0.025)[3])
    assert np.array_equal(sb.freq, H.settings(1024, 0.75, 1, 0.025)[5])


def test_entry_point_is_in_header_table_and_library():
    from friture_amd import _lib
    header = (_lib.LIB_PATH.parents[2] / "include" / "friture_hip.h").read_text()
    assert "int frt_spectrum_batch(" in header and "frt_spectrum_batch" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "frt_spectrum_batch")
