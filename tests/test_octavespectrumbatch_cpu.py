"""OctaveSpectrumBatch without a GPU: the chunk schedule and its validation, the numpy replay the GPU tests compare against
pinned to the recording of the reference widget (tests/golden/octavespectrumbatch.npz), and the sub-block recurrence the device walks."""
import numpy as np
import pytest

from friture_amd.octavespectrum import OctaveSpectrumBatch, OctaveSpectrumState, octave_schedule
from oracle import octavespectrumbatch as H

REFERENCE_SP_MEASURED, REFERENCE_SP_BOUND = 8.3e-14, 8.3e-13
SUBBLOCK_MEASURED, SUBBLOCK_BOUND = 2.3e-15, 2.3e-14


def literal_schedule(T, chunk, pending=0):
    ends, have, t = [], pending, 0
    while True:
        need = chunk - have
        if t + need > T:
            return np.array(ends, np.int64)
        t, have = t + need, 0
        ends.append(t)


@pytest.mark.parametrize("chunk", H.LENGTHS)
def test_default_schedule_equals_a_literal_chunk_loop(chunk):
    for T in (0, 255, 256, 1024, 5000, 8192 + 768):
        for pending in (0, 100, 255):
            assert np.array_equal(octave_schedule(T, chunk, pending=pending), literal_schedule(T, chunk, pending)), (T, pending)
    # pending samples that already hold whole chunks: those chunks end before this call's first sample
    assert octave_schedule(300, 256, pending=700).tolist() == [-444, -188, 68]


def test_pending_carries_from_an_earlier_call_and_pieces_join_to_the_whole():
    batch = OctaveSpectrumBatch(3)
    T = 8192 + 768
    for chunk in H.LENGTHS:
        whole = batch.schedule(T, chunk)
        for cut in (1, 300, 1024, 4000, 8959):
            first = batch.schedule(cut, chunk)
            pending = cut - (int(first[-1]) if len(first) else 0)
            state = OctaveSpectrumState(np.zeros((1, 27)), np.zeros((1, 9, 4, 511)), np.zeros((1, pending)), pending)
            second = batch.schedule(T - cut, chunk, state=state)
            assert np.array_equal(np.concatenate([first, second + cut]), whole), (chunk, cut)
    ends = H.mixed_ends(T, 3)
    cut = int(ends[5]) + 130                                       # in the middle of chunk 6
    first, second = ends[:6], ends[6:] - cut
    assert np.array_equal(octave_schedule(cut, ends=first), first)
    assert np.array_equal(octave_schedule(T - cut, ends=second, pending=130), second)


def test_bad_chunks_and_ends_are_refused_with_index_and_length():
    for chunk in (100, 1280, 0, 384):
        with pytest.raises(ValueError, match=f"chunk {chunk}"):
            octave_schedule(4096, chunk)
    with pytest.raises(ValueError, match="chunk 1 has 100 samples"):
        octave_schedule(4096, ends=[256, 356])
    with pytest.raises(ValueError, match="chunk 0 has 1280 samples"):
        octave_schedule(4096, ends=[1280])
    with pytest.raises(ValueError, match="chunk 2 has 0 samples"):
        octave_schedule(4096, ends=[256, 512, 512])
    with pytest.raises(ValueError, match="chunk 1 has -256 samples"):
        octave_schedule(4096, ends=[512, 256])                    # unsorted
    with pytest.raises(ValueError, match="end 4352 beyond the 4096 samples"):
        octave_schedule(4096, ends=np.arange(256, 4353, 256))
    with pytest.raises(ValueError, match="chunk 0 has 356 samples"):
        octave_schedule(4096, ends=[256], pending=100)
    with pytest.raises(Exception, match="Unknown bandsperoctave"):
        OctaveSpectrumBatch(5)


def test_settings_are_the_widgets():
    from oracle import dsp
    for bpo in (1, 3, 6):
        batch = OctaveSpectrumBatch(bpo, weighting=2, response_time=0.125)
        alphas, _ = dsp.band_smoothing_setup(bpo, 0.125)
        assert np.array_equal(batch.alphas, alphas) and np.array_equal(batch.w, H.band_weight(bpo, 2))
        fi, flow, fhigh = dsp.octave_frequencies(9 * bpo, bpo)
        assert np.array_equal(batch.flow, flow) and np.array_equal(batch.fhigh, fhigh) and len(batch.f_nominal) == 9 * bpo


def test_walking_subblocks_and_emitting_at_chunk_ends_equals_the_per_chunk_formula():
    """sp = E_b + sp (1 - alpha)^(256 / dec) over a chunk's 256-sample sub-blocks against exp_smoothed_value over the chunk:
    the largest relative difference in sp measured here is 2.3e-15 (a few ulp); asserted with one decade over it, 2.3e-14."""
    worst = 0.0
    for bpo in (1, 3):
        x = H.sweep(16384, 5).astype(np.float64)
        ends = H.mixed_ends(len(x), 9)
        assert set(np.diff(ends, prepend=0).tolist()) == set(H.LENGTHS)
        a, b = H.replay(x, ends, bpo), H.replay(x, ends, bpo, subblocks=True)
        worst = max(worst, float(np.max(np.abs(a["energy"] - b["energy"]) / a["energy"])))
    print(f"sub-block walk against the per-chunk formula: {worst:.3e} (measured {SUBBLOCK_MEASURED}, bound {SUBBLOCK_BOUND})")
    assert worst <= SUBBLOCK_BOUND


@pytest.mark.parametrize("bpo", [1, 3])
@pytest.mark.parametrize("weighting", [0, 1])
def test_replay_equals_the_reference_widget_fed_the_same_chunks(golden, bpo, weighting):
    """The replay against what OctaveSpectrum_Widget.handle_new_data (friture/octavespectrum.py:91-122) left in dispbuffers and
    handed to setdata, chunk by chunk (oracle/golden_octavespectrumbatch.py), chunk lengths mixed from {256, 512, 768, 1024}.
    Both sides are the same numpy operations on tables that agree to rounding: the largest relative difference in sp measured
    here is 8.3e-14; asserted with one decade over it, 8.3e-13.  dB: 1e-11 absolute (10 / ln 10 times the relative bound,
    rounded up)."""
    g = golden("octavespectrumbatch")
    assert (bpo, weighting) in H.GOLDEN_CASES
    x, ends = H.golden_input(), H.golden_ends()
    assert np.array_equal(x, H.sweep(16384, 5).astype(np.float64)) and np.array_equal(ends, H.mixed_ends(len(x), 9))
    assert np.array_equal(ends, g["ends"])
    shown, sps = g[f"bpo{bpo}_w{weighting}_db"], g[f"bpo{bpo}_w{weighting}_sp"]
    mine = H.WidgetReplay(bpo, weighting)
    start, worst = 0, 0.0
    for c, e in enumerate(ends.tolist()):
        sp, db = mine.push(x[start:e])
        start = e
        want = sps[c]
        assert np.all(want > 0)
        worst = max(worst, float(np.max(np.abs(sp - want) / want)))
        assert np.max(np.abs(db - shown[c])) <= 1e-11
    print(f"replay against the reference widget, sp: {worst:.3e} (measured {REFERENCE_SP_MEASURED}, bound {REFERENCE_SP_BOUND})")
    assert len(shown) == len(ends) and worst <= REFERENCE_SP_BOUND
