"""SpectrogramBatch without a GPU: the numpy replay of the widget chain against tests/golden/spectrogrambatch/
(recorded from the reference classes by oracle/golden_spectrogrambatch.py), the frame schedule and the column table against
the recorded tables, and the new entry point in the header, the ctypes table and the library."""
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from conftest import synth
from oracle import spectrogrambatch as H
from oracle import spectrumbatch as SH
from oracle.cases import chunk_ends
from oracle.cases import ragged_ends as _ragged
from friture_amd.plotting import frequency_scales as fscales
from friture_amd.spectrogram import SpectrogramBatch, SpectrogramState
from friture_amd.spectrum import SpectrumBatch, SpectrumState

GOLDEN = Path(__file__).resolve().parent / "golden" / "spectrogrambatch"
SCALES = {"linear": fscales.Linear, "log": fscales.Logarithmic, "mel": fscales.Mel, "erb": fscales.Erb, "octave": fscales.Octave}


@pytest.fixture(scope="module")
def gold():
    return H.load_golden(GOLDEN)


def batch_of(case):
    keys = ("fft_size", "overlap", "spec_min", "spec_max", "weighting", "minfreq", "maxfreq", "screen_width", "screen_height", "timerange_s")
    return SpectrogramBatch(scale=SCALES[case["scale"]], **{k: case[k] for k in keys})


@pytest.mark.parametrize("name", list(H.GOLDEN_CASES))
def test_replay_reproduces_the_reference(gold, name):
    """The restatement the GPU tests compare with is the reference: pixels, normalised frames and the column table, exactly."""
    case = H.GOLDEN_CASES[name]
    g = gold[name]
    st = H.settings(**case)
    assert np.array_equal(H.synth(case["kind"], case["n"], case["seed"]), g["x"]) and np.array_equal(H.case_ends(case), g["ends"])
    assert np.array_equal(st["targets"], g["targets"]) and np.array_equal(st["weight"], g["weight"]) and np.array_equal(st["lut"], g["lut"])
    ref = H.replay(g["x"], g["ends"], st)
    for k in ("norm", "frame_start", "refresh_chunk", "pixels", "src", "a", "filler", "column_refresh"):
        assert ref[k].shape == g[k].shape and np.array_equal(ref[k], g[k]), k
    assert ref["pixels"].dtype == np.uint32 and ref["pixels"].shape[1] > 0


def test_the_golden_cases_cover_what_they_are_there_for(gold):
    assert H.settings(**H.GOLDEN_CASES["thirds_1000"])["needed"] != int(H.settings(**H.GOLDEN_CASES["thirds_1000"])["needed"])
    assert H.settings(**H.GOLDEN_CASES["chirp_1024"])["ratio"] > 1 > H.settings(**H.GOLDEN_CASES["up_512"])["ratio"]
    thirds = gold["thirds_1000"]
    assert thirds["filler"].sum() == 1 and not gold["chirp_1024"]["filler"].any() and not gold["up_512"]["filler"].any()
    f = int(np.argmax(thirds["filler"]))
    assert np.all(thirds["pixels"][:, f] == thirds["lut"][0])                   # np.zeros through the colour transform
    assert np.any(np.diff(gold["up_512"]["ends"]) != 512)                       # ragged chunks
    assert gold["chirp_1024"]["pixels"].shape[1] >= 9


@pytest.mark.parametrize("name", list(H.GOLDEN_CASES))
def test_schedule_and_columns_reproduce_the_recorded_tables(gold, name):
    case = H.GOLDEN_CASES[name]
    g = gold[name]
    sb = batch_of(case)
    st = H.settings(**case)
    assert sb.hop == st["hop"] and sb.needed == st["needed"] and sb.ratio == st["ratio"]
    assert np.array_equal(sb.freq, st["freq"]) and np.array_equal(sb.w, st["weight"]) and np.array_equal(sb.targets, g["targets"])
    assert np.array_equal(sb.lut, g["lut"])
    fs, rc = sb.schedule(case["n"], ends=g["ends"])
    assert np.array_equal(fs, g["frame_start"]) and np.array_equal(rc, g["refresh_chunk"])
    if case["chunk"] is not None:
        assert all(np.array_equal(a, b) for a, b in zip(sb.schedule(case["n"], chunk=case["chunk"]), (fs, rc)))
    t = sb.columns(case["n"], ends=g["ends"])
    assert t.src.dtype == np.int64 and t.a.dtype == np.float64 and t.filler.dtype == bool and t.column_refresh.dtype == np.int64
    assert np.array_equal(t.filler, g["filler"]) and np.array_equal(t.column_refresh, g["column_refresh"])
    live = ~g["filler"]
    assert np.array_equal(t.src[live], g["src"][live]) and np.array_equal(t.a[live], g["a"][live])
    # a carried state: the recording cut at every chunk end gives the same tables
    for c in range(0, len(g["ends"]) - 1, max(1, len(g["ends"]) // 7)):
        cut = int(g["ends"][c])
        fa, ra = sb.schedule(cut, ends=g["ends"][:c + 1])
        ta = sb.columns(cut, ends=g["ends"][:c + 1])
        carried = SpectrogramState(None, cut - int(fa[-1]) * sb.hop, None, ta.orig_index, ta.resampled_index)
        fb, rb = sb.schedule(case["n"] - cut, ends=g["ends"][c + 1:] - cut, state=carried)
        tb = sb.columns(case["n"] - cut, ends=g["ends"][c + 1:] - cut, state=carried)
        assert np.array_equal(np.concatenate([fa, fb[1:] + fa[-1]]), fs) and np.array_equal(np.concatenate([ra, rb + c + 1]), rc)
        assert np.array_equal(np.concatenate([ta.src, tb.src + fa[-1]]), t.src) and np.array_equal(np.concatenate([ta.a, tb.a]), t.a)
        assert np.array_equal(np.concatenate([ta.filler, tb.filler]), t.filler)
        assert np.array_equal(np.concatenate([ta.column_refresh, tb.column_refresh + len(ra)]), t.column_refresh)
        assert (tb.orig_index, tb.resampled_index) == (t.orig_index, t.resampled_index)


@pytest.mark.parametrize("width,timerange,chunk", [(800, 10., 512), (333, 7., 640), (1920, 1., 4096), (100, 20., 512), (799, 3., 2048)])
@pytest.mark.parametrize("fft_size,overlap", [(4096, Fraction(3, 4)), (1000, Fraction(2, 3)), (512, Fraction(1, 2))])
def test_columns_equal_the_replayed_resampler(fft_size, overlap, width, timerange, chunk):
    """The column table against the restated time resampler (which the golden pins) over more settings: either both raise at the
    same refresh, or the tables agree, fillers included."""
    T = 60000
    sb = SpectrogramBatch(fft_size=fft_size, overlap=overlap, screen_width=width, screen_height=3, timerange_s=timerange)
    st = H.settings(fft_size=fft_size, overlap=overlap, screen_width=width, screen_height=3, timerange_s=timerange)
    fs, _ = sb.schedule(T, chunk=chunk)
    try:
        ref = H.screen_replay(np.zeros((int(fs[-1]), len(st["freq"]))), fs, st)
    except ValueError as e:
        with pytest.raises(ValueError, match=str(e).split(":")[0] + ":"):
            sb.columns(T, chunk=chunk)
        return
    t = sb.columns(T, chunk=chunk)
    assert np.array_equal(t.filler, ref["filler"]) and np.array_equal(t.column_refresh, ref["column_refresh"])
    assert np.array_equal(t.src, ref["src"]) and np.array_equal(t.a, ref["a"])
    assert (t.orig_index, t.resampled_index) == (ref["orig_index"], ref["resampled_index"])


def test_over_emission_raises_naming_the_refresh():
    c = H.OVER_EMISSION
    sb = SpectrogramBatch(fft_size=c["fft_size"], overlap=c["overlap"], screen_width=c["screen_width"], screen_height=c["screen_height"],
                          timerange_s=c["timerange_s"])
    with pytest.raises(ValueError, match=f"refresh {c['refresh']}:"):
        sb.columns(c["n"], chunk=c["chunk"])
    st = H.settings(**c)
    fs, _ = sb.schedule(c["n"], chunk=c["chunk"])
    with pytest.raises(ValueError, match=f"refresh {c['refresh']}:"):          # so does the restated reference
        H.screen_replay(np.zeros((int(fs[-1]), len(st["freq"]))), fs, st)


@pytest.mark.parametrize("fft_size", [32, 1024, 8192, 16384])
@pytest.mark.parametrize("overlap", [0.75, 0.5, 0.0])
def test_spectrum_batch_schedule_is_unchanged_and_shared(fft_size, overlap):
    """SpectrumBatch.schedule on its own cases (test_spectrumbatch_cpu) against the widget's bookkeeping replayed by the oracle, now
    that both classes call one helper; SpectrogramBatch.schedule returns the same tables."""
    sb, gb = SpectrumBatch(fft_size, overlap), SpectrogramBatch(fft_size, Fraction(overlap))
    T = 100000
    for ends, pending in [(chunk_ends(T, 512), 0), (chunk_ends(T, 5 * sb.hop + 3), 0), (_ragged(T, fft_size), 0),
                          (_ragged(T, fft_size + 1), 1), (_ragged(T, fft_size + 2), sb.hop - 1), (_ragged(T, fft_size + 3), sb.hop + 700)]:
        frames, chunks = SH.replay_schedule(fft_size, overlap, ends, pending)
        fs, rc = sb.schedule(T, ends=ends, state=SpectrumState(None, None, pending) if pending else None)
        assert fs.dtype == np.int64 and rc.dtype == np.int64 and fs[0] == 0
        assert np.diff(fs).tolist() == frames and rc.tolist() == chunks
        gs = gb.schedule(T, ends=ends, state=SpectrogramState(None, pending, None, 0., 0.) if pending else None)
        assert np.array_equal(gs[0], fs) and np.array_equal(gs[1], rc)
    assert sb.schedule(0)[0].tolist() == [0] and sb.schedule(0)[1].size == 0
    for bad in ([600, 500], [-1], [T + 1]):
        with pytest.raises(ValueError):
            sb.schedule(T, ends=bad)
        with pytest.raises(ValueError):
            gb.schedule(T, ends=bad)
    with pytest.raises(ValueError):
        gb.schedule(T, chunk=0)


def test_resampler_recurrence_is_a_pure_function():
    """advance_indices needs no library; the class method is that function applied to the object's indices."""
    from friture_amd.signal.online_linear_2D_resampler import advance_indices
    total, src, a, orig, res = advance_indices(0., 0., 0.5859375, 3)
    assert (total, src, orig) == (5, [0, 1, 1, 2, 2], 3.) and a[0] == 1. - 0.5859375 and res == 0.5859375 * 5
    assert advance_indices(0., 0., 18.75, 18)[:3] == (0, [], [])


def test_entry_point_is_in_header_table_and_library():
    from friture_amd import _lib
    header = (_lib.LIB_PATH.parents[2] / "include" / "friture_hip.h").read_text()
    assert "int frt_specgram_batch(" in header and "frt_specgram_batch" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "frt_specgram_batch")


def test_golden_files_are_small():
    largest = max(p.stat().st_size for p in GOLDEN.parent.glob("*.npz"))
    for p in GOLDEN.glob("*.npz"):
        assert p.stat().st_size <= largest and p.stat().st_size < 1 << 20, p.name
    assert sorted(p.stem for p in GOLDEN.glob("*.npz")) == sorted(H.GOLDEN_CASES)


def test_the_oracle_synth_is_the_tests_synth():
    """oracle.cases.synth (the recorders cannot import conftest) and conftest.synth give the same arrays."""
    for kind in ("noise", "tone", "chirp"):
        for n, seed in [(1, 1), (4800, 11), (12000, 12)]:
            a, b = H.synth(kind, n, seed), synth(kind, n, seed)
            assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (n,) and np.array_equal(a, b), (kind, n)
    with pytest.raises(ValueError):
        H.synth("square", 10, 0)
