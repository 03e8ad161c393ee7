"""The cases of test_decay_edges_gpu.py without a GPU: every builder of tests/decay_helpers.py is run (each asserts
check_gaps(refs) at 1e-6 on its longdouble references), and the conditions that make a case what it claims to be are asserted on
the reference alone: which path of the kernels a shape takes, which outputs are reached, which rows are dead."""
import math

import numpy as np
import pytest

import decay_helpers as dh

TL = dh.TILE


def test_strided_probes_on_the_reference():
    """Live spans of 67 and 66 tiles, every T30 reached, and the three launch shapes: 4 rows and slabs of about 100 rows take
    every tile in one trip, 520 rows need a second."""
    x, refs = dh.strided_case()
    assert x.shape == (4, 66 * TL + 5) and x.dtype == np.float32
    assert [r["onset"] for r in refs] == [0, TL, TL, 3] and all(r["truncation"] == dh.STRIDED_T for r in refs)
    assert all(math.isfinite(r[f]) for r in refs for f in ("edt", "t10", "t20", "t30"))
    spans = dh.live_tiles([r["onset"] for r in refs], [r["truncation"] for r in refs])
    assert spans.tolist() == [67, 66, 66, 67]
    print("gaps:", [f"{r['gap_db']:.3g}" for r in refs])
    assert all(dh.strided(n, dh.STRIDED_ROWS) for n in spans)
    assert not any(dh.strided(n, 4) for n in spans) and not any(dh.strided(n, 101) for n in spans)
    assert max(spans) * TL <= 1 << 17                                # the bars were derived for live spans up to 2^17 samples


def test_live_spans_of_64_and_65_tiles_on_the_reference():
    x, onset, truncation, refs = dh.live_span_case()
    assert dh.live_tiles(onset, truncation).tolist() == [64, 65, 64, 65, 64, 65]
    assert set((onset // TL).tolist()) == {0, 1} and set((onset % TL).tolist()) == {0, 3, 7}
    assert all(math.isfinite(r["t30"]) for r in refs)


@pytest.mark.parametrize("W", dh.EDGE_BLOCKS)
def test_block_cases_on_the_reference(W):
    """What each block length is there for: the group of 8 lanes (W < 64) with and without a ragged lane, both sides of the
    dispatch, a block of a tile and one more, two blocks, one block (nothing behind the peak: no automatic truncation,
    dynamic_range 0) and none (N0 = 0)."""
    T = dh.EDGE_T
    for f32 in (False, True):
        x, refs = dh.block_case(W, f32)
        assert x.shape == (65 if f32 else 3, T) and x.dtype == (np.float32 if f32 else np.float64)
        assert {r["onset"] // TL for r in refs} == {0, 1}
        nb = T // W
        if nb >= 3:
            assert any(r["truncation"] < T for r in refs) and any(math.isfinite(r["edt"]) for r in refs)
        if nb == 1:
            assert all(r["truncation"] == T and abs(float(r["dynamic_range"])) <= 1e-12 for r in refs)
        if nb == 0:
            assert all(r["truncation"] == T and math.isnan(r["dynamic_range"]) and r["noise_db"] == -math.inf for r in refs)
    assert {W: T // W for W in (1000, 2577, 65536)} == {1000: 2, 2577: 1, 65536: 0}


@pytest.mark.parametrize("fs", dh.EDGE_FS)
def test_fs_cases_on_the_reference(fs):
    """n50 and n80 are what X3 says at each fs; the long row reaches both in every row, and its given onsets put the E50 pick on
    the first sample of a tile and on the last one of the tile before."""
    n50, n80 = dh.clarity_samples(fs)
    assert (n50, n80) == {8000: (400, 640), 11025: (551, 882), 44100: (2205, 3528), 96000: (4800, 7680), 192000: (9600, 15360)}[fs]
    for f32 in (False, True):
        x, refs = dh.fs_case(fs, f32)
        assert x.shape[1] == 4 * TL + 100 and all(math.isfinite(r["edt"]) for r in refs)
    x, onset, refs = dh.fs_long_case(fs)
    assert all(r["onset"] + n80 < r["truncation"] == x.shape[1] for r in refs)
    assert all(math.isfinite(float(r[f])) for r in refs for f in ("c50", "c80")) and all(0 < r["d50"] < 1 for r in refs)
    assert (onset[1] + n50) % TL == 0 and (onset[2] + n50) % TL == TL - 1 and onset[0] <= onset[1] < onset[0] + TL
    assert refs[0]["onset"] == dh.restate(x[0], fs=fs, block=16, truncate=None)["onset"]


@pytest.mark.parametrize("name,value", dh.EDGE_SETTINGS)
def test_setting_cases_on_the_reference(name, value):
    T, W = dh.EDGE_T, 16
    nb = T // W
    for f32 in (False, True):
        x, refs = dh.setting_case(name, value, f32)
        base = dh.restate_rows(x, block=W, real=np.longdouble)
        if name == "onset_db":
            assert all(r["onset"] >= 300 for r in refs)
            if value == 0.0:                                          # the onset is the peak, and that is another sample than at -20 dB
                assert all(r["onset"] == r["peak"] for r in refs) and any(r["onset"] > b["onset"] for r, b in zip(refs, base))
            assert all((r["onset"] <= b["onset"]) if value < -20.0 else (r["onset"] >= b["onset"]) for r, b in zip(refs, base))
        if name == "noise_tail":
            nt = max(1, math.ceil(value * nb))
            assert nt == {0.001: 1, 0.5: 81, 1.0: nb}[value]
            if value == 1.0:                                          # the truncation lands just behind the onset
                assert all(math.isnan(r["t30"]) and math.isfinite(r["edt"]) and r["truncation"] < r["onset"] + TL for r in refs)
        if name == "margin_db":
            assert all(r["truncation"] < T for r in refs)
            if value != 10.0:
                assert any(r["truncation"] != b["truncation"] for r, b in zip(refs, base))


def test_dead_rows_by_given_indices_on_the_reference():
    """Each bad pair fails exactly the test X3 gives (0 <= t0 < T, t0 < t1 <= T); the good row between them is live."""
    x, onset, truncation, good, ref = dh.dead_index_case()
    T = x.shape[1]
    ok = (onset >= 0) & (onset < T) & (truncation > onset) & (truncation <= T)
    assert ok.tolist() == [i == good for i in range(7)] and 0 < good < 6
    assert list(zip(onset.tolist(), truncation.tolist())) == [(-1, T), (T, T), (5, 0), (5, T - 100), (5, T + 1), (700, 700), (700, 100)]
    assert math.isfinite(ref["edt"]) and ref["onset"] == 5 and ref["truncation"] == T - 100


def test_an_onset_at_or_behind_the_automatic_truncation_on_the_reference():
    """The restatement calls such a row dead (X3, step 4) and leaves its neighbours alone."""
    x, onset, refs = dh.late_onset_case()
    found = dh.restate_rows(x, block=16, curve_step=7, real=np.longdouble)
    assert onset[1] == found[1]["truncation"] and onset[3] == found[3]["truncation"] + 5 and onset[3] < x.shape[1]
    for i in (1, 3):
        assert refs[i]["peak"] == refs[i]["onset"] == refs[i]["truncation"] == -1 and math.isnan(refs[i]["edt"])
        assert np.all(np.isnan(refs[i]["curve"])) and np.all(np.isnan(refs[i]["r2"]))
    for i in (0, 2, 4):
        assert all(refs[i][f] == found[i][f] for f in dh.FLOATS + dh.INDICES if not (isinstance(found[i][f], float) and math.isnan(found[i][f])))
        assert math.isfinite(refs[i]["edt"])
