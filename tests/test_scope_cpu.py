"""The oscilloscope without a GPU: width and region arithmetic, chunk schedules, the time axis, and the numpy restatement of
oracle/scope.py against tests/golden/scope.npz (recorded from the reference Scope_Widget)."""
from pathlib import Path

import numpy as np
import pytest

from oracle import scope as H

GOLDEN = Path(__file__).resolve().parent / "golden" / "scope.npz"


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def test_width_reproduces_python_rounding(g):
    from friture_amd.scope import width_for
    assert width_for(25.3) == 1214 and width_for(10.9) == 523 and width_for(50) == 2400 and width_for(0.1) == 4
    assert [width_for(t) for t in H.TIMERANGES] == list(g["widths"])


@pytest.mark.parametrize("width", [1, 2, 3, 4, 523, 1214, 2400, 2401, 24000, 24001])
def test_region_is_width_samples_and_trace_is_two_halves(width):
    """window[w//2 : -w//2] is exactly w samples for odd and even w, starting at w//2; the trace is 2 (w//2) samples."""
    from friture_amd.scope import trace_length
    win = np.arange(2 * width)
    region = win[width // 2:-width // 2]
    assert region.shape[0] == width and region[0] == width // 2
    assert trace_length(width, False) == 2 * (width // 2) and trace_length(width, True) == width


def test_scrolling_threshold():
    from friture_amd.scope import is_scrolling
    assert not is_scrolling(500) and not is_scrolling(500.0) and is_scrolling(500.1) and is_scrolling(2000)


@pytest.mark.parametrize("T,chunk", [(0, 512), (1, 512), (511, 512), (512, 512), (513, 512), (5000, 512), (4096, 1024)])
def test_chunk_ends(T, chunk):
    from friture_amd.scope import chunk_ends
    e = chunk_ends(T, chunk)
    assert e.dtype == np.int64 and e.shape[0] == -(-T // chunk)
    sizes = np.diff(np.concatenate([[0], e]))
    assert np.all(sizes[:-1] == chunk) if len(sizes) else True
    assert (len(e) == 0 and T == 0) or (e[-1] == T and 0 < sizes[-1] <= chunk)


@pytest.mark.parametrize("timerange", H.TIMERANGES)
def test_scaled_t_matches_reference_expression(timerange):
    from friture_amd.scope import is_scrolling, time_axis, trace_length, width_for
    w = width_for(timerange)
    L = trace_length(w, is_scrolling(timerange))
    time, st = time_axis(w, timerange, L)
    assert np.array_equal(time, (np.arange(L) - w // 2) / 48000.)
    assert np.array_equal(st, H.scaled_t(w, timerange, L))


def test_scaled_t_equals_recorded(g):
    for name, k in [("stereo", 5), ("tr_25.3", 7), ("exact_level", 5)]:
        tr = H.schedule(name)[k][3]
        w = H.width_for(tr)
        assert np.array_equal(g[f"{name}_full{k}_t"], H.scaled_t(w, tr, 2 * (w // 2)))


@pytest.mark.parametrize("name", H.CASES)
def test_restatement_matches_reference(g, name):
    """Every refresh whose window is the zero-padded stream: the restatement's trigger and start are the reference's."""
    ok, trig, start = g[f"{name}_ok"], g[f"{name}_trig"], g[f"{name}_start"]
    sched = H.schedule(name)
    assert ok.shape[0] == len(sched)
    for k, (s, n, rows, tr) in enumerate(sched):
        if not ok[k]:
            continue
        w = H.width_for(tr)
        scrolling = tr > 500.0
        n_win = w if scrolling else 2 * w
        r = H.refresh_np(H.expected_window(name, k, n_win), w, scrolling)
        assert (r != H.NO_TRIGGER) == bool(trig[k]), (name, k)
        if trig[k]:
            assert s + n - n_win + r == start[k], (name, k)


def test_only_the_ring_growth_case_leaves_the_stream(g):
    for name in H.CASES:
        bad = np.nonzero(~g[f"{name}_ok"])[0]
        if name == "change":
            assert bad[0] == 38 and len(bad) == 14
        else:
            assert len(bad) == 0, name
    assert not bool(g["change_full38_trig"]) and bool(g["change_full46_trig"])


def _starts_with_level(x, ends, width, level_fn):
    out = []
    for e in ends:
        win = np.zeros(2 * width)
        lo = max(e - 2 * width, 0)
        win[2 * width - (e - lo):] = x[lo:e]
        region = win[width // 2:-width // 2]
        lev = level_fn(region.max())
        pos = np.nonzero((region[:-1] < lev) & (region[1:] >= lev))[0]
        out.append(e - 2 * width + int(pos[0]) if len(pos) else H.NO_TRIGGER)
    return np.array(out)


@pytest.mark.parametrize("name,other", [("exact_level", lambda m: m * (2. / 3.)),
                                        ("exact_level_f32", lambda m: float(np.float32((m * 2.) / 3.)))])
def test_exact_level_cases_tell_the_roundings_apart(g, name, other):
    """(m * 2.) / 3. in float64 is what the reference triggers on: m * (2/3), or the level rounded to float32, start elsewhere."""
    x = H.signal(name)[0]
    ends = H.chunk_ends(x.shape[0])
    ref = g[f"{name}_start"]
    assert np.array_equal(_starts_with_level(x, ends, 2400, lambda m: (m * 2.) / 3.), ref)
    diff = _starts_with_level(x, ends, 2400, other) != ref
    assert diff.sum() >= 10


def test_batch_restatement_equals_refresh_restatement(g):
    x = H.signal("stereo")
    ends = H.chunk_ends(x.shape[1])
    assert np.array_equal(H.batch_np(x[0], ends, 2400, False), g["stereo_start"])
