"""The edge settings of tests/test_soundlevel_edges_gpu.py without a GPU: the float64 numpy restatement of the cell form
(soundlevel_helpers.cell_form) meets check_fields against the long double sequential recurrence on every one of them, so a
failure of the device on the same input points at the device, not at the bar; and the tables have the extremes the cases are
named for.  Each parity test prints its distances before it asserts."""
import numpy as np
import pytest

import soundlevel_helpers as sl
from friture_amd import soundlevel


@pytest.mark.parametrize("case", sl.EDGE_CASES, ids=sl.edge_id)
def test_cell_form_meets_the_bars(case):
    kind, T, s = case
    w, ref, seq, bar, peak = sl.cached(kind, T, **s)
    got = sl.cell_form(w, s["fs"], s["taus"], s["cell"], s["interval"])
    print(f"{sl.edge_id(case)}: worst cell form / bar {sl.worst_ratio(got, ref, bar, peak):.3f}, sequential / bar "
          f"{sl.worst_ratio(seq, ref, bar, peak):.3f}, bar {bar.min():.2e} .. {bar.max():.2e}")
    assert got.last.shape == (w.shape[0], -(-T // s["interval"]), len(s["taus"]))
    sl.check_fields(got, ref, bar, peak, w, s["interval"])


def test_the_tables_have_the_extremes_the_cases_are_named_for():
    def tables(case):
        s = case[2]
        got = soundlevel.SoundLevelBatch("Z", **s).tables()
        for g, want in zip(got, sl.tables(s["fs"], s["taus"], s["cell"])):
            assert g.tobytes() == want.tobytes()
        return got

    a, g, A, A64 = tables(sl.TABLE_CASES[0])
    assert 5.1e-6 < 1 - a[0] < 5.3e-6 and 0 < A64[0] < A[0] < 1
    a, g, A, A64 = tables(sl.TABLE_CASES[1])
    assert A[0] == 0.0 and A64[0] == 0.0 and A[1] > 0
    a, g, A, A64 = tables(sl.TABLE_CASES[2])
    assert 3.2e-15 < A[0] < 3.4e-15 and A64[0] == 0.0
    a, g, A, A64 = tables(sl.DENORMAL_CASE)
    assert 0.0 < A[0] < np.finfo(np.float64).tiny and A64[0] == 0.0
    # the rows that would show a flush to zero: behind a unit sample the sample loop walks through the denormals (row 0), and
    # behind a unit sample at the end of cell 0, cell 2 starts from A g, a denormal product of the scan (row 2)
    tiny = np.finfo(np.float64).tiny
    w = sl.unit_and_noise(sl.DENORMAL_CASE[1])
    assert w[0, 0] == 1.0 and not w[0, 1:].any() and w[1].all() and w[2, sl.UNIT_AT] == 1.0 and np.count_nonzero(w[2]) == 1
    got = sl.cell_form(w, **{k: sl.DENORMAL_CASE[2][k] for k in ("fs", "taus", "cell", "interval")})
    assert 0.0 < got.last[0, 0, 0] < tiny and got.last[0, 0, 0] == got.min[0, 0, 0]
    assert 0.0 < got.max[2, 2, 0] < tiny and got.max[2, 2, 0] == a[0] * (A[0] * g[0])


def test_the_edge_cases_are_what_they_claim():
    for kind, T, s in sl.EXTREME_CASES + [sl.LONG_INTERVAL_CASE] + sl.WALK_CASES:
        assert s["interval"] % s["cell"] == 0
    assert [(s["cell"], s["interval"] // s["cell"]) for _, _, s in sl.EXTREME_CASES] == [(16, 1), (16, 3), (48, 2), (80, 6), (1024, 1), (1024, 2)]
    assert sl.LONG_INTERVAL_CASE[2]["interval"] // sl.LONG_INTERVAL_CASE[2]["cell"] == 80
    assert [T // (64 * 16) for _, T, s in sl.WALK_CASES] == [16, 17, 32, 33]      # the steps of level two
    assert [soundlevel.SoundLevelBatch("Z", **s).state_length for _, _, s in sl.TAUS_CASES[::len(sl.TAUS_LENGTHS)]] == [14, 32, 41]
