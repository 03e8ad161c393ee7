"""SoundLevelBatch's detector on the GPU at every instance and setting that tests/test_soundlevel_gpu.py leaves out: one, three and
four time constants (spl_cells_kernel<1>, <3>, <4> and the state layout 9 ntau + 5 at each), the smallest and the largest cell,
an interval of one cell and one of more than a run of cells, level-two walks of whole rounds of 16 steps and of one step more,
and tables at their extremes (a next to 1; A and A64 that underflow to 0; a denormal A).

The bars are the suite's own (soundlevel_helpers.check_fields against the sequential recurrence in np.longdouble), and on every
input the device must be the float64 numpy restatement of the cell form (soundlevel_helpers.cell_form) bit for bit;
tests/test_soundlevel_edges_cpu.py shows that restatement inside the bars on the same inputs.  Every parity test prints its
distances before it asserts.  Inputs and references are made once per process (soundlevel_helpers.cached)."""
import numpy as np
import pytest

import soundlevel_helpers as sl
from sos_helpers import decaying_noise
from soundlevel_helpers import as_fields, pieces_equal_whole, same_bits, same_detector_state, same_result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import soundlevel
    return soundlevel


def parity(mod, case):
    """The detector on the case's input: check_fields against the long double recurrence, then the bits of cell_form.  Returns
    (the batch, w, the DetectorResult)."""
    kind, T, s = case
    w, ref, seq, bar, peak = sl.cached(kind, T, **s)
    batch = mod.SoundLevelBatch("Z", **s)
    d = batch.detect(w)
    got = as_fields(d)
    print(f"{sl.edge_id(case)}: worst device / bar {sl.worst_ratio(got, ref, bar, peak):.3f}, sequential / bar "
          f"{sl.worst_ratio(seq, ref, bar, peak):.3f}, bar {bar.min():.2e} .. {bar.max():.2e}")
    assert got.last.shape == (w.shape[0], -(-T // s["interval"]), len(s["taus"])) and d.total_count == T and d.state.n == T
    sl.check_fields(got, ref, bar, peak, w, s["interval"])
    want = sl.cell_form(w, s["fs"], s["taus"], s["cell"], s["interval"])
    for name in sl.FIELD_NAMES:
        same_bits(getattr(got, name), getattr(want, name))
    return batch, w, d


@pytest.mark.parametrize("case", sl.TAUS_CASES, ids=sl.edge_id)
def test_every_number_of_time_constants(mod, case):
    """1, 3 and 4 time constants at interval 480 and cell 32, 3 float64 rows of 2049, of 64 * 32 + 33 and (three runs: level two
    multiplies every A64 by a U that is not 0) of 2 * 64 * 32 + 33 samples.  For one and for four time constants the pieces of
    the 64 * 32 + 33 row give the bits and the state of the whole (the state is 9 ntau + 5 doubles per row); for four, 5 rows in
    slabs of one row give the bits of one launch."""
    batch, w, d = parity(mod, case)
    ntau, T = batch.ntau, case[1]
    assert batch.state_length == 9 * ntau + 5 and d.state.data.shape == (3, 9 * ntau + 5)
    if T != sl.PIECES_LENGTH or ntau == 3:
        return
    whole, state = pieces_equal_whole(batch, w, sl.PIECE_CUTS)
    same_detector_state(state, whole.state)
    if ntau == 4:
        rows = decaying_noise(5, T, 77, rt=1.0)
        cells, runs = T // 32 + 1, T // 32 // 64 + 1
        per_row = 8 * (ntau * (2 * (cells + 1) + 2 * runs) + (2 + 3 * ntau) * (cells + 1))
        one = batch.detect(rows)
        slabs = batch.detect(rows, scratch_bytes=per_row + 8)    # a little more than one row's scratch: one row per launch
        same_result(slabs, one)
        same_detector_state(slabs.state, one.state)


@pytest.mark.parametrize("case", sl.EXTREME_CASES, ids=sl.edge_id)
def test_cell_and_interval_extremes(mod, case):
    """(cell, interval) = (16, 16), (16, 48), (48, 96), (80, 480), (1024, 1024), (1024, 2048): the smallest cell is one tile, so
    the loop never asks for a next one; an interval of one cell; the largest cell."""
    parity(mod, case)


def test_an_interval_longer_than_a_run(mod):
    """Cell 16 and interval 1280: 80 cells per interval, so an interval's fold crosses a run seam; whole and in pieces cut at the
    run seam inside interval 0, at the interval's end and one sample behind it."""
    batch, w, d = parity(mod, sl.LONG_INTERVAL_CASE)
    assert batch.interval // batch.cell == 80
    whole, state = pieces_equal_whole(batch, w, sl.LONG_INTERVAL_CUTS)
    same_detector_state(state, whole.state)


@pytest.mark.parametrize("case", sl.WALK_CASES, ids=sl.edge_id)
def test_level_two_walks_of_whole_and_partial_rounds(mod, case):
    """Cell 16, interval 1024, three time constants, one row of 17, 18, 33 and 34 runs: level two makes 16, 17, 32 and 33 steps,
    that is whole rounds of the 16 values of Q it keeps ahead, and a whole round followed by one step."""
    parity(mod, case)


@pytest.mark.parametrize("case", sl.TABLE_CASES + [sl.DENORMAL_CASE], ids=sl.edge_id)
def test_table_extremes(mod, case):
    """fs 192 kHz with Slow (a = 1 - 5.2e-6); tau = 20 us, where A = a^1024 and A64 are exactly 0, and where A = 3.3e-15 and A64 = 0;
    tau = 20 us alone at cell 704, where A = a^704 is a denormal double: behind a unit sample the averages walk through the
    denormals in the sample loop, and behind a unit sample at the end of cell 0 the scan makes the denormal product A g.  The device
    keeps them (float64 denormals are not flushed), bit for bit with numpy."""
    batch, w, d = parity(mod, case)
    if case is sl.DENORMAL_CASE:
        tiny = np.finfo(np.float64).tiny
        assert 0.0 < d.last[0, 0, 0] < tiny and 0.0 < d.max[2, 2, 0] < tiny
