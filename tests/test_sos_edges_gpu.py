"""SosBatch on the GPU at every instance and setting that tests/test_sos_gpu.py leaves out: every section count K = 1 .. 8 in bank
and in row mode over two runs and in bank mode over three (the first length at which level two's product with M^64 counts),
every cell size across a run seam, level-two walks of whole rounds of 16 steps and of one step more, banks of 1, 4
and 64 filters, stiff and real-pole filters across a run seam, and reverse on strided float32 rows.

The bar is the suite's own: per output row within max(64 e_seq, 1e-13) of the sequential recurrence in np.longdouble
(sos_helpers.bar); tests/test_sos_edges_cpu.py shows the float64 numpy restatement of the cell form inside it on the same inputs.
Every parity test prints its distances (the last figure: the worst device / bar) before it asserts.  Inputs and references are
made once per process (sos_helpers.cached)."""
import numpy as np
import pytest

import sos_helpers as sh
from sos_helpers import parity, run_pieces, same_bits, same_state

pytestmark = pytest.mark.gpu

S = sh.EDGE_CELL


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import sosfilter
    return sosfilter


@pytest.mark.parametrize("mode", ["bank", "row"])
@pytest.mark.parametrize("K", sh.SECTION_COUNTS)
def test_every_section_count(mod, K, mode):
    """T = 64 * 32 + 33 at cell 32: two runs, one step of level two.  Bank mode: 2 float64 rows into F = 5 bands, so the second
    filter group has three idle wavefronts.  Row mode: 3 rows through 2 filters; also in slabs of one row (row0 % F != 0) and with
    float32 in and out."""
    x, sos, fan, yld, y64 = sh.cached("sections", K, mode)
    batch = mod.SosBatch(sos, cell=S)
    assert batch.sections == K
    res = batch.run(x, fan=fan)
    assert res.y.dtype == np.float64 and res.y.shape == ((2, 5, sh.SECTIONS_LENGTH) if fan else (3, sh.SECTIONS_LENGTH))
    parity(res.y, "sections", (K, mode), f"K {K} {mode}")
    if fan:
        return
    slabs = batch.run(x, scratch_bytes=1)
    same_bits(slabs.y, res.y)
    same_state(slabs.state, res.state)
    x32 = x.astype(np.float32)
    y32 = batch.run(x32).y
    assert y32.dtype == np.float32
    same_bits(y32, batch.run(x32, dtype=np.float64).y.astype(np.float32))


@pytest.mark.parametrize("K", sh.SECTION_COUNTS)
def test_every_section_count_over_three_runs(mod, K):
    """T = 2 * 64 * 32 + 33 at cell 32, one row into the five bands: with two runs level two only adds Q_0 to M^64 times U_0 = 0;
    its second step is the first whose 2K x 2K product with M^64 counts (the 125 Hz band's M^64 has entries of 4e-5 at K = 1 and
    near 1 from K = 3 on, far above the bar)."""
    x, sos, fan, yld, y64 = sh.cached("three_runs", K)
    parity(mod.SosBatch(sos, cell=S).run(x, fan=True).y, "three_runs", (K,), f"K {K}, three runs")


@pytest.mark.parametrize("cell", sh.CELLS)
def test_every_cell_size_across_a_run_seam(mod, cell):
    """T = 65 cell + 17: 66 cells, two runs, the last cell partial; K = 3 in bank mode, one row into three octaves."""
    x, sos, fan, yld, y64 = sh.cached("cells", cell)
    batch = mod.SosBatch(sos, cell=cell)
    res = batch.run(x, fan=True)
    assert res.state.n == 65 * cell + 17
    parity(res.y, "cells", (cell,), f"cell {cell}")


@pytest.mark.parametrize("nr", sh.WALK_RUNS)
def test_level_two_walks_of_whole_and_partial_rounds(mod, nr):
    """nr runs at cell 32: level two makes nr - 1 = 16, 17, 32, 33 steps, that is whole rounds of the 16 values of Q it keeps
    ahead, and a whole round followed by one step.  The filter is the 16 Hz octave of order 1, whose state outlives a run: a
    U_r that is wrong or late shows in every run behind it."""
    x, sos, fan, yld, y64 = sh.cached("walk", nr)
    batch = mod.SosBatch(sos, cell=S)
    whole = batch.run(x)
    assert x.shape[1] // S // 64 + 1 == nr
    parity(whole.y, "walk", (nr,), f"{nr - 1} steps of level two")
    if nr == 18:                                                 # the second piece starts one sample into run 16
        y, state = run_pieces(batch, x, [16 * 64 * S + 1], False)
        same_bits(y, whole.y)
        same_state(state, whole.state)


@pytest.mark.parametrize("F", sh.WIDTHS)
def test_bank_widths(mod, F):
    """F = 1 (three idle wavefronts), 4 (exactly one filter group) and 64 (the maximum): K = 1, one row of 65 samples.  Output row
    f of the bank has the bits of a row-mode run through filter f alone."""
    x, sos, fan, yld, y64 = sh.cached("width", F)
    y = mod.SosBatch(sos, cell=S).run(x, fan=True).y
    assert y.shape == (1, F, 2 * S + 1)
    parity(y, "width", (F,), f"F {F}")
    for f in range(F):
        same_bits(mod.SosBatch(sos[f], cell=S).run(x).y[0], y[0, f])


@pytest.mark.parametrize("cell", sh.STIFF_CELLS)
@pytest.mark.parametrize("kind", sh.STIFF_KINDS)
def test_stiff_and_real_pole_filters_across_a_run_seam(mod, kind, cell):
    """The 20 Hz third-octave of order 4 and the A and C weightings (double real poles at 20.6 Hz) on 2 rows of 65 cell + 17
    samples that decay by 60 dB in 2 s, row mode."""
    x, sos, fan, yld, y64 = sh.cached("stiff", kind, cell)
    batch = mod.SosBatch(sos, cell=cell)
    assert batch.sections == {"band20": 4, "A": 3, "C": 2}[kind]
    parity(batch.run(x).y, "stiff", (kind, cell), f"{kind} at cell {cell}")


def test_reverse_on_strided_float32_rows(mod):
    """K = 2, F = 5 in bank mode at cell 64, T = 64 * 64 + 77: float32 rows as a strided view with a lead-in of 3, float32 output,
    on the host and on the device."""
    import torch
    T = 64 * 64 + 77
    wide = np.zeros((3, T + 8), np.float32)
    wide[:, 3:3 + T] = sh.decaying_noise(3, T, 600, dtype=np.float32)
    view = wide[:, 3:3 + T]
    batch = mod.SosBatch(sh.bank(5, 2), cell=64)
    back = batch.run(view, fan=True, reverse=True)
    assert back.state is None and back.y.dtype == np.float32 and back.y.shape == (3, 5, T)
    forward = batch.run(np.ascontiguousarray(view[:, ::-1]), fan=True).y
    assert forward.dtype == np.float32 and np.abs(forward).max() > 0
    same_bits(back.y, forward[..., ::-1])
    dev = torch.from_numpy(wide).cuda()[:, 3:3 + T]
    assert not dev.is_contiguous()
    same_bits(batch.run(dev, fan=True, reverse=True).y, back.y)
