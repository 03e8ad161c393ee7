"""The edge inputs of tests/test_sos_edges_gpu.py without a GPU: the float64 numpy restatement of the cell form
(sos_helpers.cell_form) stays within max(64 e_seq, 1e-13) of the long double sequential recurrence on every one of them, so a
failure of the device on the same input points at the device, not at the bar.  Each test prints its distances before it asserts."""
import numpy as np
import pytest

import sos_helpers as sh


def ident(case):
    name, args, cell = case
    return "-".join([name] + [str(a) for a in args])


@pytest.mark.parametrize("case", sh.EDGE_INPUTS, ids=ident)
def test_cell_form_stays_within_the_bar(case):
    name, args, cell = case
    x, sos, fan, yld, y64 = sh.cached(name, *args)
    assert yld.shape[1] == x.shape[1] and yld.shape[0] == x.shape[0] * (len(sh.normalise(sos)) if fan else 1)
    e, d, b = sh.distance(y64, yld), sh.distance(sh.cell_form(x, sos, cell, fan), yld), sh.bar(y64, yld)
    print(f"{ident(case)} at cell {cell}: e_seq {e.max():.2e}, cell form {d.max():.2e}, worst cell form / bar {(d / b).max():.3f}")
    assert np.all(d <= b)


def test_the_edge_inputs_are_what_they_claim():
    """The shapes that make the cases edges: the runs, the steps of level two, the filters per row, the section counts."""
    from friture_amd import sosfilter
    for name, args, cell in sh.EDGE_INPUTS:
        x, sos, fan = sh.INPUTS[name](*args)
        batch = sosfilter.SosBatch(sos, cell=cell)                   # the host's own check of the poles passes
        runs = x.shape[1] // cell // sh.RUN + 1
        if name == "sections":
            assert batch.sections == args[0] and runs == 2 and batch.filters == (5 if fan else 2) and x.shape[0] == (2 if fan else 3)
        elif name == "three_runs":
            assert batch.sections == args[0] and runs == 3 and batch.filters == 5 and fan
            assert np.abs(batch.tables()[2][0]).max() > 1e-5         # the 125 Hz band remembers across a run: far above the bar
        elif name == "cells":
            assert (batch.sections, batch.filters, runs, x.shape[1] % cell) == (3, 3, 2, 17) and fan
        elif name == "walk":
            assert (batch.sections, batch.filters, runs) == (1, 1, args[0]) and x.shape[1] % cell == 5
            assert np.abs(batch.tables()[2]).max() > 0.1             # and so does the walk's filter
        elif name == "width":
            assert (batch.sections, batch.filters, x.shape) == (1, args[0], (1, 65)) and fan
        else:
            assert batch.sections == {"band20": 4, "A": 3, "C": 2}[args[0]] and runs == 2 and x.shape[0] == 2 and not fan
    assert sorted(k - 1 for k in sh.WALK_RUNS) == [16, 17, 32, 33]
