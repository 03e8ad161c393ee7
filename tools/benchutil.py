"""Shared by the widget bench tools (bench_levels, bench_scope, bench_plotcurves, bench_spectrumbatch): the event-timed repeat
and the one JSON result line."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

HBM_PEAK = 8e12


def time_call(fn, reps, before_each=None):
    """(median_s, min_s, max_s) of `reps` calls of fn(), each between two device events and followed by a synchronisation;
    before_each() runs untimed ahead of every call.  The caller warms up."""
    import torch
    ts = []
    for _ in range(reps):
        if before_each is not None:
            before_each()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts)), min(ts), max(ts)


def emit(res, out=None):
    """Print the result as one JSON line and write it to `out` when given."""
    line = json.dumps(res)
    print(line)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(line + "\n")
