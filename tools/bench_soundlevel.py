"""SoundLevelBatch (soundlevel.hip): the sound level meter over whole recordings.

Shapes: (a) 64 rows x 2^20 float32, A-weighted, Fast and Slow; (b) 8 rows x 2^22 float64, Z-weighted; (c) 8 rows x 2^20 float32
into the 18 third-octave bands (Z).  Interval 4800 at 48 kHz throughout.  The rows are decaying Gaussian noise made on the device.
Per shape, on CUDA tensors between device events after a warm-up, median / min / max of --reps calls: the whole chain
(SoundLevelBatch.run), and the detector alone (SoundLevelBatch.detect on the weighted float64 rows) with the bytes it has to move
(the samples read twice) as a share of the 8 TB/s HBM peak.  With --cells the detector at every listed cell size (the default
cell was chosen from such a run on shape (a)).  Beside them, same session, same weighted rows: the route a user had before the
class: w.double().square(), SosBatch with one one-pole section [g, 0, 0, 1, -a, 0] per time constant in bank mode, then reshape,
amax, amin and sum per interval in torch; and scipy.signal.lfilter on ONE row on the host, multiplied by the row count: an
extrapolation, not a measurement of the batch.  Prints one JSON line and writes it to --out."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FS, INTERVAL = 48000, 4800
SHAPES = [("a", 64, 1 << 20, "float32", "A", None), ("b", 8, 1 << 22, "float64", "Z", None), ("c", 8, 1 << 20, "float32", "Z", "third")]


def stats(t):
    med, tmin, tmax = t
    return {"median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--cells", default="", help="cell sizes to time the detector at beside the default, e.g. 96,160,240,480")
    ap.add_argument("--no-routes", action="store_true", help="SoundLevelBatch alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from friture_amd import _lib, sosfilter, soundlevel
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_soundlevel", "interval": INTERVAL, "default_cell": soundlevel.SoundLevelBatch("Z", interval=INTERVAL).cell, "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, R, T, dtype, weighting, bands in SHAPES:
        if label not in a.shapes.split(","):
            continue
        t = torch.arange(T, device="cuda", dtype=torch.float64) / FS
        x = (torch.randn((R, T), device="cuda", dtype=torch.float64, generator=g) * 10.0 ** (-3.0 * t / (0.4 * T / FS))).to(getattr(torch, dtype))
        del t
        batch = soundlevel.SoundLevelBatch(weighting, interval=INTERVAL, bands=bands)
        w = x                                                     # the rows the detector sees
        for sos, fan in batch._filters:
            w = sos.run(w, fan=fan, dtype="float64").y.reshape(-1, T)
        rows = w.shape[0]
        moved = w.numel() * w.element_size() * 2                  # the samples read by both passes
        row = {"shape": label, "rows": R, "samples": T, "dtype": dtype, "weighting": weighting, "bands": batch.n_bands, "taus": list(batch.taus),
               "detector_rows": rows, "detector_dtype": str(w.dtype).split(".")[-1], "reps": a.reps, "algorithmic_bytes": moved, "cells": {}}
        batch.run(x)
        torch.cuda.synchronize()
        row["chain"] = stats(time_call(lambda: batch.run(x), a.reps))
        for cell in [None] + [int(c) for c in a.cells.split(",") if c]:
            det = soundlevel.SoundLevelBatch("Z", interval=INTERVAL, cell=cell)
            det.detect(w)
            torch.cuda.synchronize()
            t3 = time_call(lambda: det.detect(w), a.reps)
            entry = dict(stats(t3), hbm_share=moved / t3[0] / HBM_PEAK)
            row["cells"][str(det.cell)] = entry
            if cell is None:
                row["detector"] = dict(entry, cell=det.cell)
            del det
        if not a.no_routes:
            aa, gg, _, _ = batch.tables()
            poles = sosfilter.SosBatch(np.array([[[gi, 0.0, 0.0, 1.0, -ai, 0.0]] for ai, gi in zip(aa, gg)]))
            J = T // INTERVAL

            def route():
                q = w.double().square()
                e = poles.run(q, fan=True).y[..., :J * INTERVAL].reshape(rows, len(aa), J, INTERVAL)
                return e.amax(-1), e.amin(-1), e[..., -1], q[:, :J * INTERVAL].reshape(rows, J, INTERVAL).sum(-1)
            got = route()
            torch.cuda.synchronize()
            want = batch.detect(w, flush=False)
            row["torch_route"] = dict(stats(time_call(route, a.reps)),
                                      what="w.double().square(), SosBatch of one-pole sections in bank mode, reshape, amax, amin, sum in torch",
                                      distance_max=float(((got[0].transpose(1, 2) - want.max).abs().amax() / want.max.abs().amax()).cpu()))
            row["torch_route_over_detector"] = row["torch_route"]["median_ms"] / row["detector"]["median_ms"]
            del got, want
            try:
                from scipy.signal import lfilter
            except ImportError:
                row["scipy_route"] = "not measured: scipy is not installed"
            else:
                one = w[0].cpu().numpy().astype(np.float64)
                t0 = time.perf_counter()
                q = one * one
                for ai, gi in zip(aa, gg):
                    lfilter([gi], [1.0, -ai], q)
                dt = time.perf_counter() - t0
                row["scipy_route"] = {"what": "scipy.signal.lfilter per time constant, float64, one host thread, ONE row timed once and multiplied by "
                                              "the detector's row count: an extrapolation", "one_row_ms": dt * 1e3, "extrapolated_ms": dt * rows * 1e3}
                row["scipy_route_over_detector"] = dt * rows * 1e3 / row["detector"]["median_ms"]
        res["shapes"].append(row)
        del x, w, batch
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
