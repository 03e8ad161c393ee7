"""SosBatch (sosfilter.hip): IIR second-order-section filters and band banks over whole recordings.

Shapes: (a) 64 responses x 2^17 float64 into the six octave bands, order 3, bank mode; (b) 8 rows x 2^22 float32 through one
order-3 filter, row mode; (c) 1 row x 2^24 float32 into the 18 third-octave bands, bank mode.  The rows are decaying Gaussian
noise made on the device.  Per shape: SosBatch(..).run on a CUDA tensor between device events after a warm-up, median / min / max
of --reps calls, and the bytes the algorithm moves (x read twice, y written once) as a share of the 8 TB/s HBM peak.  With
--cells the same at every listed cell size (the default cell was chosen from such a run).  Beside them, same session, same data:
(a) the route without the class, six ConvolveBatch(band_filter(..)).run calls; (b) scipy.signal.sosfilt on ONE row on the host,
multiplied by the row count: an extrapolation, not a measurement of the batch.  For (c), a kernel trace of its own
(--no-routes --shapes c under the profiler) gives the level-two scan alone.  Prints one JSON line and writes it to --out."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FS = 48000
SHAPES = [("a", 64, 1 << 17, "float64", "octave", True), ("b", 8, 1 << 22, "float32", None, False), ("c", 1, 1 << 24, "float32", "third", True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--cells", default="", help="cell sizes to time beside the default, e.g. 64,256,512")
    ap.add_argument("--no-routes", action="store_true", help="SosBatch alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from friture_amd import _lib, convolve, decay, sosfilter
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_sos", "default_cell": sosfilter.SosBatch(sosfilter.butter_band_sos(500.0, 1000.0)).cell, "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, R, T, dtype, bands, fan in SHAPES:
        if label not in a.shapes.split(","):
            continue
        t = torch.arange(T, device="cuda", dtype=torch.float64) / FS
        x = (torch.randn((R, T), device="cuda", dtype=torch.float64, generator=g) * 10.0 ** (-3.0 * t / (0.4 * T / FS))).to(getattr(torch, dtype))
        del t
        sos = sosfilter.band_sos(bands, FS, 3)[1] if bands else sosfilter.butter_band_sos(707.0, 1414.0, FS, 3)
        F = len(sos) if fan else 1
        moved = x.numel() * x.element_size() * (2 + F)             # x read by passes 1 and 3, y written once
        row = {"shape": label, "rows": R, "samples": T, "dtype": dtype, "filters": F, "sections": 3, "bank": fan, "reps": a.reps,
               "algorithmic_bytes": moved, "cells": {}}
        cells = [None] + [int(c) for c in a.cells.split(",") if c]
        for cell in cells:
            batch = sosfilter.SosBatch(sos, cell=cell)
            y = batch.run(x, fan=fan).y
            torch.cuda.synchronize()
            del y
            med, tmin, tmax = time_call(lambda: batch.run(x, fan=fan), a.reps)
            entry = {"median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "hbm_share": moved / med / HBM_PEAK}
            row["cells"][str(batch.cell)] = entry
            if cell is None:
                row["sos_batch"] = dict(entry, cell=batch.cell)
            del batch
            torch.cuda.empty_cache()
        if not a.no_routes and label == "a":
            edges = decay.band_edges(bands)[1]
            fir = [convolve.ConvolveBatch(decay.band_filter(lo, hi, FS)) for lo, hi in edges]

            def route():
                for c in fir:
                    c.run(x)
            route()
            torch.cuda.synchronize()
            med2, tmin, tmax = time_call(route, a.reps)
            row["fir_route"] = {"what": "six ConvolveBatch(band_filter(..)).run calls, handles made beforehand", "taps": [c.L for c in fir],
                                "median_ms": med2 * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3}
            row["fir_route_over_sos_batch"] = med2 * 1e3 / row["sos_batch"]["median_ms"]
            del fir
        if not a.no_routes and label == "b":
            try:
                from scipy.signal import sosfilt
            except ImportError:
                row["scipy_route"] = "not measured: scipy is not installed"
            else:
                one = x[0].cpu().numpy().astype(np.float64)
                t0 = time.perf_counter()
                ref = sosfilt(sos, one)
                dt = time.perf_counter() - t0
                got = sosfilter.SosBatch(sos).run(x[:1], dtype=torch.float64).y[0].cpu().numpy()
                row["scipy_route"] = {"what": "scipy.signal.sosfilt, float64, one host thread, ONE row timed once and multiplied by the row count: "
                                              "an extrapolation", "one_row_ms": dt * 1e3, "extrapolated_ms": dt * R * 1e3,
                                      "distance_row_0": float(np.abs(got - ref).max() / np.abs(ref).max())}
                row["scipy_route_over_sos_batch"] = dt * R * 1e3 / row["sos_batch"]["median_ms"]
        res["shapes"].append(row)
        del x
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
