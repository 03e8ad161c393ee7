"""Resampler (resample.hip): whole recordings from another sample rate to 48 kHz.

Shapes: (a) 8 streams x 2^22 float32 samples at 44100 Hz (L 160, M 147, K 129); (b) 64 x 2^20 float32 at 44100 Hz; (c) 8 x 2^22
float64 at 96000 Hz (L 1, M 2, K 257).  Per shape: Resampler.run on a CUDA tensor between device events after a warm-up, median
/ min / max of --reps calls; the bytes the algorithm must move (samples read plus samples written, in their dtypes) as a share
of the 8 TB/s HBM peak; n_out * K fused multiply-adds per stream as a share of the 78.6 TFLOP/s float64 vector peak (2 flops
each).  The CPU figure is scipy.signal.resample_poly with the same prototype on ONE stream (float64; best of --cpu-reps), scaled
by the stream count: an extrapolation, labelled as one.  Prints one JSON line and writes it to --out when given."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

F64_VECTOR_PEAK = 78.6e12
SHAPES = [("a", 8, 1 << 22, "float32", 44100), ("b", 64, 1 << 20, "float32", 44100), ("c", 8, 1 << 22, "float64", 96000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.resample import Resampler
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_resample", "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, S, T, dtype, rate in SHAPES:
        if label not in a.shapes.split(","):
            continue
        x = 0.25 * torch.randn((S, T), device="cuda", dtype=getattr(torch, dtype), generator=g)
        r = Resampler(rate)
        y = r.run(x).y
        torch.cuda.synchronize()
        n_out = y.shape[1]
        del y
        med, tmin, tmax = time_call(lambda: r.run(x), a.reps)
        nbytes = S * (T + n_out) * x.element_size()
        fma = S * n_out * r.K
        row = {"shape": label, "streams": S, "samples": T, "dtype": dtype, "rate_in": rate, "L": r.L, "M": r.M, "K": r.K,
               "outputs": n_out, "median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "reps": a.reps,
               "algorithmic_bytes": nbytes, "GBps": nbytes / med / 1e9, "hbm_share": nbytes / med / HBM_PEAK,
               "fma": fma, "f64_TFLOPs": 2 * fma / med / 1e12, "f64_vector_share": 2 * fma / med / F64_VECTOR_PEAK}
        if not a.gpu_only:
            from scipy.signal import resample_poly
            x1 = x[0].double().cpu().numpy()
            best = None
            for _ in range(a.cpu_reps):
                t0 = time.perf_counter()
                resample_poly(x1, r.L, r.M, window=r.prototype / r.L)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            row["scipy_resample_poly_ms_extrapolated"] = best * S * 1e3
            row["scipy_resample_poly_measured"] = f"1 stream (float64, one thread of this host): {best * 1e3:.1f} ms, scaled by {S} streams"
            row["speedup_over_extrapolated_scipy"] = best * S / med
        res["shapes"].append(row)
        del x
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
