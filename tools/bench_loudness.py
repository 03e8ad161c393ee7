"""LoudnessBatch (loudness.hip): BS.1770 / R 128 loudness and true peak of whole recordings.

Shapes: (a) 2 streams x 2^24 float32 samples (one stereo programme of 5.8 minutes); (b) 64 x 2^20 float32 (32 programmes);
(c) 8 x 2^22 float64.  Per shape: LoudnessBatch("stereo").run on a CUDA tensor between device events after a warm-up, with
and without the true peak, median / min / max of --reps calls; the bytes the algorithm must move (the samples, read once) as
a share of the 8 TB/s HBM peak; the interpolator's 4 * 32 + 1 fused multiply-adds per sample as a share of the 78.6 TFLOP/s
float64 vector peak (2 flops each).  Beside them, same session, same data: the peaks by the route a user has without the
class, Resampler(48000, 192000, zeros=16).run followed by abs().amax() (it writes and re-reads four times the recording), and
the K-weighting on the host, scipy.signal.lfilter twice plus the squares' sum on ONE stream (float64; best of --cpu-reps),
scaled by the stream count: an extrapolation, labelled as one.  Prints one JSON line and writes it to --out when given."""
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
SHAPES = [("a", 2, 1 << 24, "float32"), ("b", 64, 1 << 20, "float32"), ("c", 8, 1 << 22, "float64")]
STAGES = (((1.53512485958697, -2.69169618940638, 1.19839281085285), (1.0, -1.69065929318241, 0.73248077421585)),
          ((1.0, -2.0, 1.0), (1.0, -1.99004745483398, 0.99007225036621)))


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
    from friture_amd.loudness import LoudnessBatch
    from friture_amd.resample import Resampler
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_loudness", "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, S, T, dtype in SHAPES:
        if label not in a.shapes.split(","):
            continue
        x = 0.25 * torch.randn((S, T), device="cuda", dtype=getattr(torch, dtype), generator=g)
        row = {"shape": label, "streams": S, "samples": T, "dtype": dtype, "channels": "stereo", "tp_zeros": 16, "reps": a.reps}
        nbytes = S * T * x.element_size()
        for key, true_peak in (("with_true_peak", True), ("without_true_peak", False)):
            b = LoudnessBatch("stereo", true_peak=true_peak)
            first = b.run(x)
            torch.cuda.synchronize()
            row.setdefault("integrated_lufs", [float(v) for v in first.integrated[:2].cpu()])
            med, tmin, tmax = time_call(lambda: b.run(x), a.reps)
            row[key] = {"median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "algorithmic_bytes": nbytes,
                        "GBps": nbytes / med / 1e9, "hbm_share": nbytes / med / HBM_PEAK}
            if true_peak:
                fma = S * T * (4 * 2 * b.tp_zeros + 1)
                row[key].update({"fma": fma, "f64_TFLOPs": 2 * fma / med / 1e12, "f64_vector_share": 2 * fma / med / F64_VECTOR_PEAK})
            del first
        r = Resampler(48000, 192000, zeros=16)

        def route():
            return r.run(x, dtype=torch.float64).y.abs().amax(dim=1)
        peak = route()
        torch.cuda.synchronize()
        whole = LoudnessBatch("stereo").run(x).true_peak.amax(dim=1)
        row["resampler_route_same_peak"] = bool(torch.equal(peak, whole))
        del peak, whole
        med, tmin, tmax = time_call(route, a.reps)
        row["resampler_route"] = {"what": "Resampler(48000, 192000, zeros=16).run(x, dtype=float64).y.abs().amax(dim=1): the true peak alone",
                                  "median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3}
        row["resampler_route_over_true_peak_part"] = med * 1e3 / max(row["with_true_peak"]["median_ms"] - row["without_true_peak"]["median_ms"], 1e-9)
        if not a.gpu_only:
            from scipy.signal import lfilter
            x1 = x[0].double().cpu().numpy()
            best = None
            for _ in range(a.cpu_reps):
                t0 = time.perf_counter()
                y = x1
                for bq, aq in STAGES:
                    y = lfilter(bq, aq, y)
                np.sum((y[:T // 4800 * 4800] ** 2).reshape(-1, 4800), axis=1)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            row["host_lfilter_ms_extrapolated"] = best * S * 1e3
            row["host_lfilter_measured"] = f"1 stream (float64, scipy.signal.lfilter twice + sub-block sums, one thread of this host): {best * 1e3:.1f} ms, scaled by {S} streams"
            row["speedup_over_extrapolated_host_without_true_peak"] = best * S * 1e3 / row["without_true_peak"]["median_ms"]
        res["shapes"].append(row)
        del x
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
