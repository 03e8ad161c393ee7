"""ConvolveBatch (convolve.hip): partitioned FFT convolution of whole recordings with a long FIR.

Shapes: (a) 8 streams x 2^22 float32 samples, L = 65536 taps (a 1.4 s room response at 48 kHz); (b) 64 x 2^20 float32,
L = 4096; (c) 1 x 2^24 float64, L = 262144.  Per shape: ConvolveBatch(h).run on a CUDA tensor (one flushed call) between device
events after a warm-up, median / min / max of --reps calls; the complex multiply-adds of the partition sums, 8 flops each, as a
share of the 78.6 TFLOP/s float64 vector peak; the bytes the algorithm must move (the rows read and the outputs written once) as
a share of the 8 TB/s HBM peak.  Beside them, same session, same data, what a user does without the class: one full-length
torch.fft.rfft / multiply / irfft in float64 on the device; and scipy.signal.oaconvolve on one host thread, timed once on ONE
stream and multiplied by the stream count: an extrapolation, not a measurement of the batch.  Also the largest distance
between the class and the full-length transform in units of max|x| sum|h|, and on shape (a) block 2048 against 4096, the
figures behind the default's upper clamp.  Prints one JSON line and writes it to --out when given."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

F64_VECTOR_PEAK = 78.6e12
SHAPES = [("a", 8, 1 << 22, "float32", 65536), ("b", 64, 1 << 20, "float32", 4096), ("c", 1, 1 << 24, "float64", 262144)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--no-host", action="store_true", help="leave out scipy.signal.oaconvolve on the host")
    ap.add_argument("--no-routes", action="store_true", help="ConvolveBatch alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from friture_amd import _lib
    from friture_amd.convolve import ConvolveBatch
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_convolve", "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, S, T, dtype, L in SHAPES:
        if label not in a.shapes.split(","):
            continue
        x = 0.25 * torch.randn((S, T), device="cuda", dtype=getattr(torch, dtype), generator=g)
        h = np.random.default_rng(L).standard_normal(L) * np.exp(-6.0 * np.arange(L) / L)
        row = {"shape": label, "streams": S, "samples": T, "dtype": dtype, "taps": L, "reps": a.reps}

        def measure(block):
            b = ConvolveBatch(h, block)
            y = b.run(x).y
            torch.cuda.synchronize()
            med, tmin, tmax = time_call(lambda: b.run(x), a.reps)
            blocks = -(-(T + L - 1) // b.block)
            flops = S * blocks * b.partitions * (b.block + 1) * 8.0
            nbytes = x.numel() * x.element_size() + y.numel() * y.element_size()
            return y, {"block": b.block, "partitions": b.partitions, "median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3,
                       "f64_TFLOPs": flops / med / 1e12, "f64_vector_share": flops / med / F64_VECTOR_PEAK, "algorithmic_bytes": nbytes,
                       "hbm_share": nbytes / med / HBM_PEAK}

        y, row["convolve_batch"] = measure(None)
        if label == "a" and not a.no_routes:
            for block in (2048, 4096):
                row[f"block_{block}"] = measure(block)[1]
        if not a.no_routes:
            n = 1 << (T + L - 2).bit_length()
            hd = torch.from_numpy(h).cuda()

            def route():
                return torch.fft.irfft(torch.fft.rfft(x.double(), n) * torch.fft.rfft(hd, n), n)[:, :T + L - 1]
            full = route()
            torch.cuda.synchronize()
            scale = float(x.abs().max()) * float(np.sum(np.abs(h)))
            row["distance_to_full_length_transform"] = float((y.double() - full).abs().max()) / scale
            del full
            med2, tmin, tmax = time_call(route, a.reps)
            row["full_length_fft"] = {"what": f"torch.fft.rfft / multiply / irfft at {n} points in float64 on the device",
                                      "median_ms": med2 * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3}
            row["full_length_fft_over_convolve_batch"] = med2 / row["convolve_batch"]["median_ms"] * 1e3
        del y
        if not a.no_host and not a.no_routes:
            try:
                from scipy.signal import oaconvolve
            except ImportError:
                row["host_oaconvolve"] = None
            else:
                one = x[0].cpu().numpy().astype(np.float64)
                t0 = time.perf_counter()
                oaconvolve(one, h)
                dt = time.perf_counter() - t0
                row["host_oaconvolve"] = {"what": "scipy.signal.oaconvolve, float64, one host thread, ONE stream timed once and multiplied by the "
                                                  "stream count: an extrapolation", "one_stream_ms": dt * 1e3, "extrapolated_ms": dt * S * 1e3}
                row["host_oaconvolve_over_convolve_batch"] = dt * S * 1e3 / row["convolve_batch"]["median_ms"]
        res["shapes"].append(row)
        del x
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
