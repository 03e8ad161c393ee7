"""TransferBatch (transfer.hip): Welch cross-spectra, H1 and coherence of whole two-row recordings.

Shapes: (a) 8 pairs x 2^22 float32 samples at the defaults (N = 8192, hop 4096); (b) 64 pairs x 2^20 float32 at N = 1024
(hop 512); (c) 1 pair x 2^24 float64 at the defaults.  Per shape: TransferBatch(...).run on a CUDA tensor between device events
after a warm-up, the running estimate, median / min / max of --reps calls; the bytes the algorithm must move (both rows, read
once) as a share of the 8 TB/s HBM peak; the transform's 5 N log2 N flops per frame as a share of the 78.6 TFLOP/s float64
vector peak.  Beside them, same session, same data: what a user does without the class, torch.stft of both rows (in the
input's precision, complex spectrograms in HBM), the products and their means, h1 and the coherence; and the largest
distance between the two routes' h1.  Prints one JSON line and writes it to --out when given."""
from __future__ import annotations

import argparse
import math
import sys
from pathlib import Path

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

F64_VECTOR_PEAK = 78.6e12
SHAPES = [("a", 8, 1 << 22, "float32", 8192), ("b", 64, 1 << 20, "float32", 1024), ("c", 1, 1 << 24, "float64", 8192)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.transfer import TransferBatch
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_transfer", "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, S, T, dtype, N in SHAPES:
        if label not in a.shapes.split(","):
            continue
        x = 0.25 * torch.randn((S, 2, T), device="cuda", dtype=getattr(torch, dtype), generator=g)
        x[:, 1] = 0.5 * x[:, 0] + 0.3 * torch.roll(x[:, 0], 1, -1) + 0.1 * x[:, 1]
        b = TransferBatch(N)
        frames = b.frames_after(T)
        row = {"shape": label, "pairs": S, "samples": T, "dtype": dtype, "fft_size": N, "hop": b.hop, "frames": frames, "reps": a.reps}
        first = b.run(x)
        torch.cuda.synchronize()
        med, tmin, tmax = time_call(lambda: b.run(x), a.reps)
        nbytes, flops = x.numel() * x.element_size(), S * frames * 5 * N * math.log2(N)
        row["transfer_batch"] = {"median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "algorithmic_bytes": nbytes,
                                 "GBps": nbytes / med / 1e9, "hbm_share": nbytes / med / HBM_PEAK, "f64_TFLOPs": flops / med / 1e12,
                                 "f64_vector_share": flops / med / F64_VECTOR_PEAK}
        w = torch.from_numpy(b.window).to(device="cuda", dtype=x.dtype)

        def route():
            X = torch.stft(x[:, 0], N, hop_length=b.hop, window=w, center=False, return_complex=True) / N
            Y = torch.stft(x[:, 1], N, hop_length=b.hop, window=w, center=False, return_complex=True) / N
            sxx, syy, sxy = (X.abs() ** 2).mean(-1), (Y.abs() ** 2).mean(-1), (X.conj() * Y).mean(-1)
            return sxy / sxx, sxy.abs() ** 2 / (sxx * syy)
        h1, _ = route()
        torch.cuda.synchronize()
        row["stft_route_h1_distance"] = float((h1 - first.h1[:, 0]).abs().max() / first.h1.abs().max())
        del h1, first
        med2, tmin, tmax = time_call(route, a.reps)
        row["stft_route"] = {"what": f"torch.stft of both rows ({dtype}), |X|^2, |Y|^2, conj(X) Y, means over the frames, h1, coherence",
                             "median_ms": med2 * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3}
        row["stft_route_over_transfer_batch"] = med2 / med
        res["shapes"].append(row)
        del x
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
