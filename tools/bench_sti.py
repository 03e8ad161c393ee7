"""MtfBatch (mtf.hip): the modulation transfer of whole batches of impulse responses at the 14 modulation frequencies of the STI.

Shapes: (a) 448 rows x 2^17 float64 (64 responses x 7 octave bands of 2.7 s at 48 kHz); (b) 1792 rows x 2^16 float32; (c) 1 row x
2^24 float32.  The rows are decaying Gaussian noise, made on the device.  Per shape: MtfBatch().run on a CUDA tensor between device
events after a warm-up, median / min / max of --reps calls; the bytes the algorithm must move (the samples, read once) as a share
of the 8 TB/s HBM peak, and the float64 operations it must do (4 nf per sample: a real-times-complex multiply-add per frequency)
per second.  Beside them, same session, same data: the torch composition a user writes without the class, x.double().square()
times a [T, nf] complex128 phasor matrix made ahead (its largest distance from the class's m is reported; the matrix is made with
torch's float64 sincos of the unreduced phase, which is what costs it accuracy at 2^24); and the numpy restatement of
tests/sti_helpers.py on ONE row, multiplied by the row count: an extrapolation, not a measurement of the batch.  sti_from_mtf on
the 64 x 7 x 14 values of shape (a) is timed as well.  Prints one JSON line and writes it to --out when given."""
from __future__ import annotations

import argparse
import math
import sys
import time
from pathlib import Path

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

FS = 48000
SHAPES = [("a", 448, 1 << 17, "float64"), ("b", 1792, 1 << 16, "float32"), ("c", 1, 1 << 24, "float32")]


def torch_route(x, phasor):
    """m [R, nf] of rows x: the squares as one matrix product with the phasor matrix [T, nf] complex128."""
    import torch
    e = x.double().square()
    S = torch.matmul(e.to(torch.complex128), phasor)
    return S.abs() / e.sum(1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--no-host", action="store_true", help="leave out the numpy restatement on the host")
    ap.add_argument("--no-routes", action="store_true", help="MtfBatch alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from friture_amd import _lib
    from friture_amd.sti import MOD_FREQS, MtfBatch, sti_from_mtf
    torch.cuda.set_device(0)
    _lib.init(0)
    nf = len(MOD_FREQS)
    res = {"tool": "bench_sti", "modulation_frequencies": nf, "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, R, T, dtype in SHAPES:
        if label not in a.shapes.split(","):
            continue
        t = torch.arange(T, device="cuda", dtype=torch.float64) / FS
        rt = torch.linspace(0.25, 0.6, R, device="cuda", dtype=torch.float64)[:, None] * (T / FS) / 2.7
        x = (torch.randn((R, T), device="cuda", dtype=torch.float64, generator=g) * 10.0 ** (-3.0 * t / rt)).to(getattr(torch, dtype))
        mb = MtfBatch()
        row = {"shape": label, "rows": R, "samples": T, "dtype": dtype, "reps": a.reps}
        out = mb.run(x)
        torch.cuda.synchronize()
        med, tmin, tmax = time_call(lambda: mb.run(x), a.reps)
        samples, flops = x.numel() * x.element_size(), 4 * nf * x.numel()
        row["mtf_batch"] = {"median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "algorithmic_bytes": samples,
                            "hbm_share": samples / med / HBM_PEAK, "float64_operations": flops, "tflops_float64": flops / med / 1e12}
        row["m_range"] = [float(out.m.min()), float(out.m.max())]
        if label == "a":
            m = out.m.reshape(R // 7, 7, nf).contiguous()
            sti_from_mtf(m)
            torch.cuda.synchronize()
            med_i, imin, imax = time_call(lambda: sti_from_mtf(m), a.reps)
            row["sti_from_mtf"] = {"responses": R // 7, "median_ms": med_i * 1e3, "min_ms": imin * 1e3, "max_ms": imax * 1e3}
        if not a.no_routes:
            phasor = torch.exp(-2j * math.pi * t[:, None] * torch.tensor(MOD_FREQS, device="cuda", dtype=torch.float64)[None, :])
            m2 = torch_route(x, phasor)
            torch.cuda.synchronize()
            row["torch_route_distance"] = float((m2 - out.m).abs().max())
            del m2
            med2, tmin, tmax = time_call(lambda: torch_route(x, phasor), a.reps)
            row["torch_route"] = {"what": "x.double().square() as complex128 times a [T, nf] complex128 phasor matrix made ahead, abs, over the row sums",
                                  "median_ms": med2 * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3}
            row["torch_route_over_mtf_batch"] = med2 / med
            del phasor
        if not a.no_host and not a.no_routes:
            import sti_helpers
            n = min(T, 1 << 20)                                      # the phasors of a longer row do not fit a host's patience
            one = x[:1, :n].cpu().numpy()
            sti_helpers.restate_mtf(one[:, :1024])
            t0 = time.perf_counter()
            ref_m, _ = sti_helpers.restate_mtf(one)
            dt = time.perf_counter() - t0
            row["host_restatement"] = {"what": "the numpy restatement (tests/sti_helpers.py), float64 sums, the phasors reduced in longdouble within the timed call, one "
                                               "host thread, the first min(T, 2^20) samples of ONE row timed once and scaled to the batch's samples: an extrapolation",
                                       "samples_timed": n, "timed_ms": dt * 1e3, "extrapolated_ms": dt * R * (T / n) * 1e3}
            if n == T:
                row["host_restatement"]["m_distance_row_0"] = float(np.abs(ref_m[0] - out.m[0].cpu().numpy()).max())
            row["host_restatement_over_mtf_batch"] = dt * R * (T / n) / med
        res["shapes"].append(row)
        del x, out, t
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
