"""DeconvolveBatch and rfft_rows (deconvolve.hip): deconvolution of sweep recordings by regularised spectral division.

Shapes: (a) 8 rows x 2^19 float32 samples against a sweep of 2^18 at n = 2^20 (a 5.4 s sweep at 48 kHz and as much room behind
it); (b) 64 x 2^16 float32, sweep 2^16, n = 2^17; (c) 1 x 2^23 float64, sweep 2^22, n = 2^24.  Per shape:
DeconvolveBatch(sweep, n, 1e-6).run on a CUDA tensor between device events after a warm-up, median / min / max of --reps calls,
and the bytes its five passes must move (the rows read once, every scratch row written and read once, G read once per row, h
written once) as a share of the 8 TB/s HBM peak.  Beside it, same session, same data, what a user writes without the class:
torch.fft.rfft of the rows and of the sweep, the regularised division and torch.fft.irfft, in float64 on the device (the class
transforms its sweep once, at creation: the route with the sweep's inverse spectrum made ahead is timed too).  rfft_rows alone
beside torch.fft.rfft.  Also the largest distance between the two results in units of max |h|.  Prints one JSON line and
writes it to --out when given; --no-routes runs the class alone (for a kernel trace)."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = [("a", 8, 1 << 19, "float32", 1 << 18, 1 << 20), ("b", 64, 1 << 16, "float32", 1 << 16, 1 << 17),
          ("c", 1, 1 << 23, "float64", 1 << 22, 1 << 24)]
REG = 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--no-routes", action="store_true", help="DeconvolveBatch and rfft_rows alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.deconvolve import DeconvolveBatch, exp_sweep, rfft_rows
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_deconvolve", "reg": REG, "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, S, T, dtype, Lx, n in SHAPES:
        if label not in a.shapes.split(","):
            continue
        sweep = exp_sweep(20.0, 20000.0, Lx, fade=480)
        y = 0.25 * torch.randn((S, T), device="cuda", dtype=getattr(torch, dtype), generator=g)
        row = {"shape": label, "rows": S, "samples": T, "dtype": dtype, "sweep": Lx, "n": n, "reps": a.reps}
        Mc = n // 2
        db = DeconvolveBatch(sweep, n=n, reg=REG)
        h = db.run(y).h
        torch.cuda.synchronize()
        med, tmin, tmax = time_call(lambda: db.run(y), a.reps)
        # column pass (rows in, A out), row pass (A, Z), pair (Z and G in, W out), column pass (W, Z), row pass (Z in, h out)
        nbytes = S * (T * y.element_size() + 7 * Mc * 16 + (Mc + 1) * 16 + n * 8)
        row["deconvolve_batch"] = {"median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "pass_bytes": nbytes,
                                   "hbm_share": nbytes / med / HBM_PEAK}
        spec = rfft_rows(y, n)
        torch.cuda.synchronize()
        med_r, tmin, tmax = time_call(lambda: rfft_rows(y, n), a.reps)
        fbytes = S * (T * y.element_size() + 5 * Mc * 16 + (Mc + 1) * 16)
        row["rfft_rows"] = {"median_ms": med_r * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "pass_bytes": fbytes,
                            "hbm_share": fbytes / med_r / HBM_PEAK}
        if not a.no_routes:
            xd = torch.from_numpy(sweep).cuda()

            def inverse_spectrum():
                X = torch.fft.rfft(xd, n)
                P = X.real * X.real + X.imag * X.imag
                return X.conj() / (P + REG * P.max())

            def route():
                return torch.fft.irfft(torch.fft.rfft(y.double(), n) * inverse_spectrum(), n)

            G = inverse_spectrum()

            def route_ahead():
                return torch.fft.irfft(torch.fft.rfft(y.double(), n) * G, n)

            def forward():
                return torch.fft.rfft(y.double(), n)

            full = route()
            torch.cuda.synchronize()
            row["distance_to_torch_route"] = float((h - full).abs().max()) / float(full.abs().max())
            row["rfft_distance_to_torch"] = float((spec - forward()).abs().max()) / float(spec.abs().max())
            del full
            for name, fn, what in (("torch_route", route, "torch.fft.rfft of the rows and the sweep, the division, torch.fft.irfft: float64, on the device"),
                                   ("torch_route_sweep_ahead", route_ahead, "the same with the sweep's inverse spectrum made ahead"),
                                   ("torch_rfft", forward, "torch.fft.rfft(y.double(), n)")):
                fn()
                torch.cuda.synchronize()
                m, lo, hi = time_call(fn, a.reps)
                row[name] = {"what": what, "median_ms": m * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3}
            row["torch_route_over_deconvolve_batch"] = row["torch_route"]["median_ms"] / (med * 1e3)
            row["torch_route_sweep_ahead_over_deconvolve_batch"] = row["torch_route_sweep_ahead"]["median_ms"] / (med * 1e3)
            row["torch_rfft_over_rfft_rows"] = row["torch_rfft"]["median_ms"] / (med_r * 1e3)
            del G, xd
        res["shapes"].append(row)
        del y, h, spec, db
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
