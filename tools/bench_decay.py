"""DecayBatch (decay.hip): reverberation times and clarity of whole batches of impulse responses.

Shapes: (a) 640 rows x 2^17 float64 (64 responses x 10 bands of 2.7 s at 48 kHz); (b) 248 rows x 2^18 float32; (c) 1 row x 2^20
float64.  The rows are decaying Gaussian noise over a stationary floor, made on the device.  Per shape: DecayBatch().run on a
CUDA tensor between device events after a warm-up, median / min / max of --reps calls, once with the parameters alone and once
with the curve at step 48; the bytes the algorithm must move (the samples read once plus the curve written) as a share of the
8 TB/s HBM peak, and the same share on two reads of the samples, the floor of any kernel whose thresholds need the row's total.
Beside them, same session, same data: the torch composition a user writes without the class, given the onsets and truncations
the class found so that the values match (square, flip, cumsum, flip, log10, masks, masked sums; its largest distance from the
class's T30 and C80 is reported); and the numpy restatement of tests/decay_helpers.py on ONE row, multiplied by the row
count: an extrapolation, not a measurement of the batch.  Prints one JSON line and writes it to --out when given."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

FS = 48000
SHAPES = [("a", 640, 1 << 17, "float64"), ("b", 248, 1 << 18, "float32"), ("c", 1, 1 << 20, "float64")]
RANGES = ((0.0, -10.0), (-5.0, -15.0), (-5.0, -25.0), (-5.0, -35.0))


def torch_route(x, t0, t1):
    """EDT / T10 / T20 / T30 [R, 4], C50, C80, D50, Ts of rows x with the onsets t0 and truncations t1, in full-size passes."""
    import torch
    T = x.shape[1]
    idx = torch.arange(T, device=x.device)
    inside = (idx >= t0[:, None]) & (idx < t1[:, None])
    e = x.double().square() * inside
    E = e.flip(1).cumsum(1).flip(1)
    E0 = E.gather(1, t0[:, None])
    L = 10 * torch.log10(E / E0)
    times = []
    for hi, lo in RANGES:
        a = (inside & (L > hi)).sum(1) if hi else torch.zeros_like(t0)
        m = inside & (L > lo) & ((L <= hi) if hi else inside)
        n = m.sum(1).double()
        k = (idx - t0[:, None] - a[:, None]).double()
        Lm = torch.where(m, L, torch.zeros_like(L))
        SL, SkL = Lm.sum(1), (k * Lm).sum(1)
        Sk, vk = n * (n - 1) / 2, n * n * (n * n - 1) / 12
        rt = -60 / ((n * SkL - Sk * SL) / vk * FS)
        reached = (inside & (L <= lo)).any(1)
        times.append(torch.where(reached, rt, torch.full_like(rt, float("nan"))))

    def at(n):
        u = t0 + n
        return torch.where(u < t1, E.gather(1, u.clamp(max=T - 1)[:, None])[:, 0], torch.zeros(len(u), dtype=E.dtype, device=E.device))
    E0 = E0[:, 0]
    E50, E80 = at(round(0.05 * FS)), at(round(0.08 * FS))
    ts = ((idx - t0[:, None]).double() * e).sum(1) / E0 / FS
    return torch.stack(times, 1), 10 * torch.log10((E0 - E50) / E50), 10 * torch.log10((E0 - E80) / E80), (E0 - E50) / E0, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--no-host", action="store_true", help="leave out the numpy restatement on the host")
    ap.add_argument("--no-routes", action="store_true", help="DecayBatch alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from friture_amd import _lib
    from friture_amd.decay import DecayBatch
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_decay", "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, R, T, dtype in SHAPES:
        if label not in a.shapes.split(","):
            continue
        t = torch.arange(T, device="cuda", dtype=torch.float64) / FS
        rt = torch.linspace(0.25, 0.6, R, device="cuda", dtype=torch.float64)[:, None] * (T / FS) / 2.7
        x = torch.randn((R, T), device="cuda", dtype=torch.float64, generator=g) * 10.0 ** (-3.0 * t / rt)
        x = (x + 1e-4 * torch.randn((R, T), device="cuda", dtype=torch.float64, generator=g)).to(getattr(torch, dtype))
        del t
        db = DecayBatch()
        row = {"shape": label, "rows": R, "samples": T, "dtype": dtype, "reps": a.reps}
        samples = x.numel() * x.element_size()
        for name, kw in (("params", {}), ("params_and_curve", {"keep": ("params", "curve"), "curve_step": 48})):
            out = db.run(x, **kw)
            torch.cuda.synchronize()
            med, tmin, tmax = time_call(lambda: db.run(x, **kw), a.reps)
            curve = 0 if out.curve is None else out.curve.numel() * 8
            row[name] = {"median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "algorithmic_bytes": samples + curve,
                         "hbm_share": (samples + curve) / med / HBM_PEAK, "hbm_share_two_reads": (2 * samples + curve) / med / HBM_PEAK}
        row["truncation_over_samples"] = float((out.truncation - out.onset).double().mean()) / T
        row["t30_s"] = [float(out.t30.min()), float(out.t30.max())]
        if not a.no_routes:
            times, c50, c80, d50, ts = torch_route(x, out.onset, out.truncation)
            torch.cuda.synchronize()
            row["torch_route_distance"] = {"t30_relative": float(((times[:, 3] - out.t30) / out.t30).abs().max()),
                                           "c80_db": float((c80 - out.c80).abs().max())}
            del times, c50, c80, d50, ts
            med2, tmin, tmax = time_call(lambda: torch_route(x, out.onset, out.truncation), a.reps)
            row["torch_route"] = {"what": "square, flip, cumsum, flip, log10, masks, masked sums in float64 on the device, onsets and truncations given",
                                  "median_ms": med2 * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3}
            row["torch_route_over_decay_batch"] = med2 * 1e3 / row["params"]["median_ms"]
        if not a.no_host and not a.no_routes:
            import decay_helpers
            one = x[0].cpu().numpy()
            t0 = time.perf_counter()
            ref = decay_helpers.restate(one)
            dt = time.perf_counter() - t0
            row["host_restatement"] = {"what": "the numpy restatement (tests/decay_helpers.py), float64, one host thread, ONE row timed once and "
                                               "multiplied by the row count: an extrapolation", "one_row_ms": dt * 1e3, "extrapolated_ms": dt * R * 1e3,
                                       "t30_relative_distance_row_0": abs(float(ref["t30"]) - float(out.t30[0])) / float(ref["t30"])}
            row["host_restatement_over_decay_batch"] = dt * R * 1e3 / row["params"]["median_ms"]
        res["shapes"].append(row)
        del x, out
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
