"""SpatialBatch (spatial.hip): inter-aural cross-correlation of whole batches of binaural impulse responses.

Shapes: (a) 640 pairs x 2^17 float64 (64 heads x 10 bands of 2.7 s at 48 kHz), the defaults (max_lag 48: 97 lags; windows early,
late, whole); (b) 8 pairs x 2^22 float32, the defaults; (c) 1 pair x 2^24 float32 at max_lag=128 (257 lags).  The pairs are decaying
Gaussian noise with a shared component, made on the device.  Per shape: SpatialBatch.run on a CUDA tensor between device events
after a warm-up, median / min / max of --reps calls; the multiply-adds the definition needs, (2 M + 1) per sample of the windows'
union (from the onsets the class found), over the call time as a share of the float64 vector peak (64 multiply-adds per clock
and CU, the CU count from the device, at the 2.4 GHz the part is specified for: a share of a nominal peak, the clock held under
this load is not measured here); and one read of both rows as a share of the 8 TB/s HBM peak.  These are whole-call figures
(five kernels, the staging of the outputs), not the correlation kernel's own share.  Beside them, same session, same data: the
torch composition a user writes without the class, given the onsets: per window a masked copy of l, then 2 M + 1 shifted products
with the zero-extended r and their sums, in float64 on the device (its largest distance from the class's iacc is reported).
Prints one JSON line and writes it to --out when given."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FS = 48000
CLOCK_HZ, FMA_PER_CLOCK_AND_CU = 2.4e9, 64
SHAPES = [("a", 640, 1 << 17, "float64", None), ("b", 8, 1 << 22, "float32", None), ("c", 1, 1 << 24, "float32", 128)]


def torch_route(x, t0, windows, M):
    """iacc [S, W] of pairs x [S, 2, T] with the onsets t0 and windows in samples (b = -1: to the end), in full-size passes."""
    import torch
    S, _, T = x.shape
    idx = torch.arange(T, device=x.device)
    l = x[:, 0].double()
    rz = torch.nn.functional.pad(x[:, 1].double(), (M, M))
    out = []
    for a, b in windows:
        A = (t0 + a).clamp(max=T)
        B = torch.full_like(t0, T) if b < 0 else (t0 + b).clamp(max=T)
        inside = (idx >= A[:, None]) & (idx < B[:, None])
        lw = l * inside
        El, Er = (lw * lw).sum(1), (rz[:, M:M + T].square() * inside).sum(1)
        C = torch.stack([(lw * rz[:, k:k + T]).sum(1) for k in range(2 * M + 1)], 1)
        out.append((C / (El * Er).sqrt()[:, None]).abs().amax(1))
    return torch.stack(out, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--no-routes", action="store_true", help="SpatialBatch alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.spatial import SpatialBatch
    torch.cuda.set_device(0)
    _lib.init(0)
    ncu, _ = _lib.device_info(0)
    fma_peak = ncu * FMA_PER_CLOCK_AND_CU * CLOCK_HZ
    res = {"tool": "bench_spatial", "compute_units": ncu, "fma_peak_per_s": fma_peak,
           "fma_peak_is": "64 float64 multiply-adds per clock and CU at a nominal 2.4 GHz; the clock held under load was not measured", "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, S, T, dtype, max_lag in SHAPES:
        if label not in a.shapes.split(","):
            continue
        t = torch.arange(T, device="cuda", dtype=torch.float64) / FS
        env = 10.0 ** (-3.0 * t / (0.45 * (T / FS) / 2.7))
        common = torch.randn((S, 1, T + 8), device="cuda", dtype=torch.float64, generator=g)
        x = 0.4 * torch.randn((S, 2, T), device="cuda", dtype=torch.float64, generator=g)
        x[:, 0] += 0.6 * common[:, 0, 8:]
        x[:, 1] += 0.6 * common[:, 0, 3:T + 3]                          # the shared component reaches r five samples late
        x = (x * env).to(getattr(torch, dtype))
        del t, env, common
        sb = SpatialBatch() if max_lag is None else SpatialBatch(max_lag=max_lag)
        M = sb.max_lag
        out = sb.run(x)
        torch.cuda.synchronize()
        med, tmin, tmax = time_call(lambda: sb.run(x), a.reps)
        union = int((T - out.onset - min(w[0] for w in sb.windows)).clamp(min=0).sum())      # the defaults' windows cover [t0, T)
        fmas, samples = (2 * M + 1) * union, x.numel() * x.element_size()
        row = {"shape": label, "pairs": S, "samples": T, "dtype": dtype, "max_lag": M, "lags": 2 * M + 1, "windows": len(sb.windows), "reps": a.reps,
               "run": {"median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "multiply_adds": fmas, "algorithmic_bytes": samples,
                       "fp64_share": fmas / med / fma_peak, "hbm_share": samples / med / HBM_PEAK},
               "iacc_early": [float(out.iacc[:, 0].min()), float(out.iacc[:, 0].max())]}
        if not a.no_routes:
            theirs = torch_route(x, out.onset, sb.windows, M)
            torch.cuda.synchronize()
            row["torch_route_distance"] = {"iacc": float((theirs - out.iacc).abs().max())}
            del theirs
            med2, tmin, tmax = time_call(lambda: torch_route(x, out.onset, sb.windows, M), a.reps)
            row["torch_route"] = {"what": "per window a masked copy of l, then 2 M + 1 shifted products with the zero-extended r and their sums, "
                                          "float64 on the device, onsets given", "median_ms": med2 * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3}
            row["torch_route_over_spatial_batch"] = med2 / med
        res["shapes"].append(row)
        del x, out
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
