"""PitchBatch (pitchbatch.hip around the kernels of pitch.hip): whole recordings through the pitch tracker widget's chain.

Shapes: (a) 8 streams x 2^22 float64 samples at the defaults (fft_size 4096, 75 % overlap, 512-sample chunks, 10 s curve);
(b) 64 streams x 2^20 float32; (c) 8 streams x 2 rows x 2^22 float64.  Per shape: the batch call (device events around
PitchBatch.run on a CUDA tensor after a warm-up, median / min / max of --reps); for the one-row shapes PitchEngine.track on the same
samples (widened to float64 ahead of the clock) in the same session, timed the same way — the difference is what the level over
rows, the gate hand-over, the read-out and the state cost, to be read against track's own spread; the chunk-by-chunk route —
PitchTracker.update() per 512-sample chunk pushed into a ring, ONE stream, the first --route-chunks chunks, host clock (every
update ends in a synchronisation), scaled linearly to all chunks and streams; for the two-row shape also today's
PitchTracker._run (raw estimates from the device, the gate in a host loop over frames) on one stream, scaled by the streams.
Prints one JSON line and writes it to --out when given."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

from benchutil import emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = [("a", 8, 1, 1 << 22, "float64"), ("b", 64, 1, 1 << 20, "float32"), ("c", 8, 2, 1 << 22, "float64")]


def signal(torch, S, rows, T, dtype, seed):
    """Harmonic tones whose pitch wanders, one per row, with a little noise: frames that pass the gate and frames that do not."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(T, device="cuda", dtype=torch.float64)
    f0 = 110.0 * 2 ** (3 * torch.rand((S * rows, 1), device="cuda", dtype=torch.float64, generator=g))
    phase = 2 * np.pi * f0 * (t / 48000.0) * (1 + 0.02 * torch.sin(2 * np.pi * 0.3 * t / 48000.0))
    x = 0.2 * (torch.sin(phase) + 0.5 * torch.sin(2 * phase)) * (torch.sin(2 * np.pi * 0.11 * t / 48000.0) > -0.5)
    x += 1e-3 * torch.randn((S * rows, T), device="cuda", dtype=torch.float64, generator=g)
    x = x.reshape((S, rows, T) if rows > 1 else (S, T))
    return x.to(getattr(torch, dtype)).contiguous()


def route_chunks(pt, x1, n_chunks, chunk=512):
    """Seconds for the first n_chunks chunks of one stream ([rows, T] float64 numpy) through PitchTracker.update()."""
    from friture_amd.ringbuffer import RingBuffer
    best = None
    for _ in range(2):
        ring = RingBuffer()
        ring.push(x1[:, :0])
        tracker = pt.PitchTracker(ring)
        tracker.update()
        t0 = time.perf_counter()
        for c in range(n_chunks):
            ring.push(x1[:, c * chunk:(c + 1) * chunk])
            tracker.update()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--route-chunks", type=int, default=256)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd import pitch_tracker as pt
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_pitchbatch", "shapes": []}
    for label, S, rows, T, dtype in SHAPES:
        if label not in a.shapes.split(","):
            continue
        x = signal(torch, S, rows, T, dtype, 7)
        pb = pt.PitchBatch(dual_channels=rows == 2)
        r = pb.run(x)
        torch.cuda.synchronize()
        F, R = r.estimates.shape[1], len(r.refresh_chunk)
        voiced = float((~torch.isnan(r.estimates)).double().mean())
        del r
        med, tmin, tmax = time_call(lambda: pb.run(x), a.reps)
        row = {"shape": label, "streams": S, "rows": rows, "samples": T, "dtype": dtype, "fft_size": pb.fft_size, "frames": F,
               "refreshes": R, "history": pb.n_history, "voiced_share": voiced, "reps": a.reps,
               "batch_median_ms": med * 1e3, "batch_min_ms": tmin * 1e3, "batch_max_ms": tmax * 1e3}
        if rows == 1:
            xd = x.double().contiguous()
            eng = pt.PitchEngine(pb.fft_size, pb.step, S)
            eng.track(xd)
            torch.cuda.synchronize()
            tm, t0, t1 = time_call(lambda: eng.track(xd), a.reps)
            row.update({"track_median_ms": tm * 1e3, "track_min_ms": t0 * 1e3, "track_max_ms": t1 * 1e3,
                        "batch_minus_track_ms": (med - tm) * 1e3, "track_spread_ms": (t1 - t0) * 1e3,
                        "batch_within_track_spread": bool(med - tm <= t1 - t0)})
            del xd, eng
        if not a.batch_only:
            x1 = x[0].double().cpu().numpy().reshape(rows, T)
            nc = min(a.route_chunks, T // 512)
            dt = route_chunks(pt, x1, nc)
            scaled = dt / nc * (T // 512) * S
            row["chunk_route_ms_scaled"] = scaled * 1e3
            row["chunk_route_measured"] = f"1 stream, first {nc} chunks: {dt * 1e3:.1f} ms, scaled by {T // 512}/{nc} x {S} streams"
            row["batch_beats_chunk_route"] = bool(med < scaled)
            if rows == 2:
                from friture_amd.ringbuffer import RingBuffer
                tracker = pt.PitchTracker(RingBuffer())
                tracker._run(x1[:, :1 << 16])
                ts = []
                for _ in range(3):
                    tracker.prev_f0 = None
                    t0 = time.perf_counter()
                    tracker._run(x1)
                    ts.append(time.perf_counter() - t0)
                row["host_gate_route_ms_scaled"] = float(np.median(ts)) * S * 1e3
                row["host_gate_route_measured"] = (f"PitchTracker._run on 1 stream of [2, {T}] host samples: median of 3 "
                                                   f"{np.median(ts) * 1e3:.1f} ms (min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f}), "
                                                   f"scaled by {S} streams")
                row["batch_beats_host_gate_route"] = bool(med < float(np.median(ts)) * S)
        res["shapes"].append(row)
        del x
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
