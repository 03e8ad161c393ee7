"""Per-push latency of the pitch tracker's live chain: PitchTrackerStream (pitchstream.hip) against PitchTracker.

    python tools/bench_pitchstream.py --out profiles/pitchstream_latency.json

Shapes: the defaults (fft_size 4096, 75 % overlap, 10 s curve: one frame every second chunk) with one row and with two rows in
the ring.  Per shape and repeat: --pushes (1000) pushes of 512 samples after --warmup (50), host clock around RingBuffer.push +
update() — a host ring in, the estimates (and for the stream the latest estimate and the curve) on the host: every refreshing
update ends in a synchronisation.  Routes, all in this session on the same chunks: PitchTrackerStream; PitchTracker, the
baseline (one row: the throughput kernels once per update; two rows: raw estimates back, the gate as a host loop); the numpy
WidgetReplay of oracle/pitchbatch.py, --replay-pushes (200).  Figures: p50 / p99 / mean over all pushes and over the pushes
that complete a frame; and a sweep of one push of 1 .. 64 frames with the product by either kernel (the crossover).
--repeats (3) tells the baseline's own spread: the bar is that the stream's p50 over refreshing pushes lies below the
baseline's by more than the baseline's repeat-to-repeat spread (max - min of its p50).

--trace: for a separate `rocprofv3 --kernel-trace --stats` run — one row, 20 warm-up and 200 timed pushes (100 refreshes of one
frame) through the stream, then the same through PitchTracker: launches per refreshing push = launches / 110 per route, and
live_strength_kernel stands beside pitch_strength_kernel on one frame.
Prints one JSON line and writes it to --out when given."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

from benchutil import emit

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CHUNK = 512


def signal(rows, n, seed):
    """Harmonic tones whose pitch wanders, one per row, with a little noise: frames that pass the gate and frames that do not."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 48000.0
    out = []
    for _ in range(rows):
        f0 = 110.0 * 2 ** (3 * rng.random())
        phase = 2 * np.pi * f0 * t * (1 + 0.02 * np.sin(2 * np.pi * 0.3 * t))
        x = 0.2 * (np.sin(phase) + 0.5 * np.sin(2 * phase)) * (np.sin(2 * np.pi * 0.11 * t) > -0.5)
        out.append(x + 1e-3 * rng.standard_normal(n))
    return np.stack(out)


def figures(ts):
    ts = np.sort(np.asarray(ts)) * 1e6
    return {"p50_us": float(ts[len(ts) // 2]), "p99_us": float(ts[int(len(ts) * 0.99)]), "mean_us": float(ts.mean()), "pushes": len(ts)}


def time_route(push, chunks, warmup):
    """push(chunk) -> refreshed; per-push wall times of the chunks after the warm-up, all and refreshing ones."""
    for c in chunks[:warmup]:
        push(c)
    every, fresh = [], []
    for c in chunks[warmup:]:
        t0 = time.perf_counter()
        refreshed = push(c)
        dt = time.perf_counter() - t0
        every.append(dt)
        if refreshed:
            fresh.append(dt)
    return {"all": figures(every), "refreshing": figures(fresh)}


def tracker_route(cls, rows):
    from friture_amd.ringbuffer import RingBuffer
    ring = RingBuffer()
    ring.push(np.zeros((rows, 0)))
    trk = cls(ring)

    def push(c):
        ring.push(c)
        return trk.update()
    return push, trk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--replay-pushes", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd import pitch_tracker as pt
    from friture_amd.ringbuffer import RingBuffer
    from oracle import pitchbatch as H
    torch.cuda.set_device(0)
    _lib.init(0)
    if a.trace:
        x = signal(1, 220 * CHUNK, 7)
        chunks = [x[:, i * CHUNK:(i + 1) * CHUNK] for i in range(220)]
        for cls in (pt.PitchTrackerStream, pt.PitchTracker):
            push, _ = tracker_route(cls, 1)
            time_route(push, chunks, 20)
        return
    res = {"tool": "bench_pitchstream", "fft_size": pt.DEFAULT_FFT_SIZE, "overlap": 0.75, "chunk": CHUNK, "warmup": a.warmup,
           "clock": "host, around RingBuffer.push + update()", "shapes": []}
    for rows in (1, 2):
        n = a.warmup + a.pushes
        x = signal(rows, n * CHUNK, 7 + rows)
        chunks = [x[:, i * CHUNK:(i + 1) * CHUNK] for i in range(n)]
        row = {"rows": rows, "repeats": []}
        for _ in range(a.repeats):
            rep = {}
            for name, cls in (("stream", pt.PitchTrackerStream), ("tracker", pt.PitchTracker)):
                push, trk = tracker_route(cls, rows)
                rep[name] = time_route(push, chunks, a.warmup)
                rep[name]["voiced_share"] = float(np.mean(~np.isnan(trk.get_estimates(5.0))))
            replay = H.WidgetReplay()
            rep["numpy_replay"] = time_route(replay.push, chunks[:a.warmup + a.replay_pushes], a.warmup)
            row["repeats"].append(rep)
        p50 = {name: [rep[name]["refreshing"]["p50_us"] for rep in row["repeats"]] for name in ("stream", "tracker", "numpy_replay")}
        spread = max(p50["tracker"]) - min(p50["tracker"])
        row["refreshing_p50_us"] = {name: float(np.median(v)) for name, v in p50.items()}
        row["tracker_p50_spread_us"] = spread
        row["stream_below_tracker_by_us"] = float(np.median(p50["tracker"]) - np.median(p50["stream"]))
        row["bar_met"] = bool(max(p50["stream"]) < min(p50["tracker"]) and row["stream_below_tracker_by_us"] > spread)
        res["shapes"].append(row)
    # where the few-frames product kernel hands over to the tiled one: a push of F frames with the threshold above and below F
    x = signal(1, 4096 + 63 * 1024, 5)
    sweep = []
    for frames in (1, 2, 4, 8, 12, 16, 24, 32, 64):
        span, entry = x[:, :4096 + (frames - 1) * 1024], {"frames": frames}
        for name, crossover in (("few_frames_kernel_us", 1024), ("tiled_kernel_us", 0)):
            trk = pt.PitchTrackerStream(RingBuffer())
            trk.crossover = crossover
            ts = []
            for i in range(40):
                t0 = time.perf_counter()
                trk._push(span)
                ts.append(time.perf_counter() - t0)
            entry[name] = float(np.median(ts[10:])) * 1e6
        sweep.append(entry)
    res["crossover_sweep"] = {"what": "median host time of one push of `frames` frames (30 of 40 pushes), product by either kernel",
                              "default_crossover": pt.PitchTrackerStream(RingBuffer()).crossover, "points": sweep}
    emit(res, a.out)


if __name__ == "__main__":
    main()
