"""PCM ingest (pcm.hip, recording.decode_pcm): interleaved integer recordings to planar float rows.

Shapes: (a) s16 x 2 channels x 2^24 frames, a CUDA uint8 tensor to float32; (b) s24 x 8 channels x 2^22 frames, a CUDA tensor to
float64; (c) shape (a) from a host numpy buffer with to="cuda", end to end.  Each beside what a user does without the kernel,
measured in the same session on the same data and checked to give the same bits: (a) the int16 view transposed, converted and
scaled in torch; (b) the byte gather of the 24-bit samples in torch; (c) the numpy conversion on the host and the upload of the
float result.  Device shapes are timed between device events (median / min / max of --reps calls after a warm-up), (c) by the
host clock around a synchronisation.  The rate of (a) and (b) is bytes read plus bytes written as a share of the 8 TB/s HBM
peak; for (c) the yardstick is the plain upload of the raw bytes (half the float bytes), measured alongside, and the same call with
slab_bytes = 8 MB shows what the overlap of the host copy with the upload is worth.  Prints one JSON
line and writes it to --out when given."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def host_time(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), min(ts), max(ts)


def stats(prefix, t):
    return {f"{prefix}_median_ms": t[0] * 1e3, f"{prefix}_min_ms": t[1] * 1e3, f"{prefix}_max_ms": t[2] * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--scale", type=int, default=0, help="halve the frame counts this many times (a quick look)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.recording import decode_pcm
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_pcm", "reps": a.reps, "shapes": []}
    rng = np.random.default_rng(0)
    want = a.shapes.split(",")

    def device_row(label, fmt, width, C, T, dtype, baseline):
        raw = torch.from_numpy(rng.integers(0, 256, T * C * width, dtype=np.uint8)).cuda()
        y = decode_pcm(raw, fmt, C, dtype=dtype)
        same = bool(torch.equal(y, baseline(raw, T, C)))
        del y
        for fn in (lambda: decode_pcm(raw, fmt, C, dtype=dtype), lambda: baseline(raw, T, C)):        # warm: allocator blocks, clocks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = time_call(lambda: decode_pcm(raw, fmt, C, dtype=dtype), a.reps)
        tb = time_call(lambda: baseline(raw, T, C), a.reps)
        nbytes = T * C * (width + np.dtype(dtype).itemsize)
        row = {"shape": label, "format": fmt, "channels": C, "frames": T, "input": "cuda uint8", "output": np.dtype(dtype).name,
               "algorithmic_bytes": nbytes, **stats("decode_pcm", t), "GBps": nbytes / t[0] / 1e9, "hbm_share": nbytes / t[0] / HBM_PEAK,
               **stats("torch_baseline", tb), "baseline_GBps": nbytes / tb[0] / 1e9, "same_bits_as_baseline": same,
               "speedup_over_baseline": tb[0] / t[0], "beats_baseline_by_more_than_its_spread": bool(tb[1] > t[2])}
        res["shapes"].append(row)

    def baseline_a(raw, T, C):
        return raw.view(torch.int16).view(T, C).t().to(torch.float32).mul_(2.0 ** -15).contiguous()

    def baseline_b(raw, T, C):
        b = raw.view(T, C, 3)
        v = b[..., 0].to(torch.int32) | (b[..., 1].to(torch.int32) << 8) | (b[..., 2].to(torch.int32) << 16)
        return ((v ^ 0x800000) - 0x800000).t().to(torch.float64).mul_(2.0 ** -23).contiguous()

    Ta, Tb = (1 << 24) >> a.scale, (1 << 22) >> a.scale
    if "a" in want:
        device_row("a", "s16", 2, 2, Ta, np.float32, baseline_a)
    if "b" in want:
        device_row("b", "s24", 3, 8, Tb, np.float64, baseline_b)
    if "c" in want:
        C, T = 2, Ta
        raw = rng.integers(0, 256, T * C * 2, dtype=np.uint8)

        def numpy_way():
            x = np.ascontiguousarray(raw.view("<i2").reshape(T, C).T.astype(np.float32) * np.float32(2.0 ** -15))
            return torch.from_numpy(x).cuda()

        y = decode_pcm(raw, "s16", C, to="cuda")
        same = bool(torch.equal(y, numpy_way()))
        del y
        t = host_time(lambda: decode_pcm(raw, "s16", C, to="cuda"), a.reps)
        tb = host_time(numpy_way, a.reps)
        t8 = host_time(lambda: decode_pcm(raw, "s16", C, to="cuda", slab_bytes=8 << 20), a.reps)
        tc = host_time(lambda: torch.from_numpy(raw).cuda(), a.reps)
        res["shapes"].append({"shape": "c", "format": "s16", "channels": C, "frames": T, "input": "host numpy uint8", "output": "float32, cuda",
                              "raw_bytes": int(raw.nbytes), **stats("end_to_end", t), "raw_GBps": raw.nbytes / t[0] / 1e9,
                              **stats("end_to_end_8MB_slabs", t8),
                              **stats("numpy_then_upload", tb), **stats("plain_upload_of_the_raw_bytes", tc),
                              "upload_GBps": raw.nbytes / tc[0] / 1e9, "same_bits_as_baseline": same, "speedup_over_baseline": tb[0] / t[0],
                              "beats_baseline_by_more_than_its_spread": bool(tb[1] > t[2])})
    emit(res, a.out)


if __name__ == "__main__":
    main()
