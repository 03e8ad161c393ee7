"""PCM export (pcmenc.hip, recording.encode_pcm): planar float rows to interleaved integer PCM.

Shapes: (a) 2 rows x 2^24 float32 to s16, CUDA to CUDA; (b) 8 rows x 2^22 float64 to s24 with dither, CUDA to CUDA, and the same
call without dither so that dither's cost is visible; (c) shape (a) from a CUDA tensor to host bytes (to="host"), end to end.
Each beside what a user does without the kernel, measured in the same session on the same data and checked to give the same
bits: (a) torch's (x * 32768).round().clamp(-32768, 32767).to(int16).T.contiguous(); (b) the torch byte scatter of the 24-bit
samples, without dither; (c) .cpu() of the float rows and the conversion in numpy, with the plain download of the same byte
count as the floor.  The data is noise of 0.3 full scale, so a few samples clip.  Device shapes are timed between device events
(median / min / max of --reps calls after a warm-up), (c) by the host clock around a synchronisation.  The rate of (a) and (b)
is bytes read plus bytes written as a share of the 8 TB/s HBM peak.  Prints one JSON line and writes it to --out when given."""
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
    from friture_amd.recording import encode_pcm
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_pcmenc", "reps": a.reps, "shapes": []}
    want = a.shapes.split(",")

    def noise(S, T, dtype):
        g = torch.Generator(device="cuda")
        g.manual_seed(S * 1000 + 1)
        return 0.3 * torch.randn((S, T), dtype=dtype, device="cuda", generator=g)

    def timed(fn, out):
        """encode into a buffer that exists already, as the baseline's result is written into fresh memory by torch's allocator"""
        for _ in range(3):
            fn(out)
        torch.cuda.synchronize()
        return time_call(lambda: fn(out), a.reps)

    def baseline_a(x):
        return (x * 32768).round().clamp(-32768, 32767).to(torch.int16).T.contiguous().view(torch.uint8).reshape(-1)

    def baseline_b(x):
        q = (x * 8388608).round().clamp(-8388608, 8388607).to(torch.int32).T.contiguous()               # [T, C]
        return torch.stack([q & 0xFF, (q >> 8) & 0xFF, (q >> 16) & 0xFF], dim=-1).to(torch.uint8).reshape(-1)

    Ta, Tb = (1 << 24) >> a.scale, (1 << 22) >> a.scale
    if "a" in want:
        x = noise(2, Ta, torch.float32)
        got = encode_pcm(x, "s16")
        same = bool(torch.equal(got.data, baseline_a(x)))
        out = torch.empty_like(got.data)
        t = timed(lambda o: encode_pcm(x, "s16", out=o), out)
        for _ in range(3):
            baseline_a(x)
        torch.cuda.synchronize()
        tb = time_call(lambda: baseline_a(x), a.reps)
        nbytes = 2 * Ta * (4 + 2)
        res["shapes"].append({"shape": "a", "format": "s16", "rows": 2, "frames": Ta, "input": "cuda float32", "output": "cuda uint8",
                              "algorithmic_bytes": nbytes, "clipped": got.clipped.tolist(), **stats("encode_pcm", t),
                              "GBps": nbytes / t[0] / 1e9, "hbm_share": nbytes / t[0] / HBM_PEAK, **stats("torch_baseline", tb),
                              "baseline_GBps": nbytes / tb[0] / 1e9, "same_bits_as_baseline": same, "speedup_over_baseline": tb[0] / t[0],
                              "beats_baseline_by_more_than_its_spread": bool(tb[1] > t[2])})
        del x, got, out
    if "b" in want:
        x = noise(8, Tb, torch.float64)
        got = encode_pcm(x, "s24")
        same = bool(torch.equal(got.data, baseline_b(x)))
        out = torch.empty_like(got.data)
        t_plain = timed(lambda o: encode_pcm(x, "s24", out=o), out)
        t_dither = timed(lambda o: encode_pcm(x, "s24", dither=True, seed=1, out=o), out)
        for _ in range(3):
            baseline_b(x)
        torch.cuda.synchronize()
        tb = time_call(lambda: baseline_b(x), a.reps)
        nbytes = 8 * Tb * (8 + 3)
        res["shapes"].append({"shape": "b", "format": "s24", "rows": 8, "frames": Tb, "input": "cuda float64", "output": "cuda uint8",
                              "algorithmic_bytes": nbytes, "clipped": got.clipped.tolist(), **stats("encode_pcm_dither", t_dither),
                              **stats("encode_pcm_no_dither", t_plain), "GBps_dither": nbytes / t_dither[0] / 1e9,
                              "hbm_share_dither": nbytes / t_dither[0] / HBM_PEAK, "GBps_no_dither": nbytes / t_plain[0] / 1e9,
                              "hbm_share_no_dither": nbytes / t_plain[0] / HBM_PEAK, **stats("torch_baseline_no_dither", tb),
                              "baseline_GBps": nbytes / tb[0] / 1e9, "same_bits_as_baseline_no_dither": same,
                              "speedup_over_baseline_no_dither": tb[0] / t_plain[0], "speedup_over_baseline_with_dither": tb[0] / t_dither[0],
                              "beats_baseline_by_more_than_its_spread": bool(tb[1] > t_dither[2])})
        del x, got, out
    if "c" in want:
        x = noise(2, Ta, torch.float32)

        def numpy_way():
            h = x.cpu().numpy()
            return np.ascontiguousarray(np.clip(np.rint(h.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2").T).view(np.uint8).reshape(-1)

        got = encode_pcm(x, "s16", to="host")
        same = bool(np.array_equal(got.data, numpy_way()))
        n_out = int(got.data.nbytes)
        raw = torch.empty(n_out, dtype=torch.uint8, device="cuda")
        t = host_time(lambda: encode_pcm(x, "s16", to="host"), a.reps)
        t8 = host_time(lambda: encode_pcm(x, "s16", to="host", slab_bytes=8 << 20), a.reps)
        tb = host_time(numpy_way, a.reps)
        tc = host_time(lambda: raw.cpu(), a.reps)
        res["shapes"].append({"shape": "c", "format": "s16", "rows": 2, "frames": Ta, "input": "cuda float32", "output": "host numpy uint8",
                              "encoded_bytes": n_out, **stats("end_to_end", t), "encoded_GBps": n_out / t[0] / 1e9,
                              **stats("end_to_end_8MB_slabs", t8), **stats("cpu_then_numpy", tb),
                              **stats("plain_download_of_the_encoded_bytes", tc), "download_GBps": n_out / tc[0] / 1e9,
                              "same_bits_as_baseline": same, "speedup_over_baseline": tb[0] / t[0],
                              "beats_baseline_by_more_than_its_spread": bool(tb[1] > t[2])})
    emit(res, a.out)


if __name__ == "__main__":
    main()
