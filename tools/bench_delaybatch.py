"""DelayEstimatorBatch (delaybatch.hip): whole two-channel recordings through the delay estimator's chain.

Shapes: (a) 8 streams x 2 x 2^22 float32 samples at the default range of 1 s; (b) 64 x 2 x 2^20 at 1 s; (c) 8 x 2 x 2^22 at 0.1 s;
all at 512-sample chunks.  Per shape, in one session on the same data, medians of --reps with (max - min) / median as spread:
  run       DelayEstimatorBatch.run on a CUDA tensor (device events around the call, after a warm-up), against
            DelayEstimatorStream fed the first 256 chunks of ONE stream chunk by chunk (wall clock, the object waits for its
            windows itself) and SCALED LINEARLY to all chunks of all streams: `stream_scaled_ms` is an extrapolation, not a run;
  decimate  frt_delaybatch_decimate alone on the [2 S][T] device array, against frt_decimate_multiple on the same samples as
            float64 (it takes nothing else), one lane per channel over the whole signal.
Prints one JSON line and writes it to --out when given.  The share of each kernel comes from a separate
`rocprofv3 --kernel-trace --stats` run of this tool with --batch-only."""
from __future__ import annotations

import argparse
import ctypes
import sys
import time
from pathlib import Path

import numpy as np

from benchutil import emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = [("a", 8, 1 << 22, 1.0), ("b", 64, 1 << 20, 1.0), ("c", 8, 1 << 22, 0.1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.delay_estimator import DelayEstimatorBatch, DelayEstimatorStream
    from friture_amd.signal.decimate import _chain_handle
    torch.cuda.set_device(0)
    lib = _lib.init(0)
    vp, DP = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    res = {"tool": "bench_delaybatch", "chunk": 512, "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, S, T, delayrange in SHAPES:
        if label not in a.shapes.split(","):
            continue
        x = 0.25 * torch.randn((S, 2, T), device="cuda", dtype=torch.float32, generator=g) + 0.01
        x[:, 1] = torch.roll(x[:, 0], 124, dims=1) + 0.0025 * torch.randn((S, T), device="cuda", dtype=torch.float32, generator=g)
        batch = DelayEstimatorBatch(delayrange)
        r = batch.run(x)
        torch.cuda.synchronize()
        W = len(r.window_end)
        del r
        med, tmin, tmax = time_call(lambda: batch.run(x), a.reps)
        row = {"shape": label, "streams": S, "samples": T, "delayrange_s": delayrange, "windows": W, "slabs": batch.last_slabs,
               "reps": a.reps, "run_median_ms": med * 1e3, "run_spread": (tmax - tmin) / med}
        # the decimation alone
        n_out = ctypes.c_int64(0)
        rows = x.reshape(2 * S, T)
        out = torch.empty((2 * S, T // 4), dtype=torch.float64, device="cuda")
        zf = torch.empty((2 * S, 2, 12), dtype=torch.float64, device="cuda")
        b, ac = batch.bdec, batch.adec

        def decimate():
            _lib.check(lib.frt_delaybatch_decimate(b.ctypes.data_as(DP), ac.ctypes.data_as(DP), 13, 2, vp(rows.data_ptr()), 0, 2 * S, T, T, 0,
                                                   None, vp(out.data_ptr()), T // 4, vp(zf.data_ptr()), ctypes.byref(n_out)))
        decimate()
        torch.cuda.synchronize()
        dmed, dmin, dmax = time_call(decimate, a.reps)
        row.update({"decimate_median_ms": dmed * 1e3, "decimate_spread": (dmax - dmin) / dmed})
        if not a.batch_only:
            h = _chain_handle(b, ac, 2 * S)
            _lib.check(lib.frt_octbank_set_stream(h, None))
            wide = rows.to(torch.float64)
            got = ctypes.c_int(0)

            def sequential():
                _lib.check(lib.frt_octbank_reset(h))
                _lib.check(lib.frt_decimate_multiple(h, 2, vp(wide.data_ptr()), T, vp(out.data_ptr()), ctypes.byref(got)))
            sequential()
            torch.cuda.synchronize()
            smed, smin, smax = time_call(sequential, min(a.reps, 3))
            row.update({"sequential_decimate_median_ms": smed * 1e3, "sequential_decimate_spread": (smax - smin) / smed,
                        "sequential_decimate_reps": min(a.reps, 3), "decimate_speedup": smed / dmed})
            del wide
            one = x[0].to(torch.float64).cpu().numpy()
            chunks = 256
            ts = []
            for _ in range(a.reps):
                stream = DelayEstimatorStream(delayrange)
                stream.handle_new_data(one[:, :512])                 # the object's first push allocates
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for c in range(1, chunks + 1):
                    stream.handle_new_data(one[:, c * 512:(c + 1) * 512])
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
                del stream
            per_chunk = float(np.median(ts)) / chunks
            row.update({"stream_chunks_timed": chunks, "stream_per_chunk_us": per_chunk * 1e6, "stream_spread": (max(ts) - min(ts)) / float(np.median(ts)),
                        "stream_scaled_ms": per_chunk * (T // 512) * S * 1e3, "stream_scaled_is_extrapolated": True,
                        "run_speedup_over_scaled_stream": per_chunk * (T // 512) * S / med})
        res["shapes"].append(row)
        del x, batch, rows, out
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
