"""SpectrumBatch (spectrumbatch.hip): whole recordings through the spectrum widget's chain.

Shapes: (a) 64 streams x 2^22 float32 samples at the defaults (fft_size 8192, 75 % overlap, 512-sample chunks); (b) 1 stream x
2^22; (c) 64 streams x 2^20 at fft_size 1024.  Per shape: the batch call (device events around SpectrumBatch.run on a CUDA
tensor after a warm-up, median / min / max of --reps); the per-refresh route on the same data — StftEngine(..., 64).psd once plus
one frt_spectrum_post per refresh on device buffers, what SpectrumAnalyzerStream._post_dev does — timed on ONE stream and the
first --route-refreshes refreshes with a host clock (every call ends in a synchronisation) and scaled linearly to all refreshes
and streams; the numpy oracle replay (oracle.spectrumbatch.replay) on one stream and its first --oracle-refreshes
refreshes, scaled the same way.  Bytes are what the algorithm must move: samples read, float64 PSD written and read, dB written,
as a share of the 8 TB/s HBM peak.  Prints one JSON line and writes it to --out when given.  The split between the STFT launch
and the new kernels comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool with --batch-only."""
from __future__ import annotations

import argparse
import ctypes
import sys
import time
from pathlib import Path

import numpy as np

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = [("a", 64, 1 << 22, 8192), ("b", 1, 1 << 22, 8192), ("c", 64, 1 << 20, 1024)]


def route_per_refresh(torch, _lib, sb, x1, n_refresh):
    """Seconds for the first n_refresh refreshes of one stream on the per-refresh route (x1: [T] float32 CUDA tensor)."""
    from friture_amd.stft import StftEngine
    lib = _lib.init()
    fs, _ = sb.schedule(x1.shape[0])
    n_refresh = min(n_refresh, len(fs) - 1)
    F = int(fs[n_refresh])
    N, hop, B = sb.fft_size, sb.hop, sb.n_bins
    x = torch.cat([torch.zeros(N, dtype=torch.float64, device="cuda"), x1[:F * hop].double()])[None, :(F - 1) * hop + N].contiguous()
    eng = StftEngine(N, hop, 1, 64)
    disp = [torch.zeros(B, dtype=torch.float64, device="cuda") for _ in range(2)]
    wd = torch.from_numpy(sb.w).cuda()
    db = np.empty(B)
    peak, pitch = ctypes.c_int(0), ctypes.c_int(0)
    vp = ctypes.c_void_p
    best = None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        psd = eng.psd(x)[0]
        for r in range(n_refresh):
            a, n = int(fs[r]), int(fs[r + 1] - fs[r])
            _lib.check(lib.frt_spectrum_post(vp(psd.data_ptr() + a * B * 8), 0, n, B, B, sb.kernel.ctypes.data, len(sb.kernel),
                                             float(sb.alpha), vp(disp[0].data_ptr()), vp(wd.data_ptr()), None, vp(disp[1].data_ptr()),
                                             db.ctypes.data, ctypes.byref(peak), ctypes.byref(pitch)))
            disp.reverse()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, n_refresh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--route-refreshes", type=int, default=256)
    ap.add_argument("--oracle-refreshes", type=int, default=32)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.spectrum import SpectrumBatch
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_spectrumbatch", "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, S, T, N in SHAPES:
        if label not in a.shapes.split(","):
            continue
        x = 0.25 * torch.randn((S, T), device="cuda", dtype=torch.float32, generator=g)
        sb = SpectrumBatch(N)
        r = sb.run(x)
        torch.cuda.synchronize()
        R, B = r.db.shape[1], r.db.shape[2]
        F = int(sb.schedule(T)[0][-1])
        del r
        med, tmin, tmax = time_call(lambda: sb.run(x), a.reps)
        nbytes = S * T * 4 + 2 * S * F * B * 8 + S * R * B * 8
        row = {"shape": label, "streams": S, "samples": T, "fft_size": N, "refreshes": R, "frames": F, "bins": B,
               "batch_median_ms": med * 1e3, "batch_min_ms": tmin * 1e3, "batch_max_ms": tmax * 1e3, "reps": a.reps,
               "algorithmic_bytes": nbytes, "GBps": nbytes / med / 1e9, "hbm_share": nbytes / med / HBM_PEAK}
        if not a.batch_only:
            dt, nr = route_per_refresh(torch, _lib, sb, x[0], a.route_refreshes)
            row["per_refresh_route_ms_scaled"] = dt / nr * R * S * 1e3
            row["per_refresh_route_measured"] = f"1 stream, first {nr} refreshes: {dt * 1e3:.2f} ms, scaled by {R}/{nr} x {S} streams"
            row["batch_beats_route"] = bool(med < dt / nr * R * S)
            from oracle import spectrumbatch as H
            no = min(a.oracle_refreshes, R)
            n_samp = (int(sb.schedule(T)[1][no - 1]) + 1) * 512
            xo = x[0, :n_samp].cpu().numpy().astype(np.float64)[None, None]
            t0 = time.perf_counter()
            H.replay(xo, fft_size=N)
            to = time.perf_counter() - t0
            row["numpy_oracle_ms_one_stream_scaled"] = to / no * R * 1e3
            row["numpy_oracle_measured"] = f"1 stream, first {no} refreshes: {to * 1e3:.1f} ms, scaled by {R}/{no}"
        res["shapes"].append(row)
        del x
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
