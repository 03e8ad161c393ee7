"""SpectrogramBatch (specgrambatch.hip): whole recordings through the spectrogram widget's chain.

Shapes: (a) 64 streams x 2^22 float32 samples at the defaults (fft_size 4096, 75 % overlap, 400 rows, 800 columns per 10 s,
512-sample chunks); (b) 1 stream x 2^22; (c) 64 streams x 2^20 at fft_size 1024.  Per shape: the batch call (device events around
SpectrogramBatch.run on a CUDA tensor after a warm-up, median / min / max of --reps); the per-stream route the library offered
before on the same data — StftEngine(..., 64).norm once, then one frt_screen_columns per stream with the same column table, device
buffers in and out — timed the same way on --route-streams streams and scaled linearly to all streams; the frt_specgram_batch ENTRY alone on the first time
slab of the batch call (its frames already in device memory; the time includes the entry's host work — interval search, tile
table, staging of the column table — and its synchronisation, so it bounds the kernel from above), scaled by frames to the
recording, as a share of the batch call and as a rate on its algorithmic bytes (frames read once, pixels written) against the
8 TB/s HBM peak.  The kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run with --batch-only.  Prints one
JSON line and writes it to --out when given."""
from __future__ import annotations

import argparse
import ctypes
import sys
from pathlib import Path

import numpy as np

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = [("a", 64, 1 << 22, 4096), ("b", 1, 1 << 22, 4096), ("c", 64, 1 << 20, 1024)]


def frames_of(torch, sb, x, F):
    """The float64 window of the first F frames of x [S, T] as a fresh widget sees them (frame 0 ends at sample 0)."""
    N, hop = sb.fft_size, sb.hop
    S = x.shape[0]
    return torch.cat([torch.zeros((S, N), dtype=torch.float64, device="cuda"), x[:, :F * hop].double()], dim=1)[:, :(F - 1) * hop + N].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--route-streams", type=int, default=4)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.spectrogram import SpectrogramBatch
    from friture_amd.stft import StftEngine
    torch.cuda.set_device(0)
    lib = _lib.init(0)
    vp = ctypes.c_void_p
    res = {"tool": "bench_spectrogrambatch", "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, S, T, N in SHAPES:
        if label not in a.shapes.split(","):
            continue
        x = 0.25 * torch.randn((S, T), device="cuda", dtype=torch.float32, generator=g)
        sb = SpectrogramBatch(N)
        r = sb.run(x)
        torch.cuda.synchronize()
        H, P, B = r.pixels.shape[1], r.pixels.shape[2], sb.n_bins
        F = int(sb.schedule(T)[0][-1])
        del r
        med, tmin, tmax = time_call(lambda: sb.run(x), a.reps)
        row = {"shape": label, "streams": S, "samples": T, "fft_size": N, "frames": F, "bins": B, "height": H, "columns": P,
               "batch_median_ms": med * 1e3, "batch_min_ms": tmin * 1e3, "batch_max_ms": tmax * 1e3, "reps": a.reps}
        if not a.batch_only:
            table = sb.columns(T)
            src, wts = np.ascontiguousarray(np.where(table.filler, -1, table.src), np.int32), np.ascontiguousarray(table.a)
            # ---- the frt_specgram_batch entry alone, on the first slab of the batch call ------------------------------------------------
            nf = min(F, max(1, (1 << 30) // (S * B * 8)))
            nc = int(np.searchsorted(table.src, nf))
            eng = sb._engine(S)
            norm = torch.empty((S, nf, B), dtype=torch.float64, device="cuda")
            eng.norm(frames_of(torch, sb, x, nf), out=norm)
            old = torch.zeros((2, S, H), dtype=torch.float64, device="cuda")
            pix = torch.empty((S, H, nc), dtype=torch.int32, device="cuda")
            call = lambda: _lib.check(lib.frt_specgram_batch(
                vp(norm.data_ptr()), S, nf, B, B, nf * B, sb.freq.ctypes.data, sb.targets.ctypes.data, H, src.ctypes.data, wts.ctypes.data, nc,
                vp(old[0].data_ptr()), vp(old[1].data_ptr()), sb.lut.ctypes.data, vp(pix.data_ptr()), 0, nc))
            call()
            kmed, kmin, kmax = time_call(call, a.reps)
            kbytes = S * nf * B * 8 + S * H * nc * 4
            row.update({"entry_slab_frames": nf, "entry_slab_columns": nc, "entry_slab_median_ms": kmed * 1e3, "entry_slab_min_ms": kmin * 1e3,
                        "entry_slab_max_ms": kmax * 1e3, "entry_algorithmic_bytes": kbytes, "entry_GBps": kbytes / kmed / 1e9,
                        "entry_hbm_share": kbytes / kmed / HBM_PEAK, "entry_ms_scaled_to_recording": kmed * F / nf * 1e3,
                        "entry_share_of_batch_call": kmed * F / nf / med})
            del norm, pix
            # ---- the per-stream route: one transform, then one frt_screen_columns per stream -----------------------------------
            ns = min(S, a.route_streams)
            eng1 = StftEngine(N, sb.hop, ns, 64)
            eng1.set_epilogue(sb.w, sb.spec_min, sb.spec_max, None)
            norm = torch.empty((ns, F, B), dtype=torch.float64, device="cuda")
            pix = torch.empty((H, P), dtype=torch.int32, device="cuda")
            route_src = np.ascontiguousarray(table.src, np.int32)
            old_in, old_out = torch.zeros(H, dtype=torch.float64, device="cuda"), torch.zeros(H, dtype=torch.float64, device="cuda")

            def route():
                eng1.norm(frames_of(torch, sb, x[:ns], F), out=norm)
                for s in range(ns):
                    _lib.check(lib.frt_screen_columns(vp(norm[s].data_ptr()), B, F, sb.freq.ctypes.data, sb.targets.ctypes.data, H,
                                                      vp(old_in.data_ptr()), route_src.ctypes.data, wts.ctypes.data, P, sb.lut.ctypes.data,
                                                      vp(pix.data_ptr()), vp(old_out.data_ptr())))
            route()
            rmed, rmin, rmax = time_call(route, a.reps)
            k = S / ns
            row.update({"route_streams_measured": ns, "route_median_ms": rmed * 1e3, "route_min_ms": rmin * 1e3, "route_max_ms": rmax * 1e3,
                        "route_ms_scaled": rmed * k * 1e3, "route_note": f"{ns} of {S} streams measured, scaled by {k:g}",
                        "route_over_batch": rmed * k / med,
                        "batch_not_slower_beyond_spread": bool(rmed * k - med > -max(tmax - tmin, (rmax - rmin) * k))})
            del norm, pix
        res["shapes"].append(row)
        del x
        torch.cuda.empty_cache()
    emit(res, a.out)


if __name__ == "__main__":
    main()
