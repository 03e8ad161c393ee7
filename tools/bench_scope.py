"""Oscilloscope (scope.hip): batch throughput and interactive latency.

Batch: 64 streams x 2 rows x 2^22 float32 samples refreshed every 512 samples at width 2400 (50 ms) and 24000 (500 ms), starts
only, and 8 streams x 2 rows at width 2400 with raw traces; device events around the call after a warm-up, repeated.  Bytes are
what the algorithm must move: row 0 once (starts only: the other rows are not read) or every row once (traces), plus the
outputs, as a share of the 8 TB/s HBM peak.  Interactive: p50 per 512-sample stereo chunk of Scope on a host RingBuffer and on a
DeviceRingBuffer, against the reference's numpy body restated here (ring window, trigger search, slices, scaled arrays).  Prints
one JSON line and writes it to --out when given.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def numpy_body(ring, timerange=50):
    """Scope_Widget.handle_new_data (friture/scope.py:78-135) for two channels, numpy on the host ring."""
    from numpy import arange, where
    width = int(timerange * 1e-3 * 48000)

    def step(floatdata):
        window = ring.data(2 * width)
        triggerdata = window[0, width // 2:-width // 2]
        level = triggerdata.max() * 2. / 3.
        pos = where((triggerdata[:-1] < level) * (triggerdata[1:] >= level))[0]
        if len(pos) == 0:
            return
        shift = pos[0] + width // 2
        window = window[:, shift - width // 2:shift + width // 2]
        y, y2 = window[0, :], window[1, :]
        t = (arange(len(y)) - width // 2) / 48000.
        (t * 1e3 + timerange / 2.) / timerange
        1. - (y + 1) / 2.
        1. - (y2 + 1) / 2.
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", action="store_true")
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.ringbuffer import DeviceRingBuffer, RingBuffer
    from friture_amd.scope import Scope, ScopeBatch
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_scope", "batch": []}
    T, chunk = 1 << 22, 512
    g = torch.Generator(device="cuda").manual_seed(0)
    for S, tr, traces in [(64, 50, None), (64, 500, None), (8, 50, "raw")]:
        t = torch.arange(T, device="cuda", dtype=torch.float64) / 48000.
        x = torch.empty((S, 2, T), device="cuda", dtype=torch.float32)
        for s in range(S):                                 # a tone per stream plus noise: triggers within its first period
            f = 200. + 37. * s
            x[s, 0] = (0.5 * torch.sin(2 * np.pi * f * t) + 0.05 * torch.randn(T, device="cuda", dtype=torch.float64,
                                                                               generator=g)).float()
            x[s, 1] = (0.3 * torch.cos(2 * np.pi * f * t)).float()
        del t
        sb = ScopeBatch(tr)
        r = sb.run(x, chunk=chunk, traces=traces)
        torch.cuda.synchronize()
        med, tmin, tmax = time_call(lambda: sb.run(x, chunk=chunk, traces=traces), a.reps)
        K = r.starts.shape[1]
        rows_read = 2 if traces else 1
        nbytes = S * rows_read * T * x.element_size() + r.starts.numel() * 8 + (r.traces.numel() * 8 if traces else 0)
        res["batch"].append({"streams": S, "rows": 2, "samples": T, "dtype": "float32", "chunk": chunk, "timerange_ms": tr,
                             "width": sb.width, "refreshes": K, "traces": traces or "none",
                             "triggered_share": float(r.triggered.float().mean().item()),
                             "median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "bytes": nbytes,
                             "GBps": nbytes / med / 1e9, "hbm_share": nbytes / med / HBM_PEAK,
                             "ns_per_refresh": med / (S * K) * 1e9})
        del x, r
        torch.cuda.empty_cache()
    if not a.batch_only:
        rng = np.random.default_rng(0)
        tt = np.arange(400 * 512) / 48000.
        sig = np.stack([0.5 * np.sin(2 * np.pi * 441. * tt) + 0.05 * rng.standard_normal(tt.shape[0]),
                        0.3 * np.sin(2 * np.pi * 660. * tt)])
        chunks = [np.ascontiguousarray(sig[:, i * 512:(i + 1) * 512]) for i in range(400)]

        def p50(ring, f, device=False):
            cs = [torch.from_numpy(c).cuda() for c in chunks] if device else chunks
            ts = []
            for i, c in enumerate(cs):
                ring.push(c)
                if device:
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                f(c)
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts[20:])) * 1e6

        def scope_on(ring):
            sc = Scope()
            sc.set_buffer(ring)
            return sc.handle_new_data
        host, dev, ref = RingBuffer(), DeviceRingBuffer(), RingBuffer()
        res["interactive_us_p50"] = {"Scope_host_ring_2ch": p50(host, scope_on(host)),
                                     "Scope_device_ring_2ch": p50(dev, scope_on(dev), device=True),
                                     "numpy_widget_body_2ch": p50(ref, numpy_body(ref))}
        # the numpy body per refresh, times the refreshes of the 64-stream batch: what the restatement would take
        res["numpy_batch_estimate_ms_64x2^22_w2400"] = res["interactive_us_p50"]["numpy_widget_body_2ch"] * 64 * (T // chunk) * 1e-3
    emit(res, a.out)


if __name__ == "__main__":
    main()
