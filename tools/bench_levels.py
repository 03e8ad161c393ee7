"""Level meters + long-time levels (levels.hip): batch throughput and interactive latency.

Batch: 64 ch x 2^22 float32 and 8 ch x 2^22 float64, chunk 512, rt = 20, timed with device events after a warm-up, repeated;
algorithmic bytes = input + outputs, as a share of the 8 TB/s HBM peak.  Interactive: p50 per 512-sample chunk of the
2-channel Levels and the LongLevels objects, against the reference-shaped numpy chain restated here.  Prints one JSON line
and writes it to --out when given.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def numpy_chain(kernel, alpha, alpha2):
    """The reference's per-chunk host work (levels.py:92-110 for 2 channels, longlevels.py:148-171 fed by 512 samples)."""
    from friture_amd.iec import dB_to_IEC
    state = {"max": [1e-30, 1e-30], "rms": [1e-30, 1e-30]}

    def step(y):
        for c in range(2):
            v = np.abs(y[c]).max()
            state["max"][c] = v if v > state["max"][c] * (1. - alpha2) else state["max"][c] * (1. - alpha2)
            N = y.shape[1]
            state["rms"][c] = float(alpha * np.dot(kernel[kernel.shape[0] - N:], y[c] ** 2) + state["rms"][c] * (1. - alpha) ** N)
            dB_to_IEC(max(20. * np.log10(state["max"][c]), 10. * np.log10(state["rms"][c])))
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", action="store_true")
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.levels import Levels, LevelsBatch
    from friture_amd.longlevels import LongLevels
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_levels", "batch": []}
    for C, dt in [(64, torch.float32), (8, torch.float64)]:
        T = 1 << 22
        x = (0.1 * torch.randn(C, T, device="cuda", dtype=torch.float64)).to(dt)
        lb = LevelsBatch(C, 20, 512)
        m, lo = lb.run(x)
        torch.cuda.synchronize()
        med, tmin, tmax = time_call(lambda: lb.run(x), a.reps, before_each=lb.reset)
        nbytes = x.numel() * x.element_size() + m.numel() * 8 + lo.numel() * 8
        res["batch"].append({"channels": C, "samples": T, "dtype": str(dt).split(".")[-1], "chunk": 512, "rt": 20,
                             "median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3, "bytes": nbytes,
                             "GBps": nbytes / med / 1e9, "hbm_share": nbytes / med / HBM_PEAK})
    if not a.batch_only:
        rng = np.random.default_rng(0)
        chunks = [0.1 * rng.standard_normal((2, 512)) for _ in range(400)]
        lv, ll = Levels(), LongLevels()

        def p50(f):
            for c in chunks[:20]:
                f(c)
            ts = []
            for c in chunks:
                t0 = time.perf_counter()
                f(c)
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts)) * 1e6
        res["interactive_us_p50"] = {"Levels_2ch": p50(lv.handle_new_data), "LongLevels": p50(ll.handle_new_data),
                                     "numpy_meter_chain_2ch": p50(numpy_chain(lv.kernel, lv.alpha, lv.alpha2))}
    emit(res, a.out)


if __name__ == "__main__":
    main()
