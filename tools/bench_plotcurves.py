"""Plot curves (curves.hip): batch throughput and interactive latency.

Batch: (a) 64 streams x 64 refreshes x 8193 bins float64, every output; (b) the same with keep="last"; (c) 64 channels x 8192
refreshes x 27 bands float32, the layout of FirBank.energies(..., as_db=True), every output.  Device events around the call after a
warm-up, repeated.  Bytes are what the algorithm must move: the input once, the state in and out, the outputs, as a share of the
8 TB/s HBM peak.  Interactive: p50 of one SpectrumPlot.setdata at 8193 bins and one HistPlot.setdata at 27 bands, against the
numpy body of oracle.plotcurves.NumpyCurves plus the edges the widgets recompute every refresh.  Prints one JSON line and
writes it to --out when given.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

from benchutil import HBM_PEAK, emit, time_call

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", action="store_true")
    a = ap.parse_args()
    import torch
    from friture_amd import _lib
    from friture_amd.plotcurves import CurveBatch, HistPlot, SpectrumPlot, bin_edges
    torch.cuda.set_device(0)
    _lib.init(0)
    res = {"tool": "bench_plotcurves", "batch": []}
    g = torch.Generator(device="cuda").manual_seed(0)
    for label, S, R, B, dt, keep in [("a", 64, 64, 8193, torch.float64, "all"), ("b", 64, 64, 8193, torch.float64, "last"),
                                     ("c", 64, 8192, 27, torch.float32, "all")]:
        y = (-60. + 15. * torch.randn((S, R, B), device="cuda", dtype=torch.float64, generator=g)).to(dt)
        cb = CurveBatch(-100., 0.)
        r = cb.run(y, keep=keep)
        torch.cuda.synchronize()
        med, tmin, tmax = time_call(lambda: cb.run(y, keep=keep), a.reps)
        nbytes = y.numel() * y.element_size() + 2 * r.state.numel() * 8 + sum(o.numel() * 8 for o in r[:4])
        res["batch"].append({"workload": label, "streams": S, "refreshes": R, "bins": B, "dtype": str(dt).split(".")[-1],
                             "keep": keep, "median_ms": med * 1e3, "min_ms": tmin * 1e3, "max_ms": tmax * 1e3,
                             "bytes": nbytes, "GBps": nbytes / med / 1e9, "hbm_share": nbytes / med / HBM_PEAK,
                             "ns_per_refresh_per_lane_walk": med / R * 1e9})
        del y, r
        torch.cuda.empty_cache()
    if not a.batch_only:
        from oracle import plotcurves as H
        from friture_amd.plotting import frequency_scales as fs
        rng = np.random.default_rng(0)

        def p50(f, rows):
            ts = []
            for y in rows:
                t0 = time.perf_counter()
                f(y)
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts[20:])) * 1e6

        x = H.freqs(8193)
        spec_rows = [-60. + 15. * rng.standard_normal(8193) for _ in range(300)]
        sp = SpectrumPlot()
        sp.setspecrange(-100., 0.)
        sp.setfreqscale(fs.Logarithmic)
        sp.setfreqrange(20., 22000.)
        npc = H.NumpyCurves(-100., 0.)

        def numpy_spectrum(y):                     # the widget body: edges and screen x every refresh, curves, peaks
            xl, xr = bin_edges(x)
            sp.horizontal.toScreen(xl)
            sp.horizontal.toScreen(xr)
            npc.setdata(y)

        fl, fh, fc = H.bands(3)
        hist_rows = [-60. + 15. * rng.standard_normal(27) for _ in range(300)]
        hp = HistPlot()
        hp.setspecrange(-100., 0.)
        nph = H.NumpyCurves(-100., 0.)

        def numpy_hist(y):
            sxl, sxr = hp.horizontal.toScreen(fl), hp.horizontal.toScreen(fh)
            (sxl + sxr) / 2
            nph.setdata(y)

        res["interactive_us_p50"] = {
            "SpectrumPlot_8193": p50(lambda y: sp.setdata(x, y, 1234.5, 440.), spec_rows),
            "numpy_spectrum_body_8193": p50(numpy_spectrum, spec_rows),
            "HistPlot_27": p50(lambda y: hp.setdata(fl, fh, fc, y), hist_rows),
            "numpy_hist_body_27": p50(numpy_hist, hist_rows)}
    emit(res, a.out)


if __name__ == "__main__":
    main()
