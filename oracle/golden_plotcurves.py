"""Record plotcurves.npz from the reference's own SpectrumPlotWidget and HistPlot.

Driven by oracle/make_golden.py (needs the reference checkout): the stand-ins of oracle/refshim.py plus FilledCurve,
Spectrum_Data / HistPlot_Data and format_frequency without the pitch tracker's widget stack, then the reference classes replay
the cases of oracle/plotcurves.py (inputs regenerated from seeds there, never stored).  Recorded per data event: whether setdata drew, whether the peak curve was set, the baseline, the fmax / fpitch labels
(text and screen position), and digests of every array handed to FilledCurve.setData and setBarLabels and of the peak state
afterwards; the whole arrays of a few refreshes (oracle.plotcurves.FULL_REFRESHES).
"""
from __future__ import annotations

import enum

import numpy as np

from . import plotcurves as H
from . import refshim

DIG = ["sxl", "sxr", "sy", "z", "sp", "zp", "peak", "pint", "pdecay", "barx"]


def install_stubs():
    refshim.install()
    from friture.pitch_tracker_data import format_frequency
    refshim.module("friture.pitch_tracker", format_frequency=format_frequency)
    refshim.module("friture.spectrum_data", Spectrum_Data=refshim.PlotData)
    refshim.module("friture.histplot_data", HistPlot_Data=refshim.PlotData)
    refshim.module("friture.filled_curve", CurveType=enum.Enum("CurveType", "SIGNAL PEEK"), FilledCurve=refshim.Curve)


def run_case(name):
    import friture.plotting.frequency_scales as fscales
    hist = name.startswith("hist_")
    if hist:
        from friture.histplot import HistPlot
        w = HistPlot(None)
        data = w._histplot_data
    else:
        from friture.spectrumPlotWidget import SpectrumPlotWidget
        w = SpectrumPlotWidget(None)
        data = w._spectrum_data
    sig, pk = w._curve_signal, w._curve_peak
    rec = {k: [] for k in ("drew", "peakset", "baseline", "dig", "fmax_text", "fmax_pos", "fpitch_text", "fpitch_pos")}
    full = {}
    seen = [0, 0]
    for k in H.replay(name, w, fscales):
        drew, peakset = len(sig.calls) > seen[0], len(pk.calls) > seen[1]
        seen = [len(sig.calls), len(pk.calls)]
        s = sig.calls[-1] if sig.calls else (None,) * 5
        p = pk.calls[-1] if pk.calls else (None,) * 5
        rec["drew"].append(drew)
        rec["peakset"].append(peakset)
        rec["baseline"].append(np.nan if s[4] is None else float(s[4]))
        barx = data.bars[0] if hist and data.bars else None
        rec["dig"].append([H.digest(s[0]), H.digest(s[1]), H.digest(s[2]), H.digest(s[3]), H.digest(p[2]), H.digest(p[3]),
                           H.digest(w.peak), H.digest(w.peak_int), H.digest(w.peak_decay), H.digest(barx)])
        if not hist:
            rec["fmax_text"].append(data.fmax[0] if data.fmax else "")
            rec["fmax_pos"].append(float(data.fmax[1]) if data.fmax else np.nan)
            rec["fpitch_text"].append(data.fpitch[0] if data.fpitch else "")
            rec["fpitch_pos"].append(float(data.fpitch[1]) if data.fpitch else np.nan)
        if k in H.FULL_REFRESHES.get(name, ()):
            for key, v in zip(("sxl", "sxr", "sy", "z"), s[:4]):
                full[f"full{k}_{key}"] = v
            if p[2] is not None:
                full[f"full{k}_sp"], full[f"full{k}_zp"] = p[2], p[3]
            full[f"full{k}_state"] = np.array([w.peak, w.peak_int, w.peak_decay])
    out = {f"{name}_{k}": np.array(v) for k, v in rec.items() if len(v)}
    out[f"{name}_dig"] = out[f"{name}_dig"].astype(np.uint64)
    out.update({f"{name}_{k}": v for k, v in full.items()})
    return out


def plotcurves(out_dir):
    install_stubs()
    g = {"dig_fields": np.array(DIG)}
    for name in H.SPECTRUM_CASES + H.HIST_CASES:
        g.update(run_case(name))
        print(f"{name}: {len(g[name + '_drew'])} refreshes, {int(g[name + '_drew'].sum())} drawn, "
              f"{int(g[name + '_peakset'].sum())} with peaks")
    np.savez_compressed(out_dir / "plotcurves.npz", **g)
