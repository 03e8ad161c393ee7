"""Record scope.npz from the reference's own Scope_Widget.

Driven by oracle/make_golden.py (needs the reference checkout): on the stand-ins of oracle/refshim.py, the reference class is
driven chunk by chunk through the reference RingBuffer on the cases of oracle/scope.py (signals regenerated from seeds
there, never stored).  Recorded per refresh: whether Curve.setData ran (the trigger), the absolute index
of the trace's first sample (read from the view the widget cut out of the ring's window), the trace length, whether the window
the widget read equals the zero-padded stream, and a digest of the data each curve holds afterwards; the whole setData arrays
of a few refreshes (oracle.scope.FULL_REFRESHES), among them the refresh whose data(2 w) grows the ring
and one that scrolls over what the growth left.
"""
from __future__ import annotations

import numpy as np

from . import refshim
from . import scope as H


def _curve_data(curve):
    return curve.calls[-1][1] if curve.calls else np.zeros(10)


def run_case(name):
    from friture.scope import Scope_Widget
    x = H.signal(name)
    if name == "exact_level_f32":
        x = x.astype(np.float32)
    ab = refshim.AudioBuffer()
    w = Scope_Widget(None)
    w.set_buffer(ab)
    rec = {k: [] for k in ("trig", "start", "len", "ok", "dig")}
    full = {}
    for k, (s, n, rows, tr) in enumerate(H.schedule(name)):
        chunk = x[:rows, s:s + n]
        ab.push(chunk)
        w.set_timerange(tr)
        before = len(w._curve.calls)
        w.handle_new_data(chunk)
        trig = len(w._curve.calls) > before
        win = ab.last
        if trig:
            rel = (w.y.__array_interface__["data"][0] - win.__array_interface__["data"][0]) // win.strides[1]
            assert np.array_equal(w.y, win[0, rel:rel + w.y.shape[0]], equal_nan=True)
            start = ab.ringbuffer.offset - win.shape[1] + int(rel)
        else:
            start = H.NO_TRIGGER
        ok = np.array_equal(win[:rows], H.expected_window(name, k, win.shape[1]), equal_nan=True)
        rec["trig"].append(trig)
        rec["start"].append(start)
        rec["len"].append(w.y.shape[0])
        rec["ok"].append(ok)
        rec["dig"].append([H.digest(_curve_data(w._curve)), H.digest(_curve_data(w._curve_2))])
        if k in H.FULL_REFRESHES.get(name, ()):
            full[f"full{k}_trig"] = np.array(trig)
            if trig:
                full[f"full{k}_t"], full[f"full{k}_y"] = w._curve.calls[-1]
                if name == "change":
                    del full[f"full{k}_t"]                       # scaled_t depends on the width only
                full[f"full{k}_raw"] = np.array(w.y, copy=True)
                if w.y2 is not None:
                    full[f"full{k}_y2"] = w._curve_2.calls[-1][1]
    out = {f"{name}_{k}": np.array(v) for k, v in rec.items()}
    out[f"{name}_dig"] = out[f"{name}_dig"].astype(np.uint64)
    out[f"{name}_start"] = out[f"{name}_start"].astype(np.int64)
    out.update({f"{name}_{k}": v for k, v in full.items()})
    return out


def scope(out_dir):
    refshim.install()
    g = {}
    for name in H.CASES:
        g.update(run_case(name))
        print(f"{name}: {len(g[name + '_trig'])} refreshes, {int(g[name + '_trig'].sum())} triggered, "
              f"{int((~g[name + '_ok']).sum())} windows not the zero-padded stream")
    g["widths"] = np.array([H.width_for(t) for t in H.TIMERANGES])
    np.savez_compressed(out_dir / "scope.npz", **g)
