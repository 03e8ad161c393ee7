"""Record tests/golden/scope.npz from the reference's own Scope_Widget.

Runs only where the reference checkout is (oracle.refshim): stand-ins for the Qt and UI modules the widget imports, then the
reference class is driven chunk by chunk through the reference RingBuffer on the cases of tests/scope_helpers.py (signals
regenerated from seeds there, never stored).  Recorded per refresh: whether Curve.setData ran (the trigger), the absolute index
of the trace's first sample (read from the view the widget cut out of the ring's window), the trace length, whether the window
the widget read equals the zero-padded stream, and a digest of the data each curve holds afterwards; the whole setData arrays
of a few refreshes (tests/scope_helpers.FULL_REFRESHES), among them the refresh whose data(2 w) grows the ring
and one that scrolls over what the growth left.

    python tools/make_golden_scope.py
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import scope_helpers as H  # noqa: E402
from oracle import refshim  # noqa: E402


class _Any:
    """Accepts every call and attribute (Qt widgets, layouts, signals)."""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Any()

    def __getattr__(self, name):
        return _Any()


class _QObject:
    def __init__(self, parent=None, *a, **k):
        pass


class _Curve:
    def __init__(self, *a, **k):
        self.calls = []
        self.name = None

    def setData(self, x, y):
        self.calls.append((np.array(x, copy=True), np.array(y, copy=True)))


class _ScopeData:
    def __init__(self, *a, **k):
        self.plot_items = []
        self.vertical_axis = _Any()
        self.horizontal_axis = _Any()

    def add_plot_item(self, item):
        self.plot_items.append(item)

    def remove_plot_item(self, item):
        self.plot_items.remove(item)


def install_stubs():
    refshim.install()
    qtcore = types.ModuleType("PyQt6.QtCore")
    qtcore.QObject = _QObject
    qtwidgets = types.ModuleType("PyQt6.QtWidgets")
    qtwidgets.QDialog = _Any
    qtwidgets.QFormLayout = _Any
    qtwidgets.QDoubleSpinBox = _Any
    sys.modules["PyQt6.QtCore"] = qtcore
    sys.modules["PyQt6.QtWidgets"] = qtwidgets
    sys.modules["PyQt6"].QtCore = qtcore
    sys.modules["PyQt6"].QtWidgets = qtwidgets

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    module("friture.scope_data", Scope_Data=_ScopeData)
    module("friture.curve", Curve=_Curve)
    module("friture.store", GetStore=lambda: None)


class _AudioBuffer:
    """AudioBuffer.data over the reference RingBuffer, remembering the window it handed out."""

    def __init__(self):
        from friture.ringbuffer import RingBuffer
        self.ringbuffer = RingBuffer()
        self.last = None

    def push(self, x):
        self.ringbuffer.push(x, 0.)

    def data(self, length):
        self.last = self.ringbuffer.data(length)
        return self.last


def _curve_data(curve):
    return curve.calls[-1][1] if curve.calls else np.zeros(10)


def run_case(name):
    from friture.scope import Scope_Widget
    x = H.signal(name)
    if name == "exact_level_f32":
        x = x.astype(np.float32)
    ab = _AudioBuffer()
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


def main():
    install_stubs()
    g = {}
    for name in H.CASES:
        g.update(run_case(name))
        print(f"{name}: {len(g[name + '_trig'])} refreshes, {int(g[name + '_trig'].sum())} triggered, "
              f"{int((~g[name + '_ok']).sum())} windows not the zero-padded stream")
    g["widths"] = np.array([H.width_for(t) for t in H.TIMERANGES])
    out = ROOT / "tests" / "golden" / "scope.npz"
    np.savez_compressed(out, **g)
    print(f"{out}: {out.stat().st_size} bytes, {len(g)} arrays")


if __name__ == "__main__":
    main()
