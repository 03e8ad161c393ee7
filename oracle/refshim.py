"""oracle/refshim.py — import the *unmodified* reference from its checkout (build container only).

The DSP modules of the reference only need two incidental imports stubbed:
`friture.audiobackend` for the constants SAMPLING_RATE / FRAMES_PER_BUFFER (audioproc.py:24,
ringbuffer.py:25) and `PyQt6.QtGui.QColor` for colour packing (color_tranform.py:26,44-46).
Its widgets import Qt and the UI modules around them; the one set of stand-ins for those lives here
(Any, QObject, Curve, PlotData, AudioBuffer, module()), and a recorder adds only the modules its own
widget imports.  The stand-ins go into sys.modules and differ between recorders, so
oracle/make_golden.py runs every recorder module in a process of its own.
Used by the recorders that oracle/make_golden.py drives, to validate oracle/dsp.py and to record
golden fixtures; nothing that runs on the GPU box may import this module (the checkout does not
exist there).
"""
import os
import sys
import types

import numpy as np

REFERENCE_ROOT = os.environ.get("FRITURE_REFERENCE", "/root/reference")


def available() -> bool:
    return os.path.isdir(os.path.join(REFERENCE_ROOT, "friture"))


class Any:
    """Accepts every call and attribute: Qt widgets, layouts, signals, axes, settings dialogs."""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return Any()

    def __getattr__(self, name):
        return Any()


class QObject:
    def __init__(self, parent=None, *a, **k):
        pass


class QColor:
    def __init__(self, r, g, b):
        self._v = 0xFF000000 | (int(r) << 16) | (int(g) << 8) | int(b)

    def rgb(self):
        return self._v


class Curve(Any):
    """Curve / FilledCurve: records the arguments of every setData call."""

    def __init__(self, *a, **k):
        self.calls = []

    def setData(self, *args):
        self.calls.append(tuple(np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in args))


class PlotData(Any):
    """Scope_Data / Spectrum_Data / HistPlot_Data: collects the plot items and the labels."""

    def __init__(self, *a, **k):
        self.plot_items = []
        self.fmax = self.fpitch = self.bars = None

    def add_plot_item(self, item):
        self.plot_items.append(item)

    def insert_plot_item(self, i, item):
        self.plot_items.insert(i, item)

    def remove_plot_item(self, item):
        if item in self.plot_items:
            self.plot_items.remove(item)

    def setFmax(self, text, pos):
        self.fmax = (text, pos)

    def setFpitch(self, text, pos):
        self.fpitch = (text, pos)

    def setBarLabels(self, x, fc, y):
        self.bars = (np.array(x, copy=True), fc, np.array(y, copy=True))


class AudioBuffer:
    """AudioBuffer over the reference RingBuffer, remembering the window that data() handed out."""

    def __init__(self):
        from friture.ringbuffer import RingBuffer
        self.ringbuffer = RingBuffer()
        self.lastDataTime = 0.
        self.last = None

    def push(self, x):
        self.ringbuffer.push(x, 0.)

    def data(self, length):
        self.last = self.ringbuffer.data(length)
        return self.last

    def data_indexed(self, start, length):
        return self.ringbuffer.data_indexed(start, length)


def module(name, **attrs):
    """Put a stand-in module holding `attrs` into sys.modules, and onto its package if that is imported."""
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    package, _, leaf = name.rpartition(".")
    if package in sys.modules:
        setattr(sys.modules[package], leaf, m)
    return m


def blank(name):
    """A stand-in module whose every attribute is Any."""
    return module(name, __getattr__=lambda attr: Any)


def install():
    """The reference checkout on sys.path; stand-ins for PyQt6, the audio backend's constants, the store, Scope_Data and Curve."""
    if not available():
        raise RuntimeError(f"reference checkout not found at {REFERENCE_ROOT}")
    sys.dont_write_bytecode = True
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    module("friture.audiobackend", SAMPLING_RATE=48000, FRAMES_PER_BUFFER=512)
    module("PyQt6")
    module("PyQt6.QtGui", QColor=QColor)
    module("PyQt6.QtCore", QObject=QObject, pyqtSignal=Any, pyqtSlot=lambda *a, **k: (lambda f: f),
           pyqtProperty=lambda *a, **k: (lambda f: property(f)), __getattr__=lambda attr: Any)
    blank("PyQt6.QtWidgets")
    module("friture.store", GetStore=lambda: None)
    module("friture.scope_data", Scope_Data=PlotData)
    module("friture.curve", Curve=Curve)
