"""Record levels.npz from the reference's own Levels_Widget, LongLevelWidget and Subsampler.

Driven by oracle/make_golden.py (needs the reference checkout): the stand-ins of oracle/refshim.py plus the two settings
dialogs, then the reference classes are driven chunk by chunk on the signals of oracle/levels.py (regenerated from seeds
there, never stored).  Recorded per meter step: rms, old_max, level_rms, level_max, peak_iec, the BallisticPeak branch (0 follow, 1 hold,
2 decay, 3 decay below the input) and the margins of its comparisons; per long-level block: level and dB; the Subsampler's
outputs; the curves handed to Curve.setData around setduration / setmin / setmax / setresptime; the coefficients.
"""
from __future__ import annotations

import hashlib
import types

import numpy as np

from . import levels as H
from . import refshim


def install_stubs():
    refshim.install()
    refshim.module("friture.levels_settings", Levels_Settings_Dialog=refshim.Any)
    refshim.module("friture.longlevels_settings", LongLevels_Settings_Dialog=refshim.Any, DEFAULT_LEVEL_MIN=-70,
                   DEFAULT_LEVEL_MAX=-20, DEFAULT_MAXTIME=600, DEFAULT_RESPONSE_TIME=20)


class _BallisticProbe:
    """level_data_ballistic stand-in: records the branch the reference BallisticPeak takes, then forwards the value."""

    def __init__(self, inner, log):
        self._inner, self._log = inner, log

    @property
    def peak_iec(self):
        return self._inner.peak_iec

    @peak_iec.setter
    def peak_iec(self, v):
        from friture.ballistic_peak import PEAK_FALLOFF
        b = self._inner
        p0, hold, f0 = float(b._peak_iec), b._peak_hold_counter, b._peak_decay_factor
        m_follow = v - p0
        if v > p0:
            branch, m_decay = 0, np.nan
        elif hold + 1 <= PEAK_FALLOFF:
            branch, m_decay = 1, np.nan
        else:
            m_decay = f0 * p0 - v
            branch = 3 if f0 * p0 < v else 2
        b.peak_iec = v
        self._log.append((v, branch, m_follow, m_decay, float(b._peak_iec)))


def run_levels(x, sizes=None):
    from friture.ballistic_peak import BallisticPeak
    from friture.levels import Levels_Widget
    logs = [[], []]
    vm = types.SimpleNamespace(two_channels=False, level_data=types.SimpleNamespace(), level_data_2=types.SimpleNamespace(),
                               level_data_ballistic=_BallisticProbe(BallisticPeak(), logs[0]),
                               level_data_ballistic_2=_BallisticProbe(BallisticPeak(), logs[1]))
    w = Levels_Widget.__new__(Levels_Widget)
    Levels_Widget.__init__(w, None, vm)
    rows = [[], []]
    for s, n in H.chunks(x.shape[1], sizes):
        Levels_Widget.handle_new_data(w, x[:, s:s + n])
        for c, (d, rms, mx) in enumerate([(vm.level_data, w.old_rms, w.old_max), (vm.level_data_2, w.old_rms_2, w.old_max_2)][:x.shape[0]]):
            v, branch, m1, m2, peak = logs[c][-1]
            rows[c].append([rms, mx, float(d.level_rms), float(d.level_max), peak, branch, m1, m2, v])
    return np.array(rows[:x.shape[0]]), w


def long_widget(rt):
    from friture.longlevels import LongLevelWidget
    w = LongLevelWidget.__new__(LongLevelWidget)
    LongLevelWidget.__init__(w, None)
    w.setresptime(rt)
    w.audiobuffer = refshim.AudioBuffer()
    return w


def run_long(x, rt, sizes=None):
    from friture.longlevels import LongLevelWidget
    w = long_widget(rt)
    out = []
    for s, n in H.chunks(x.shape[1], sizes):
        w.audiobuffer.push(x[:, s:s + n])
        before = w.ringbuffer.offset
        LongLevelWidget.handle_new_data(w, x[:, s:s + n])
        if w.ringbuffer.offset > before:
            out.append(w.ringbuffer.data(w.ringbuffer.offset - before)[0].copy())
        # the level of the last block, linear: the FIR's output
    return w, (np.concatenate(out) if out else np.zeros(0))


def run_long_linear(x, rt):
    """The linear levels of every block, read from the widget's FIR output after each block."""
    from friture.longlevels import LongLevelWidget
    w = long_widget(rt)
    lin, db = [], []
    B = 2 ** w.Ndec
    for s in range(0, x.shape[1] - B + 1, B):
        w.audiobuffer.push(x[:, s:s + B])
        LongLevelWidget.handle_new_data(w, x[:, s:s + B])
        lin.append(float(w.level[0]))
        db.append(float(np.asarray(w.level_rms).reshape(-1)[0]))
    return np.array(lin), np.array(db)


def levels(out_dir):
    install_stubs()
    from friture.longlevels import LongLevelWidget, Subsampler, gauss
    from friture.levels import Levels_Widget
    g = {}
    # coefficients
    w = Levels_Widget.__new__(Levels_Widget)
    Levels_Widget.__init__(w, None, types.SimpleNamespace())
    g["alpha"], g["alpha2"] = np.float64(w.alpha), np.float64(w.alpha2)
    g["kernel_len"] = np.int64(w.kernel.shape[0])
    g["kernel_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(w.kernel, np.float64).tobytes()).hexdigest())
    g["kernel_head"], g["kernel_tail"] = w.kernel[:16].copy(), w.kernel[-600:].copy()
    g["gauss11"], g["gauss41"] = np.array(gauss(11, 2.)), np.array(gauss(41, 8.))
    lw = long_widget(20)
    nd = []
    for rt in range(1, 21):
        lw.setresptime(rt)
        nd.append(lw.Ndec)
    g["ndec_rt1_20"] = np.array(nd)
    # meters
    for name in ["noise", "bursts", "impulse", "stereo"]:
        g[f"meters_{name}"] = run_levels(H.signal(name))[0]
    g["meters_irregular"] = run_levels(H.signal("irregular"), H.IRREGULAR_CHUNKS)[0]
    # long levels: linear and dB per block (blocks fed one by one), and through irregular chunks
    for name, rts in [("noise", (1, 4, 20)), ("bursts", (4,)), ("impulse", (1,)), ("stereo", (20,))]:
        x = H.signal(name)
        for rt in rts:
            g[f"long_{name}_rt{rt}_lin"], g[f"long_{name}_rt{rt}_db"] = run_long_linear(x, rt)
    _, g["long_irregular_rt1_db"] = run_long(H.signal("irregular"), 1, H.IRREGULAR_CHUNKS)
    # Subsampler pushes of irregular sizes
    xs = H.signal("subsampler")
    for ndec in (8, 13):
        s = Subsampler(ndec)
        outs, pos = [], 0
        for n in H.SUBSAMPLER_PUSHES:
            outs.append(s.push(xs[pos:pos + n]))
            pos += n
        g[f"subsampler_{ndec}"] = np.concatenate(outs)
        g[f"subsampler_{ndec}_lengths"] = np.array([o.shape[0] for o in outs])
    # curves around the settings changes
    x = H.signal("curve")
    w = long_widget(4)
    w.setduration(30)
    pos, k = 0, 0
    for step, v in H.CURVE_STEPS:
        if step == "push":
            for _ in range(v):
                w.audiobuffer.push(x[:, pos:pos + H.CHUNK])
                LongLevelWidget.handle_new_data(w, x[:, pos:pos + H.CHUNK])
                pos += H.CHUNK
            t, y = w._curve.calls[-1]
            g[f"curve_{k}_t"], g[f"curve_{k}_y"] = t, y
            g[f"curve_{k}_calls"] = np.int64(len(w._curve.calls))
            k += 1
        else:
            getattr(w, step)(v)
    np.savez_compressed(out_dir / "levels.npz", **g)
