"""The plot curves' cases and CPU restatement, shared by oracle/golden_plotcurves.py, the plot-curve tests and
tools/bench_plotcurves.py: the cases recorded in tests/golden/plotcurves.npz (event lists
regenerated from seeds, never stored), a driver that replays a case on any object with the widgets' methods, and a numpy
restatement of the curve formulas and compute_peaks (friture/spectrumPlotWidget.py:122-200, friture/histplot.py:77-130)."""
from __future__ import annotations

import hashlib

import numpy as np

PEAK_DECAY_RATE = 1.0 - 3e-6
DECAY = 20.0 * np.log10(PEAK_DECAY_RATE) * 5000
SCALES = ["Linear", "Logarithmic", "Mel", "ERB", "Octave", "OctaveC"]
BPOS = [1, 3, 6, 12, 24]
# refreshes of each case whose whole arrays are stored (the others by digest)
FULL_REFRESHES = {"hold_fall": (0, 63, 64, 65, 130, 199), "nan_inf": (5, 20, 21), "ranges": (49, 50, 100),
                  "fft_change": (0, 69, 70, 109, 110), "dual": (39, 40, 89, 90), "hist_bpo3": (0, 64, 150)}


def digest(a):
    """First 8 bytes of the SHA-256 of a float64 array's bytes, as uint64 (0 for None).  Every NaN is hashed as numpy's own NaN:
    the sign and payload of a NaN made by an invalid operation differ between processors, its position does not."""
    if a is None:
        return np.uint64(0)
    a = np.asarray(a, np.float64)
    b = hashlib.sha256(np.ascontiguousarray(np.where(np.isnan(a), np.nan, a)).tobytes()).digest()
    return np.frombuffer(b[:8], np.uint64)[0]


def freqs(B):
    """The frequency vector of a B-bin spectrum (rfft of 2 (B - 1) points at 48 kHz)."""
    return np.linspace(0, 24000., B)


def bands(bpo):
    """(flow, fhigh, fc labels) of a bpo-bands-per-octave bank over 9 octaves around 1 kHz."""
    n = 9 * bpo
    i = np.arange(-(n // 2), n - n // 2)
    f = 1000. * 2. ** (i / bpo)
    fl, fh = f * 2. ** (-1. / (2 * bpo)), f * 2. ** (1. / (2 * bpo))
    return fl, fh, np.array(["%.4g" % v for v in f])


def _row(rng, B, k, loud):
    y = -70. + 6. * rng.standard_normal(B)
    if loud:
        y[rng.integers(0, B, max(1, B // 8))] = -10. + 5. * rng.standard_normal(max(1, B // 8))
    return y


def spectrum_events(name):
    """Events of a SpectrumPlot case: ("data", x, y, fmax, fpitch) and setter calls (method name, args)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    ev = [("setspecrange", (-100., 0.)), ("setfreqscale", ("Logarithmic",)), ("setfreqrange", (20., 22000.))]

    def data(B, k, loud=False):
        y = _row(rng, B, k, loud)
        fmax = float(rng.choice([55.25, 199.95, 200., 1234.5, 15000.7]))
        fpitch = float(rng.choice([0., 61.7, 440., 999.6, 1000., 3520.2]))
        return ("data", freqs(B), y, fmax, fpitch)

    if name == "hold_fall":                                  # loud for 10 refreshes, then the 64-refresh hold and a long fall
        ev += [data(64, k, loud=k < 10) for k in range(200)]
    elif name == "nan_inf":
        for k in range(160):
            e = data(64, k, loud=k % 17 == 0)
            y = e[2]
            if k % 5 == 0:
                y[rng.integers(0, 64, 3)] = np.nan
            if k in (20, 90):
                y[:] = np.nan
            if k % 7 == 0:
                y[rng.integers(0, 64)] = np.inf
            if k % 11 == 0:
                y[rng.integers(0, 64, 2)] = -np.inf
            ev.append(e)
    elif name == "ranges":
        ev = [("setspecrange", (0., -100.)), ("setfreqscale", ("Linear",)), ("setfreqrange", (0., 24000.))]
        for k in range(150):
            if k == 50:
                ev.append(("setspecrange", (-50., -50.)))
            if k == 100:
                ev.append(("setspecrange", (-120., -20.)))
            ev.append(data(32, k, loud=k % 40 == 0))
            if k in (60, 61):
                ev[-1][2][3] = np.inf
    elif name == "fft_change":                               # the three-element initial state, then two FFT sizes
        ev += [data(3, k, loud=k < 3) for k in range(70)]
        ev += [data(65, k, loud=k == 0) for k in range(40)]
        ev += [data(129, k, loud=k % 30 == 0) for k in range(40)]
    elif name == "dual":                                     # peaks off (dual channels) and on again, a bin change while off
        for k in range(160):
            if k == 40:
                ev += [("set_peaks_enabled", (False,)), ("set_baseline_dataUnits", (0.,))]
            if k == 90:
                ev += [("set_peaks_enabled", (True,)), ("set_baseline_displayUnits", (0.,))]
            if k == 120:
                ev += [("set_peaks_enabled", (False,)), ("set_baseline_dataUnits", (0.,))]
            if k == 140:
                ev += [("set_peaks_enabled", (True,)), ("set_baseline_displayUnits", (0.,))]
            ev.append(data(48 if k < 130 else 40, k, loud=k % 50 == 0))
    elif name == "pause":
        for k in range(150):
            if k == 30:
                ev.append(("pause", ()))
            if k == 45:
                ev.append(("setspecrange", (-90., 10.)))
            if k == 60:
                ev.append(("restart", ()))
            ev.append(data(40, k, loud=k % 25 == 0))
    elif name.startswith("scale_"):
        scale = name[len("scale_"):]
        ev = [("setspecrange", (-100., -10.)), ("set_baseline_dataUnits", (0.,)), ("setfreqscale", (scale,)),
              ("setfreqrange", (20., 20000.))]
        ev += [data(33, k, loud=k == 0) for k in range(12)]
        ev.append(("setfreqrange", (100., 8000.)))
        ev += [data(33, k) for k in range(4)]
    return ev


def hist_events(name):
    bpo = int(name[len("hist_bpo"):])
    rng = np.random.default_rng(1000 + bpo)
    fl, fh, fc = bands(bpo)
    n = fl.shape[0]
    ev = [("setspecrange", (-80., 0.))]
    K = 160 if bpo == 3 else 70
    for k in range(K):
        y = _row(rng, n, k, k % 60 == 0)
        if bpo == 3 and k in (30, 31):
            y[rng.integers(0, n, 2)] = np.nan
        if bpo == 3 and k == 100:
            ev.append(("pause", ()))
        if bpo == 3 and k == 110:
            ev.append(("restart", ()))
        if bpo == 3 and k == 120:
            ev.append(("setspecrange", (0., -60.)))
        ev.append(("data", fl, fh, fc, y))
    return ev


SPECTRUM_CASES = ["hold_fall", "nan_inf", "ranges", "fft_change", "dual", "pause"] + ["scale_" + s for s in SCALES]
HIST_CASES = ["hist_bpo%d" % b for b in BPOS]


def events(name):
    return hist_events(name) if name.startswith("hist_") else spectrum_events(name)


def replay(name, widget, fscales):
    """Apply a case's events to `widget` (scale names resolved in the module `fscales`); yields the index of every data event
    after the widget's setdata ran."""
    by_name = {c.NAME: c for c in (fscales.Linear, fscales.Logarithmic, fscales.Mel, fscales.Erb, fscales.Octave, fscales.OctaveC)}
    k = 0
    for ev in events(name):
        if ev[0] == "data":
            widget.setdata(*ev[1:])
            yield k
            k += 1
        elif ev[0] == "setfreqscale":
            widget.setfreqscale(by_name[ev[1][0]])
        else:
            getattr(widget, ev[0])(*ev[1])


# ---- numpy restatement ------------------------------------------------------------------------------------------------------

def to_screen_linear(v, cmin, cmax):
    if cmax == cmin:
        return 0 + 0. * v
    return (v - cmin) * 1 / (cmax - cmin) + 0


def curves_np(y, cmin, cmax):
    """scaled_y, z of one refresh."""
    M = np.max(y)
    return 1.0 - to_screen_linear(y, cmin, cmax), (y - cmin) / (np.abs(M - cmin) + 1e-3)


def peaks_np(y, peak, pint, decay):
    """One compute_peaks step on copies of the state (no reset): returns the new (peak, int, decay)."""
    peak, pint, decay = peak.copy(), pint.copy(), decay.copy()
    m1 = peak < y
    m2 = ~m1
    m2a = m2 * (pint < 0.2)
    m2b = m2 * (pint >= 0.2)
    peak[m1] = y[m1]
    peak[m2a] = peak[m2a] + decay[m2a]
    decay[m1] = DECAY
    decay[m2a] += DECAY
    pint[m1] = 1.0
    pint[m2b] *= 0.975
    return peak, pint, decay


def batch_np(y, state, cmin, cmax):
    """[S, R, B] dB rows from state [S, 3, B]: (scaled_y, z, scaled_peak, z_peak, final state), all [S, R, B] float64."""
    y = np.asarray(y, np.float64)
    S, R, B = y.shape
    out = [np.empty((S, R, B)) for _ in range(4)]
    st = np.array(state, np.float64, copy=True)
    for s in range(S):
        pk, pi, dc = st[s, 0], st[s, 1], st[s, 2]
        for r in range(R):
            out[0][s, r], out[1][s, r] = curves_np(y[s, r], cmin, cmax)
            pk, pi, dc = peaks_np(y[s, r], pk, pi, dc)
            out[2][s, r] = 1.0 - to_screen_linear(pk, cmin, cmax)
            out[3][s, r] = pi
        st[s] = pk, pi, dc
    return (*out, st)


class NumpyCurves:
    """The widgets' per-refresh numpy body (curves and peaks only, no edges): the restatement the bench compares against."""

    def __init__(self, cmin=-100., cmax=0.):
        self.cmin, self.cmax = cmin, cmax
        self.peak, self.peak_int, self.peak_decay = np.zeros(3), np.zeros(3), np.ones(3) * PEAK_DECAY_RATE

    def setdata(self, y):
        sy, z = curves_np(y, self.cmin, self.cmax)
        if len(self.peak) != len(y):
            self.peak, self.peak_int, self.peak_decay = np.ones(y.shape) * -500., np.zeros(y.shape), np.ones(y.shape) * DECAY
        m1 = self.peak < y
        m2 = ~m1
        m2a = m2 * (self.peak_int < 0.2)
        m2b = m2 * (self.peak_int >= 0.2)
        self.peak[m1] = y[m1]
        self.peak[m2a] = self.peak[m2a] + self.peak_decay[m2a]
        self.peak_decay[m1] = DECAY
        self.peak_decay[m2a] += DECAY
        self.peak_int[m1] = 1.0
        self.peak_int[m2b] *= 0.975
        return sy, z, 1.0 - to_screen_linear(self.peak, self.cmin, self.cmax), self.peak_int
