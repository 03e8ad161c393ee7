"""The plot curves without a GPU: host edges, labels and baselines of friture_amd.plotcurves and the numpy restatement of
oracle/plotcurves.py against tests/golden/plotcurves.npz (recorded from the reference SpectrumPlotWidget and HistPlot),
bit for bit; the decay step the kernel carries; the C ABI entry points."""
from pathlib import Path

import numpy as np
import pytest

from oracle import plotcurves as H
from plotcurves_helpers import check_case

GOLDEN = Path(__file__).resolve().parent / "golden" / "plotcurves.npz"
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _numpy_widget(cls):
    """The widget class with its device call replaced by the numpy restatement (host edges and labels unchanged)."""

    class W(cls):
        def _curves(self, y, peaks):
            y = np.asarray(y, np.float64)
            cmin, cmax = self.vertical.coord_min, self.vertical.coord_max
            sy, z = H.curves_np(y, cmin, cmax)
            if not peaks:
                return np.array([sy, z])
            if self._state is None or self._state.shape[1] != y.shape[0]:
                from friture_amd.plotcurves import reset_state
                self._state = self._state_host if self._state is None and y.shape[0] == 3 else reset_state(y.shape[0])
            self._state = np.array(H.peaks_np(y, *self._state))
            return np.array([sy, z, 1.0 - H.to_screen_linear(self._state[0], cmin, cmax), self._state[1]])

        def peak_state(self):
            st = self._state_host if self._state is None else self._state
            return st[0], st[1], st[2]
    return W


@pytest.mark.parametrize("name", H.SPECTRUM_CASES)
def test_spectrum_host_parts_and_restatement_match_reference(g, name):
    from friture_amd.plotcurves import SpectrumPlot
    with np.errstate(invalid="ignore"):
        check_case(g, name, _numpy_widget(SpectrumPlot)())


@pytest.mark.parametrize("name", H.HIST_CASES)
def test_histplot_host_parts_and_restatement_match_reference(g, name):
    from friture_amd.plotcurves import HistPlot
    with np.errstate(invalid="ignore"):
        check_case(g, name, _numpy_widget(HistPlot)())


def test_cases_cover_the_issue(g):
    """>= 150 refreshes past the hold, a whole NaN row, +-inf, equal and swapped ranges, the three-element state, peaks off
    while the bin count changes, pause, both baselines, all six scales and five bands-per-octave."""
    assert len(g["hold_fall_drew"]) >= 150 and len(g["hist_bpo3_drew"]) >= 150
    ev = H.events("nan_inf")
    rows = [e[2] for e in ev if e[0] == "data"]
    assert any(np.isnan(r).all() for r in rows) and any(np.isposinf(r).any() for r in rows) and any(np.isneginf(r).any() for r in rows)
    ranges = [e[1] for e in H.events("ranges") if e[0] == "setspecrange"]
    assert any(a > b for a, b in ranges) and any(a == b for a, b in ranges)
    assert [e[2].shape[0] for e in H.events("fft_change") if e[0] == "data"][0] == 3
    assert (~g["dual_peakset"]).sum() > 0 and (~g["pause_drew"]).sum() == 30
    assert len(set(np.round(g["dual_baseline"], 12))) == 2
    assert all(f"scale_{s}_dig" in g.files for s in H.SCALES) and all(f"hist_bpo{b}_dig" in g.files for b in H.BPOS)


def test_decay_step_is_numpys():
    from friture_amd import _lib
    from friture_amd.plotcurves import PEAK_DECAY_STEP
    c = _lib.load().frt_curves_decay_step()
    assert c == H.DECAY == PEAK_DECAY_STEP == 20.0 * np.log10(1.0 - 3e-6) * 5000


def test_hold_lasts_64_refreshes_then_falls_c_2c_3c():
    """Restatement properties: after a new peak the level holds while int >= 0.2 (64 refreshes), then steps by c, 2c, ..."""
    peak, pint, dec = np.array([-500.]), np.array([0.]), np.array([H.DECAY])
    peak, pint, dec = H.peaks_np(np.array([0.]), peak, pint, dec)
    held = 0
    while True:
        p2, pint, dec = H.peaks_np(np.array([-100.]), peak, pint, dec)
        if p2[0] != peak[0]:
            break
        held += 1
    assert held == 64 and 0.975 ** 64 < 0.2 <= 0.975 ** 63
    assert p2[0] == 0. + H.DECAY
    p3, _, _ = H.peaks_np(np.array([-100.]), p2, pint, dec)
    assert p3[0] == p2[0] + 2 * H.DECAY


def test_curves_entry_points_declared_and_bound():
    from friture_amd import _lib
    header = (ROOT / "include" / "friture_hip.h").read_text()
    for name in ("frt_curves_run", "frt_curves_decay_step"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(_lib.load(), name)


def test_screen_transform_matches_the_restatement_on_linear():
    from friture_amd.plotcurves import ScreenTransform
    t = ScreenTransform(-100., 0.)
    y = np.array([-120., -50., 0., np.inf, -np.inf, np.nan])
    assert np.array_equal(1.0 - t.toScreen(y), 1.0 - H.to_screen_linear(y, -100., 0.), equal_nan=True)
    t.setRange(-50., -50.)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(t.toScreen(y), [0, 0, 0, np.nan, np.nan, np.nan], equal_nan=True)
