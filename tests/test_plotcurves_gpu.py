"""The plot curves on the GPU (curves.hip) against tests/golden/plotcurves.npz (the reference SpectrumPlotWidget and HistPlot) and
against themselves (batch vs widget, dtypes, host vs device memory, carried state, keep="last", streams, the restatement)."""
from pathlib import Path

import numpy as np
import pytest

from oracle import plotcurves as H
from plotcurves_helpers import check_case

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "plotcurves.npz"


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _eq(a, b):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    b = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _rows(rng, S, R, B, holes=True):
    y = -60. + 15. * rng.standard_normal((S, R, B))
    y[rng.random((S, R, B)) < 0.02] += 50.
    if holes:
        y[rng.random((S, R, B)) < 0.002] = np.nan
        y[rng.random((S, R, B)) < 0.001] = np.inf
        y[rng.random((S, R, B)) < 0.001] = -np.inf
        y[0, R // 2] = np.nan                                   # a whole NaN row
    return y


@pytest.mark.parametrize("name", H.SPECTRUM_CASES)
def test_spectrum_plot_matches_reference(g, name):
    from friture_amd.plotcurves import SpectrumPlot
    check_case(g, name, SpectrumPlot())


@pytest.mark.parametrize("name", H.HIST_CASES)
def test_histplot_matches_reference(g, name):
    from friture_amd.plotcurves import HistPlot
    check_case(g, name, HistPlot())


def test_batch_equals_widget():
    from friture_amd.plotcurves import CurveBatch, HistPlot
    fl, fh, fc = H.bands(3)
    y = _rows(np.random.default_rng(1), 1, 150, fl.shape[0])
    w = HistPlot()
    w.setspecrange(0., -90.)
    rows = []
    for r in range(150):
        w.setdata(fl, fh, fc, y[0, r])
        rows.append([w.signal[2], w.signal[3], w.peak[2], w.peak[3]])
    res = CurveBatch(0., -90.).run(y)
    for i in range(4):
        assert _eq(res[i][0], np.array([row[i] for row in rows]))
    assert _eq(res.state[0], np.array(w.peak_state()))


def test_float32_equals_float64_of_same_values():
    from friture_amd.plotcurves import CurveBatch
    y32 = _rows(np.random.default_rng(2), 3, 70, 27).astype(np.float32)
    cb = CurveBatch(-100., 0.)
    a, b = cb.run(y32), cb.run(y32.astype(np.float64))
    for u, v in zip(a, b):
        assert _eq(u, v)


def test_host_input_equals_device_input():
    import torch
    from friture_amd.plotcurves import CurveBatch
    y = _rows(np.random.default_rng(3), 4, 80, 513)
    cb = CurveBatch(-120., -10.)
    h, d = cb.run(y), cb.run(torch.from_numpy(y).cuda())
    assert all(hasattr(v, "is_cuda") and v.is_cuda for v in d)
    for u, v in zip(h, d):
        assert _eq(u, v)
    f32 = torch.from_numpy(y.astype(np.float32)).cuda()
    for u, v in zip(cb.run(y.astype(np.float32)), cb.run(f32)):
        assert _eq(u, v)


def test_two_batches_with_carried_state_equal_one():
    from friture_amd.plotcurves import CurveBatch
    y = _rows(np.random.default_rng(4), 2, 200, 100)
    cb = CurveBatch(-100., 0.)
    one = cb.run(y)
    a = cb.run(y[:, :77])
    b = cb.run(y[:, 77:], state=a.state)
    for i in range(4):
        assert _eq(one[i], np.concatenate([a[i], b[i]], axis=1))
    assert _eq(one.state, b.state)


def test_keep_last_equals_last_row_of_all():
    import torch
    from friture_amd.plotcurves import CurveBatch
    y = _rows(np.random.default_rng(5), 3, 150, 257)
    cb = CurveBatch(-100., 0.)
    for inp in (y, torch.from_numpy(y).cuda()):
        full, last = cb.run(inp), cb.run(inp, keep="last")
        for i in range(4):
            assert _eq(last[i], full[i][:, -1:])
        assert _eq(last.state, full.state)


def test_streams_are_independent():
    from friture_amd.plotcurves import CurveBatch, initial_state
    rng = np.random.default_rng(6)
    y = _rows(rng, 5, 90, 40)
    st = initial_state(40, 5)
    st[2] = np.array(H.peaks_np(y[2, 0] + 5., *st[2]))       # one stream starts from a carried state
    cb = CurveBatch(-80., -5.)
    allr = cb.run(y, state=st)
    for s in range(5):
        one = cb.run(y[s], state=st[s])
        for i in range(4):
            assert _eq(allr[i][s], one[i])
        assert _eq(allr.state[s], one.state)


def test_strided_energies_layout_read_in_place():
    """A [C][blocks][bands] float32 tensor with a padded block stride (as FirBank.energies' rows in a larger buffer)."""
    import torch
    from friture_amd.plotcurves import CurveBatch
    y = _rows(np.random.default_rng(7), 4, 130, 27).astype(np.float32)
    buf = torch.zeros((4, 130, 32), dtype=torch.float32, device="cuda")
    buf[:, :, :27] = torch.from_numpy(y).cuda()
    view = buf[:, :, :27]
    assert not view.is_contiguous()
    cb = CurveBatch(-100., 0.)
    for u, v in zip(cb.run(view), cb.run(y)):
        assert _eq(u, v)


@pytest.mark.parametrize("S,R,B,rng_", [(8, 300, 1025, (-100., 0.)), (64, 64, 27, (-50., -50.)), (3, 2, 3, (10., -10.))])
def test_large_random_equals_restatement(S, R, B, rng_):
    from friture_amd.plotcurves import CurveBatch, initial_state
    y = _rows(np.random.default_rng(S * R + B), S, R, B)
    cb = CurveBatch(*rng_)
    res = cb.run(y)
    with np.errstate(invalid="ignore"):
        ref = H.batch_np(y, initial_state(B, S), cb.spec_min, cb.spec_max)
    for u, v in zip(res, ref):
        assert _eq(u, v)


def test_peaks_off_freezes_state_and_widget_state_lives_on_device():
    from friture_amd.plotcurves import SpectrumPlot
    w = SpectrumPlot()
    w.setspecrange(-100., 0.)
    x = H.freqs(16)
    rng = np.random.default_rng(8)
    for _ in range(5):
        w.setdata(x, -50. + 10. * rng.standard_normal(16), 100., 440.)
    assert w._state.is_cuda
    before = w.peak_state()
    w.set_peaks_enabled(False)
    w.setdata(H.freqs(20), -40. + rng.standard_normal(20), 100., 440.)
    after = w.peak_state()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
