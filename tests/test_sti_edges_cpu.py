"""The cases of test_sti_edges_gpu.py without a GPU: every builder of tests/sti_helpers.py is run and the conditions that make a
case what it claims to be are asserted on the reference alone; the reference's phase reduction is held to exact rational
arithmetic at the sample rates and frequencies that test_sti_gpu.py never used."""
from fractions import Fraction

import numpy as np
import pytest

import decay_helpers as dh
import sti_helpers as sh

TL = sh.TILE


@pytest.mark.parametrize("fs,freqs", sh.OFF_DEFAULT)
def test_phase_reduction_against_exact_fractions(fs, freqs):
    """cycles() against frac(F t / fs) in exact rationals of the doubles F and fs, at positions on and beside the table seams and
    at the row's far end: within 2e-19 of a cycle (one longdouble rounding of a value below 1, and the division by fs)."""
    t = np.array([0, 1, 63, 64, 4095, 4096, 8194, 65 * 4096 + 7, (1 << 24) - 3])
    for F in freqs:
        got = sh.cycles(F, t, fs)
        for at, c in zip(t.tolist(), got):
            want = Fraction(F) * at / Fraction(fs) % 1
            want = want - 1 if want >= Fraction(1, 2) else want
            d = abs(Fraction(float(c)) - want) if float(c) == c else abs(Fraction(*map(int, np.longdouble(c).as_integer_ratio())) - want)
            assert d <= Fraction(2, 10 ** 19), (F, fs, at, float(d))


@pytest.mark.parametrize("fs,freqs", sh.OFF_DEFAULT)
def test_off_default_cases_on_the_reference(fs, freqs):
    """Every frequency is inside the kernel's range, the float64 restatement lies within n 2^-53 = 1e-12 of the longdouble one (so
    the reference's own sums are not what the 1e-10 bar measures), and m is not 1 everywhere."""
    assert 100 <= fs <= 1e7 and all(0 < F < fs / 2 for F in freqs)
    low, high = [], []
    for f32 in (False, True):
        x, ref = sh.off_default_case(fs, freqs, f32)
        assert x.shape == (3, 2 * TL + 3) and ref[0].shape == (3, len(freqs)) and np.all(np.isfinite(ref[0]))
        m64, e64 = sh.restate_mtf(x, freqs, fs)
        d = sh.distance(m64, ref[0])
        print(fs, "float64 against longdouble:", d, "m", float(ref[0].min()), "..", float(ref[0].max()))
        assert d <= 1e-12 and sh.relative(e64, ref[1]) <= 1e-12
        low.append(float(ref[0].min()))
        high.append(float(ref[0].max()))
    assert min(low) < 0.9 and max(high) <= 1.0
    if fs == 48000:
        assert len(freqs) == 9                                       # eight wavefronts of mtf_finish take one each, one takes a second


def test_strided_probes_on_the_reference():
    x, start, ref = sh.strided_case()
    assert x.shape == (4, 66 * TL + 5) and x.dtype == np.float32 and np.all(np.isfinite(ref[0]))
    assert [int(np.flatnonzero(row)[0]) for row in x] == start.tolist() == list(sh.STRIDED_LEADS)
    spans = dh.live_tiles(start, [x.shape[1]] * 4, TL)
    assert spans.tolist() == [67, 67, 66, 67]
    print("m", float(ref[0].min()), "..", float(ref[0].max()))
    assert ref[0].max() < 0.6 and ref[0].min() > 0.005
    assert all(dh.strided(n, sh.STRIDED_ROWS) and not dh.strided(n, 4) and not dh.strided(n, 101) for n in spans)
    assert (x.shape[1] - 1) * 2.0 ** -53 <= 3.1e-11                  # the bar's derivation at this length: still under 1e-10


def test_live_spans_of_64_and_65_tiles_on_the_reference():
    x, start, stop, ref = sh.live_span_case()
    assert dh.live_tiles(start, stop, TL).tolist() == [64, 65, 64, 65, 64, 65]
    assert set((start // TL).tolist()) == {0, 1} and np.all(np.isfinite(ref[0])) and ref[0].min() < 0.9


def test_two_sample_form_at_44100():
    """The closed form the far-position test uses, at fs = 44100: F = 22049.5 is half a cycle per sample less 1 / 88200, so two
    unit samples 2^24 - 7 apart give |cos(pi (2^24 - 7) 22049.5 / 44100)|; against exact rationals and the float64 cosine."""
    a = (1 << 24) - 7
    for F in (22049.5, 0.63):
        want = Fraction(F) * a / Fraction(44100) % 1
        m = float(sh.two_sample_m(F, a, 1.0, 44100))
        assert abs(m - abs(np.cos(np.pi * float(want)))) <= 1e-15
        assert 0.0 < m < 0.9
