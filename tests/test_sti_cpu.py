"""MtfBatch and the STI steps without a GPU: the numpy restatement (tests/sti_helpers.py) against closed forms, the properties
of the index's steps on the restatement, the argument checks that come before the library, and the binding table."""
import math

import numpy as np
import pytest

import sti_helpers as sh
from friture_amd import _lib, sti

FS = 48000


@pytest.mark.parametrize("real", [np.float64, np.longdouble])
def test_restatement_gives_the_closed_form_of_an_exponential(real):
    """e[t] = r^t, r = 10^(-6 / (rt fs)), given as x[t] = r^(t / 2) in float64: m_j = |(1 - z^T) / (1 - z)| (1 - r) / (1 - r^T), z = r
    exp(-2 pi i F_j / fs).  Each e[t] is a rounded square of a rounded power, within 4 2^-53 of r^t, which moves m by at most
    8 2^-53 = 9e-16; a float64 sum of T = 4096 terms adds at most T 2^-53 = 4.5e-13 to each of the two sums: 1e-12 in float64,
    1e-14 in longdouble (the input's 9e-16 and sums at 2^-64)."""
    T, rt = 4096, 0.05
    r = 10.0 ** (-6.0 / (rt * FS))
    m, energy = sh.restate_mtf((r ** (np.arange(T) / 2.0))[None], real=real)
    want = np.array([sh.exponential_m(F, rt, FS, T) for F in sh.MOD_FREQS])
    d = sh.distance(m[0], want)
    print(real.__name__, "m", d, "energy", sh.relative(energy[0], (1 - r ** T) / (1 - r)))
    assert d <= (1e-12 if real is np.float64 else 1e-14)
    assert sh.relative(energy[0], (1 - r ** T) / (1 - r)) <= 1e-12
    assert 0.2 < m[0, -1] < m[0, 0] < 1 and np.all(np.diff(m[0]) < 0)


def test_restatement_against_the_textbook_formula():
    """The continuous decay e(t) = exp(-k fs t), k = 13.8 / (rt fs), has m = 1 / sqrt(1 + (2 pi F rt / 13.8)^2) = 1 / sqrt(1 + a^2),
    a = theta / k, theta = 2 pi F / fs.  The samples e[t] = exp(-k t) = r^t give 1 / sqrt(1 + b^2), b^2 = 4 r sin^2(theta / 2) /
    (1 - r)^2 = a^2 (1 - (k^2 + theta^2) / 12 + higher orders): b^2 is a^2 within eps = 1.01 (k^2 + theta^2) / 12.  d/d(a^2) of
    (1 + a^2)^(-1/2) is -(1 + a^2)^(-3/2) / 2, and a^2 (1 + a^2)^(-3/2) <= 0.385, so |m - textbook| <= 0.2 eps; a row cut at T
    adds at most 2 r^T.  At rt = 0.5 s and 48 kHz that is 5e-8 at 12.5 Hz, far below the 4e-4 by which 13.8 differs from 6 ln 10."""
    rt, T = 0.5, 1 << 16
    k = 13.8 / (rt * FS)
    x = np.exp(-k * np.arange(T) / 2)[None]
    m, _ = sh.restate_mtf(x, real=np.longdouble)
    for j, F in enumerate(sh.MOD_FREQS):
        theta = 2 * math.pi * F / FS
        bound = 0.2 * 1.01 * (k * k + theta * theta) / 12 + 2 * math.exp(-k * T) + 1e-14
        d = abs(float(m[0, j]) - 1 / math.sqrt(1 + (2 * math.pi * F * rt / 13.8) ** 2))
        print(F, d, bound)
        assert d <= bound < 1e-7


@pytest.mark.parametrize("real", [np.float64, np.longdouble])
def test_restatement_of_two_samples(real):
    """Two samples a apart with the amplitudes 1 and g: |1 + g^2 exp(-2 pi i F a / fs)| / (1 + g^2), wherever the pair sits and
    whatever interval holds it; an interval that holds one of them gives 1."""
    T, at, a, g = 50000, 123, 48000 - 77, 0.75
    x = np.zeros((3, T))
    x[:, at], x[:, at + a] = 1.0, g
    m, energy = sh.restate_mtf(x, start=[0, at, at + 1], stop=[T, at + a + 1, T], real=real)
    want = np.array([sh.two_sample_m(F, a, g, FS) for F in sh.MOD_FREQS])
    print(sh.distance(m[0], want), sh.distance(m[1], want), sh.distance(m[2], 1.0))
    assert sh.distance(m[0], want) <= 1e-15 and sh.distance(m[1], want) <= 1e-15 and sh.distance(m[2], 1.0) <= 1e-15
    assert np.allclose(energy, [1 + g * g, 1 + g * g, g * g], rtol=1e-15)
    assert np.min(want) < 0.5 < np.max(want)


def test_restatement_of_dead_rows():
    x = np.ones((4, 100))
    x[0] = 0.0
    x[1, 50] = math.nan
    x[2, 50] = math.inf
    m, energy = sh.restate_mtf(x, start=[0, 0, 0, 10], stop=[100, 100, 50, 60])
    assert np.all(np.isnan(m[:2])) and energy[0] == 0 and np.all(np.isfinite(m[2:]))


def test_weights_sum_to_one_and_the_constants_are_the_annex():
    for voice in ("male", "female"):
        alpha, beta = sti.WEIGHTS[voice]
        assert abs(sum(alpha) - sum(beta) - 1) <= 1e-12
        assert alpha == sh.ALPHA[voice] and beta == sh.BETA[voice]
        assert sti.SPEECH_SPECTRUM_DB[voice] == sh.SPEECH_DB[voice]
    assert sti.MOD_FREQS == sh.MOD_FREQS and sti.RECEPTION_DB == sh.RECEPTION_DB


def test_masking_function_is_continuous_at_its_seams():
    for L in (63.0, 67.0):
        below, above = sh.masking_db(math.nextafter(L, 0)), sh.masking_db(L)
        print(L, below, above)
        assert abs(below - above) <= 1e-9
    assert sh.masking_db(62.0) == -34.0 and sh.masking_db(65.0) == pytest.approx(-29.9) and sh.masking_db(100.0) == -10.0
    assert sh.masking_db(math.nextafter(100.0, 0)) == pytest.approx(-9.8)      # the standard's own step at 100 dB


def test_index_at_its_ends_and_without_a_correction():
    """m = 1 everywhere gives 1.  TI reaches 0 at m / (1 - m) = 10^-1.5, m = 0.030653: at and below 0.0306 the index is exactly 0
    (0.0307, the threshold rounded up, already gives TI = 2.3e-4).  snr_db = +inf is no correction."""
    for voice in ("male", "female"):
        assert sh.restate_sti(np.ones((1, 7, 14)), weights=voice)["sti"][0] == pytest.approx(1.0, abs=1e-12)
        for low in (0.0306, 0.01, 0.0, -0.5):
            res = sh.restate_sti(np.full((1, 7, 14), low), weights=voice)
            assert res["sti"][0] == 0 and np.all(res["ti"] == 0)
    assert 10 ** -1.5 / (1 + 10 ** -1.5) == pytest.approx(0.030653, abs=1e-6)
    assert 0 < sh.restate_sti(np.full((1, 7, 14), 0.0307))["sti"][0] < 3e-4
    m = np.random.default_rng(1).uniform(0.0, 1.0, (4, 7, 14))
    plain, inf = sh.restate_sti(m), sh.restate_sti(m, snr_db=np.full(7, math.inf))
    for f in ("sti", "mti", "ti"):
        assert np.array_equal(plain[f], inf[f])
    halved = sh.restate_sti(m, snr_db=np.zeros(7))
    assert np.all(halved["sti"] < plain["sti"])
    assert np.all(sh.restate_sti(np.where(np.arange(14) == 3, np.nan, m))["sti"] != sh.restate_sti(m)["sti"])   # NaN: a used column
    mask = np.ones((7, 14), bool)
    mask[:, 3] = False
    assert np.all(np.isfinite(sh.restate_sti(np.where(np.arange(14) == 3, np.nan, m), scheme=mask)["sti"]))      # an unused one


def test_index_falls_with_the_reverberation_time():
    rts = np.array([0.2, 0.4, 0.8, 1.6, 3.2, 6.4])
    F = np.array(sh.MOD_FREQS)
    m = 1 / np.sqrt(1 + (2 * math.pi * F[None, None, :] * rts[:, None, None] / 13.8) ** 2) * np.ones((1, 7, 1))
    for kw in ({}, {"scheme": "stipa"}, {"weights": "female"}, {"level_db": sh.SPEECH_DB["male"] + np.float64(65.0), "noise_db": np.full(7, 35.0)}):
        got = sh.restate_sti(m, **kw)["sti"]
        print(kw.keys(), got)
        assert np.all(np.diff(got) < 0) and 0 < got[-1] < got[0] < 1


def test_stipa_mask_has_two_columns_per_band():
    assert sti.STIPA.shape == (7, 14) and sti.STIPA.dtype == bool
    assert np.all(sti.STIPA.sum(axis=1) == 2) and np.all(sti.STIPA.sum(axis=0) == 1)
    assert np.array_equal(sti.STIPA, sh.stipa_mask())
    assert [tuple(np.array(sti.MOD_FREQS)[row]) for row in sti.STIPA] == [tuple(sorted(p)) for p in sh.STIPA_HZ]


def test_speech_levels_and_the_octave_bands():
    assert np.allclose(sti.speech_levels(60.0, "male"), [62.9, 62.9, 59.2, 53.2, 47.2, 41.2, 35.2], rtol=0, atol=1e-12)
    female = sti.speech_levels(60, "female")
    assert female[0] == -math.inf and np.allclose(female[1:], [65.3, 58.1, 50.9, 44.2, 43.3, 42.0], rtol=0, atol=1e-12)
    for bad in ((60.0, "child"), (math.nan, "male"), ("60", "male")):
        with pytest.raises(ValueError):
            sti.speech_levels(*bad)
    from friture_amd import decay
    centres, edges = decay.band_edges(sti.octave_bands())
    assert centres.shape == (7,) and np.allclose(centres, [1000 * 10 ** (0.3 * k) for k in range(-3, 4)], rtol=1e-12)
    assert np.allclose(edges[:6], decay.band_edges("octave")[1], rtol=1e-12) and decay.band_edges("octave")[0].shape == (6,)
    for f_lo, f_hi in edges:
        assert len(decay.band_filter(f_lo, f_hi, FS)) % 2 == 1       # every band's filter can be designed at 48 kHz


def test_arguments_are_checked_before_the_library():
    for freqs in ((), tuple(range(1, 18)), (0.0, 1.0), (1.0, 24000.0), (1.0, -2.0), (1.0, math.nan), ((1.0, 2.0),), ("a",)):
        with pytest.raises(ValueError, match="freq"):
            sti.MtfBatch(freqs)
    for fs in (0, 99, 2e7, math.nan, "48000"):
        with pytest.raises(ValueError, match="fs"):
            sti.MtfBatch(fs=fs)
    with pytest.raises(ValueError, match="freq"):
        sti.MtfBatch((1.0, 60.0), fs=100)
    mb = sti.MtfBatch()
    x = np.zeros((3, 1000), np.float32)
    with pytest.raises(TypeError):
        mb.run([[0.0] * 10])
    with pytest.raises(TypeError):
        mb.run(x.astype(np.int32))
    with pytest.raises(ValueError):
        mb.run(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="samples"):
        mb.run(np.zeros((2, 0)))
    with pytest.raises(ValueError, match="samples"):
        mb.run(np.broadcast_to(np.float32(0), (sti.MAX_SAMPLES + 1,)))
    for start in ([0, 1], [0, 1, 1000], [0, -1, 2], [0.0, 1.0, 2.0]):
        with pytest.raises(ValueError, match="start"):
            mb.run(x, start=start)
    for stop in ([1, 2], [1, 2, 1001], [0, 5, 5], [1.5, 2.0, 3.0]):
        with pytest.raises(ValueError, match="stop"):
            mb.run(x, stop=stop)
    with pytest.raises(ValueError, match="stop"):
        mb.run(x, start=[5, 5, 5], stop=[6, 5, 6])
    with pytest.raises(ValueError, match="scratch_bytes"):
        mb.run(x, scratch_bytes=-1)
    m = np.full((2, 7, 14), 0.5)
    with pytest.raises(TypeError):
        sti.sti_from_mtf(m.tolist())
    with pytest.raises(TypeError):
        sti.sti_from_mtf(m.astype(np.float32))
    for bad in (np.zeros((2, 6, 14)), np.zeros((7,)), np.zeros((2, 7, 17)), np.zeros((0, 7, 14)), np.zeros((2, 2, 7, 14))):
        with pytest.raises(ValueError):
            sti.sti_from_mtf(bad)
    for kw in ({"snr_db": np.zeros(7), "level_db": np.zeros(7)}, {"snr_db": np.zeros(7), "noise_db": np.zeros(7)}, {"noise_db": np.zeros(7)},
               {"snr_db": np.zeros(6)}, {"snr_db": np.zeros((3, 7))}, {"level_db": np.zeros((2, 6))}, {"level_db": np.zeros(7), "noise_db": np.zeros(3)}):
        with pytest.raises(ValueError):
            sti.sti_from_mtf(m, **kw)
    for weights in ("child", (np.zeros(7),), (np.zeros(6), np.zeros(6)), (np.zeros(7), np.zeros(7)), (np.full(7, math.nan), np.zeros(6)), 3):
        with pytest.raises(ValueError, match="weights"):
            sti.sti_from_mtf(m, weights=weights)
    no_band = np.ones((7, 14), bool)
    no_band[2] = False
    for scheme in ("stipa2", np.ones((7, 13), bool), np.ones((7, 14)), no_band):
        with pytest.raises(ValueError):
            sti.sti_from_mtf(m, scheme=scheme)
    with pytest.raises(ValueError, match="stipa"):
        sti.sti_from_mtf(np.full((2, 7, 3), 0.5), scheme="stipa")


def test_binding_table_lists_the_entry_points():
    names = {n for n in _lib.SIGNATURES if n.startswith(("frt_mtf_", "frt_sti_"))}
    assert names == {"frt_mtf_tile", "frt_mtf_create", "frt_mtf_destroy", "frt_mtf_set_stream", "frt_mtf_run", "frt_sti_run"}
    assert _lib.load().frt_mtf_tile() == sti.TILE
