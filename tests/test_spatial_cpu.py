"""SpatialBatch without a device: the restatement of tests/spatial_helpers.py against an independent formulation (np.correlate on
the zero-extended rows), the cases of test_spatial_gpu.py proven on the reference alone, every bad setting and argument refused on
the host before the library is touched, and the plumbing of lateral_fractions and binaural_acoustics with run() and the band front
replaced by the restatement."""
import math

import numpy as np
import pytest

import spatial_helpers as sh
from friture_amd import _lib, decay, spatial


# ---- the restatement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T, M, lead, stop", [(700, 0, 0, None), (700, 1, 13, None), (1500, 48, 100, 1400), (900, 128, 5, 777)])
def test_restatement_against_np_correlate(T, M, lead, stop):
    """C_w[tau] = sum_{t in [A, B)} l[t] r[t + tau] is np.correlate of r, zero outside [0, e) and extended by M zeros on both sides,
    with the window of l, in 'valid' mode: entry k is sum_j rz[A + k + j] l[A + j]."""
    x = sh.pair(T, 7 * T + M, lead, delay=min(M, 3))
    windows = ((0, 200), (150, -1), (0, -1), (10, 10 + max(M // 2, 3)))
    ref = sh.restate(x, max_lag=M, windows=windows, stop=stop, real=np.float64)
    e = T if stop is None else stop
    l, r = x[0, :e], np.concatenate([np.zeros(M), x[1, :e], np.zeros(M)])
    t0 = ref["onset"]
    ax = np.maximum(np.abs(x[0, :e]), np.abs(x[1, :e]))
    assert ref["peak"] == int(np.argmax(ax)) and ax[t0] >= 0.1 * ax.max() and (t0 == 0 or ax[:t0].max() < 0.1 * ax.max())
    for w, (a, b) in enumerate(windows):
        A, B = min(t0 + a, e), e if b < 0 else min(t0 + b, e)
        C = np.correlate(r[A:B + 2 * M], l[A:B], "valid")
        assert C.shape == (2 * M + 1,)
        scale = math.sqrt(np.sum(l[A:B] ** 2) * np.sum(r[A:B + 2 * M] ** 2))
        assert np.max(np.abs(C - ref["C"][w])) <= 1e-12 * scale
        El, Er = np.sum(l[A:B] ** 2), np.sum(x[1, A:B] ** 2)
        assert abs(El - ref["energy"][w, 0]) <= 1e-12 * El and abs(Er - ref["energy"][w, 1]) <= 1e-12 * Er
        f = C / math.sqrt(El * Er)
        assert ref["lag_index"][w] == int(np.argmax(np.abs(f))) and abs(ref["iacc"][w] - np.max(np.abs(f))) <= 1e-12
        assert ref["tau"][w] == (ref["lag_index"][w] - M) / 48000


def test_restatement_of_dead_silent_and_empty():
    x = sh.pair(600, 3, 10)
    bad = x.copy()
    bad[1, 400] = np.nan
    assert sh.restate(bad, max_lag=4)["dead"] and not sh.restate(bad, max_lag=4, stop=400)["dead"]
    assert sh.restate(np.zeros((2, 50)), max_lag=4)["dead"]
    quiet = x.copy()
    quiet[1] = 0
    ref = sh.restate(quiet, max_lag=4, windows=((0, -1), (10000, 10001)))
    assert np.all(np.isnan(ref["iacc"])) and list(ref["lag_index"]) == [-1, -1]
    assert ref["energy"][0, 0] > 0 and ref["energy"][0, 1] == 0 and not ref["energy"][1].any()


@pytest.mark.parametrize("M", sh.SEAM_LAGS)
@pytest.mark.parametrize("f32", (False, True))
def test_seam_cases_meet_their_conditions(M, f32):
    """check_gaps passes inside the builders; here: what the windows are there to exercise does happen."""
    for T in sh.SEAM_T:
        x, refs = sh.seam_case(T, M, f32)
        assert x.shape == (65 if f32 else 3, 2, T) and x.dtype == (np.float32 if f32 else np.float64)
        assert [r["onset"] for r in refs] == [sh.seam_lead(i, T) for i in range(len(refs))]      # pair 0: a halo that reaches below sample 0
        assert all(np.isnan(r["iacc"][3]) and r["lag_index"][3] == -1 and not r["energy"][3].any() for r in refs)      # the empty one
        assert all(r["lag_index"][2] >= 0 for r in refs)                                                                # the short one is live
        if T > sh.TILE + 200:
            assert all(r["energy"][1, 0] > 0 for r in refs)


def test_second_trip_shape():
    """17 tiles per pair against tile_groups = 16 workgroups per pair in a launch of 512 pairs: the first workgroup of every pair
    takes a second tile; one pair fewer, or one tile fewer, and none would."""
    tiles = -(-sh.SECOND_TRIP_T // sh.TILE)
    assert tiles == 17 and sh.tile_groups(sh.SECOND_TRIP_PAIRS, sh.most_tiles(sh.SECOND_TRIP_T)) == 16
    assert sh.tile_groups(sh.SECOND_TRIP_PAIRS - 1, sh.most_tiles(sh.SECOND_TRIP_T)) >= 17
    assert -(-(sh.SECOND_TRIP_T - 1) // sh.TILE) == 16
    x, onset, refs = sh.second_trip_case()
    assert x.shape == (4, 2, sh.SECOND_TRIP_T) and not onset.any() and all(r["lag_index"][0] >= 0 for r in refs)


# ---- bad settings and arguments: ValueError on the host, no library call -----------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    for name in ("load", "init", "Handle"):
        monkeypatch.setattr(_lib, name, touched)


@pytest.mark.parametrize("settings", [
    dict(fs=50), dict(fs=math.nan), dict(fs="48000"), dict(max_lag=-1), dict(max_lag=129), dict(max_lag=4.0), dict(max_lag=True),
    dict(fs=192000), dict(onset_db=1.0), dict(onset_db=math.nan), dict(onset_db=None), dict(windows=()), dict(windows=((0, 1),) * 5),
    dict(windows=((0.1, 0.1),)), dict(windows=((0.2, 0.1),)), dict(windows=((-0.1, 0.1),)), dict(windows=((0, math.inf),)),
    dict(windows=((0, 0.08, 1),)), dict(windows=((None, 0.08),)), dict(windows=5), dict(windows=((0, 1e-9),))])
def test_bad_settings_raise_on_the_host(no_library, settings):
    with pytest.raises(ValueError):
        spatial.SpatialBatch(**settings)


def test_good_settings_touch_no_library(no_library):
    sb = spatial.SpatialBatch()
    assert sb.max_lag == 48 and sb.windows == ((0, 3840), (3840, -1), (0, -1))
    assert spatial.SpatialBatch(fs=44100).max_lag == 44 and spatial.SpatialBatch(fs=192000, max_lag=0).max_lag == 0
    assert spatial.SpatialBatch(windows=sh.window_seconds(sh.seam_windows(48))).windows == sh.seam_windows(48)


@pytest.mark.parametrize("kwargs", [
    dict(stop=[0, 5]), dict(stop=[5, 101]), dict(stop=[5.0, 6.0]), dict(stop=[5, 6, 7]), dict(onset=[-1, 0]), dict(onset=[0, 100]),
    dict(onset=[5, 5], stop=[6, 5]), dict(keep=("iacf",)), dict(keep="iacf"), dict(scratch_bytes=-1), dict(scratch_bytes=1.5)])
def test_bad_arguments_raise_on_the_host(no_library, kwargs):
    with pytest.raises(ValueError):
        spatial.SpatialBatch().run(np.ones((2, 2, 100)), **kwargs)


@pytest.mark.parametrize("shape", [(100,), (3, 100), (2, 3, 100), (1, 2, 2, 100), (2, 2, 0)])
def test_bad_shapes_raise_on_the_host(no_library, shape):
    with pytest.raises(ValueError):
        spatial.SpatialBatch().run(np.ones(shape))


def test_bad_kinds_raise_on_the_host(no_library):
    with pytest.raises(TypeError):
        spatial.SpatialBatch().run(np.ones((2, 100), np.int16))
    with pytest.raises(TypeError):
        spatial.SpatialBatch().run([[1.0, 2.0], [3.0, 4.0]])


# ---- composition on the restatement -----------------------------------------------------------------------------------------------

@pytest.fixture
def restated_run(monkeypatch, no_library):
    """SpatialBatch.run replaced by the float64 restatement (numpy in, numpy out); records every call's arguments."""
    calls = []

    def run(self, pairs, onset=None, stop=None, keep=("params",), scratch_bytes=1 << 28):
        x = np.asarray(pairs)
        squeeze = x.ndim == 2
        x = x[None] if squeeze else x
        calls.append(dict(shape=x.shape, onset=None if onset is None else np.array(onset), stop=stop, keep=keep, windows=self.windows,
                          max_lag=self.max_lag))
        refs = sh.restate_pairs(x, onset=onset, stop=stop, fs=self.fs, max_lag=self.max_lag, windows=self.windows,
                                onset_db=self.onset_db, real=np.float64)
        col = lambda name, kind=np.float64: np.array([r[name] for r in refs], kind)
        cut = (lambda a: a[0]) if squeeze else (lambda a: a)
        return spatial.SpatialResult(cut(col("iacc")), cut(col("tau")), cut(col("cross_abs")), cut(col("energy")), cut(col("lag_index", np.int64)),
                                     cut(col("peak", np.int64)), cut(col("onset", np.int64)), cut(col("iacf")) if "iacf" in keep else None)
    monkeypatch.setattr(spatial.SpatialBatch, "run", run)
    return calls


def test_lateral_fractions_plumbing(restated_run):
    fs = 48000
    x = np.stack([sh.pair(9000, 50 + i, 40 * i) for i in range(3)])
    res = spatial.lateral_fractions(x, ref_energy=2.0)
    assert restated_run[0]["max_lag"] == 0 and restated_run[0]["windows"] == ((0, 3840), (240, 3840), (3840, -1), (0, -1))
    for i in range(3):
        t0 = sh.restate(x[i], max_lag=0, real=np.float64)["onset"]
        l, r = x[i, 0], x[i, 1]
        omni = np.sum(l[t0:t0 + 3840] ** 2)
        assert abs(res.lf[i] - np.sum(r[t0 + 240:t0 + 3840] ** 2) / omni) <= 1e-12
        assert abs(res.lfc[i] - np.sum(np.abs(l * r)[t0 + 240:t0 + 3840]) / omni) <= 1e-12
        late = np.sum(r[t0 + 3840:] ** 2)
        assert abs(res.late_lateral[i] - late) <= 1e-12 * late and abs(res.lj[i] - 10 * math.log10(late / 2.0)) <= 1e-10
    one = spatial.lateral_fractions(x[1], fs=fs)
    assert one.lj is None and one.lf == res.lf[1] and one.lfc == res.lfc[1] and one.late_lateral == res.late_lateral[1]
    assert np.ndim(one.lf) == 0


GAINS = (1.0, 0.5, 2.0, -1.0, 0.25, 3.0)


def _fake_band_front(calls):
    """decay.band_front's two layouts with a gain per band in place of a filter: "fir" one strided view per band, otherwise one
    [rows B, T] bank with the band index fastest."""
    def band_front(ir, edges, fs, filters, order):
        calls.append(ir)
        T, B = ir.shape[-1], len(edges)
        if filters == "fir":
            for b in range(B):
                padded = np.zeros(ir.shape[:-1] + (T + 7,))
                padded[..., 3:3 + T] = GAINS[b % 6] * ir
                yield padded[..., 3:3 + T], lambda v: v
            return
        bank = np.stack([GAINS[b % 6] * ir for b in range(B)], axis=-2)
        yield bank.reshape(-1, T), lambda v: np.repeat(np.asarray(v).reshape(-1), B)
    return band_front


@pytest.mark.parametrize("filters", ("fir", "butterworth"))
@pytest.mark.parametrize("single", (False, True))
def test_binaural_acoustics_plumbing(restated_run, monkeypatch, filters, single):
    fronts = []
    monkeypatch.setattr(decay, "band_front", _fake_band_front(fronts))
    x = np.stack([sh.pair(6000, 80 + i, 25 * i, delay=i - 1) for i in range(3)])
    x = x[1] if single else x
    res = spatial.binaural_acoustics(x, filters=filters, max_lag=6, keep=("params", "iacf"))
    S = 1 if single else 3
    assert len(fronts) == 1 and fronts[0].shape == (2 * S, 6000)
    assert np.array_equal(fronts[0].reshape(2, S, 6000), np.swapaxes(x.reshape(S, 2, 6000), 0, 1))       # ear by ear
    assert len(res.centres) == 6 and [c["shape"][0] for c in restated_run] == ([S] + [S] * 6 if filters == "fir" else [S, 6 * S])
    lead = () if single else (3,)
    assert res.bands.iacc.shape == lead + (6, 3) and res.bands.energy.shape == lead + (6, 3, 2) and res.bands.iacf.shape == lead + (6, 3, 13)
    assert res.bands.onset.shape == lead + (6,) and res.broadband.iacc.shape == lead + (3,)
    for s in range(S):
        xs = x if single else x[s]
        at = (lambda v: v) if single else (lambda v: v[s])
        t0 = int(at(res.broadband.onset))
        for b in range(6):
            ref = sh.restate(GAINS[b] * xs, max_lag=6, onset=t0, real=np.float64)
            assert np.array_equal(at(res.bands.iacc)[b], ref["iacc"]) and np.array_equal(at(res.bands.energy)[b], ref["energy"])
            assert np.array_equal(at(res.bands.lag_index)[b], ref["lag_index"]) and at(res.bands.onset)[b] == t0
            assert np.array_equal(at(res.bands.iacf)[b], ref["iacf"])
        i = at(res.bands.iacc)
        assert np.array_equal(at(res.iacc_e3), (i[2, 0] + i[3, 0] + i[4, 0]) / 3)
    assert spatial.binaural_acoustics(x, bands="third", filters=filters, max_lag=6).iacc_e3 is None
    with pytest.raises(ValueError):
        spatial.binaural_acoustics(x, filters="chebyshev")
