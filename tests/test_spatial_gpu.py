"""SpatialBatch on the device against the longdouble restatement of tests/spatial_helpers.py (the sequential definition of X8), and
against itself bit for bit where X8 promises the same bits.

The bars, for windows of at most 2^17 samples.  A float64 sum of n terms in any order, fused or not, is within n 2^-53 sum |terms|
of exact: n <= 2^17 gives 2^-36 = 1.5e-11 of sum |terms|.  For El, Er and X the terms are not negative, so that is 1.5e-11 relative:
the bar is 1e-10.  For C_w[tau], Cauchy-Schwarz bounds sum |l[t] r[t + tau]| by sqrt(El_w Er'_w), Er'_w the energy of r over [A_w -
M, B_w + M): |C - ref| <= 1e-10 sqrt(El_w Er'_w).  IACF = C / sqrt(El Er): with Er' / Er <= 4 (asserted on the reference) the error of C
is at most 2e-10, the two energies add 1e-10 relative to a value of at most 2, the division and the root a few 2^-53: the bar on iacf
and iacc is 1e-9 absolute.  lag_index, peak and onset are equal (the reference keeps its index decisions 1e-6 from their edges).
Every parity test prints its distances before it asserts."""
import numpy as np
import pytest

import spatial_helpers as sh

pytestmark = pytest.mark.gpu

TL = sh.TILE
IACF = dict(keep=("params", "iacf"))


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import spatial
    assert spatial.TILE == TL and hip.frt_spatial_tile() == TL
    return spatial


def host(res):
    """A result tuple with numpy fields."""
    return type(res)(*[v.cpu().numpy() if hasattr(v, "cpu") else v for v in res])


def same_bits(a, b):
    a, b = host(a), host(b)
    for f, u, v in zip(a._fields, a, b):
        assert (u is None) == (v is None), f
        if u is not None:
            u, v = np.asarray(u), np.asarray(v)
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), f


def pick(res, rows):
    res = host(res)
    return type(res)(*[None if v is None else v[rows] for v in res])


def batch_for(mod, M, windows=None, **settings):
    if windows is not None:
        settings["windows"] = sh.window_seconds(windows)
    return mod.SpatialBatch(max_lag=M, **settings)


# ---- parity on the seams -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f32", (False, True), ids=("3xf64", "65xf32"))
@pytest.mark.parametrize("M", sh.SEAM_LAGS)
@pytest.mark.parametrize("T", sh.SEAM_T)
def test_parity_on_the_seams(mod, T, M, f32):
    """Windows that start at sample 0 (the halo reaches below it), end at e (the halo reaches past it), are shorter than M, are
    empty, and overlap; lead-ins 0, TL - 1, TL in turn (cut to T - 1200 where they do not fit)."""
    x, refs = sh.seam_case(T, M, f32)
    res = host(batch_for(mod, M, sh.seam_windows(M)).run(x, **IACF))
    sh.compare(res, refs, f"T {T}, M {M}, {len(x)} {'float32' if f32 else 'float64'} pairs")


# ---- stop ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", (0, 48))
def test_samples_behind_stop_are_never_read_into_a_result(mod, M):
    T = 2 * TL + 3
    e = np.array([T - 700, TL + 9, T - 1], np.int64)
    base = np.stack([sh.pair(T, 4100 + i, 17 * i, delay=i - 1) for i in range(3)])
    sb = batch_for(mod, M, ((0, 900), (400, -1), (0, -1)))
    runs = []
    for fill in (np.nan, 0.0, 1e300):
        x = base.copy()
        for i in range(3):
            x[i, :, e[i]:] = fill
        runs.append(sb.run(x, stop=e, **IACF))
    same_bits(runs[0], runs[1])
    same_bits(runs[0], runs[2])
    for i in range(3):
        same_bits(pick(runs[0], i), sb.run(base[i, :, :e[i]], **IACF))
    refs = sh.restate_pairs(base, stop=e, max_lag=M, windows=((0, 900), (400, -1), (0, -1)))
    sh.check_gaps(refs)
    sh.compare(host(runs[0]), refs, f"stop, M {M}")


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", (1, 48, 128))
def test_a_delayed_copy_has_iacc_one_at_its_delay(mod, M):
    T, margin = TL + 700, 200
    l = np.zeros(T)
    l[margin:T - margin] = np.random.default_rng(M).standard_normal(T - 2 * margin)
    pairs = np.stack([np.stack([l, np.roll(l, d)]) for d in (-M, 0, M)] + [np.stack([l, -l])])
    res = host(batch_for(mod, M, ((0, -1),)).run(pairs, onset=np.zeros(4, np.int64)))
    print(f"M {M}: |iacc - 1| = {np.max(np.abs(res.iacc - 1)):.3g} (bar {sh.IACF_BAR:g}), lag_index {res.lag_index[:, 0]}")
    assert np.array_equal(res.lag_index[:, 0], [0, M, 2 * M, M]) and np.array_equal(res.tau[:, 0], np.array([-M, 0, M, 0]) / 48000)
    assert np.max(np.abs(res.iacc - 1)) <= sh.IACF_BAR


def test_a_silent_row_gives_nan_and_keeps_the_energy(mod):
    x = sh.pair(TL + 50, 77, 30)
    x[1] = 0
    res = host(batch_for(mod, 48).run(x, **IACF))
    ref = sh.restate(x)
    assert np.all(np.isnan(res.iacc)) and np.all(np.isnan(res.tau)) and np.all(np.isnan(res.iacf)) and np.all(res.lag_index == -1)
    assert res.peak == ref["peak"] and res.onset == ref["onset"] and not res.energy[:, 1].any() and not res.cross_abs.any()
    d = sh.rel_distance(res.energy[:, 0], ref["energy"][:, 0])
    print(f"a silent row: El {d:.3g} relative (bar {sh.ENERGY_BAR:g})")
    assert d <= sh.ENERGY_BAR


# ---- the same bits ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def five():
    """Five float32 pairs of 2 TL + 3 samples with different lead-ins and delays."""
    x = np.stack([sh.pair(2 * TL + 3, 900 + i, (0, TL - 1, TL, 3, 500)[i], delay=i - 2, dtype=np.float32) for i in range(5)])
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("M", (0, 48))
def test_bits_do_not_depend_on_neighbours_slabs_strides_dtype_or_kind(mod, five, M):
    import torch
    sb = batch_for(mod, M)
    whole = sb.run(five, **IACF)
    for i in range(5):
        same_bits(pick(whole, slice(i, i + 1)), sb.run(five[i:i + 1], **IACF))                    # alone
        same_bits(pick(whole, i), sb.run(five[i], **IACF))                                        # [2, T] against [1, 2, T]
    same_bits(whole, sb.run(five, scratch_bytes=1, **IACF))                                       # one pair per launch
    same_bits(whole, sb.run(five, scratch_bytes=40000, **IACF))                                   # M = 48: two pairs per launch
    same_bits(whole, sb.run(five.astype(np.float64), **IACF))                                     # float32 against float64
    wide = np.zeros((5, 3, 2, 2 * TL + 3 + 11), np.float32)
    wide[:, 1, :, 4:4 + 2 * TL + 3] = five
    view = wide[:, 1, :, 4:4 + 2 * TL + 3]
    assert view.strides[0] != 2 * view.strides[1] and view.strides[1] != view.strides[2] * view.shape[2]
    same_bits(whole, sb.run(view, **IACF))                                                        # pair stride and row stride
    dev = torch.from_numpy(np.array(five)).cuda()
    on_device = sb.run(dev, **IACF)
    assert on_device.iacc.is_cuda and on_device.lag_index.is_cuda and on_device.iacf.is_cuda
    same_bits(whole, on_device)                                                                   # numpy against CUDA
    dview = torch.from_numpy(wide).cuda()[:, 1, :, 4:4 + 2 * TL + 3]
    same_bits(whole, sb.run(dview, **IACF))
    ears_first = torch.from_numpy(np.ascontiguousarray(np.swapaxes(five, 0, 1))).cuda().transpose(0, 1)         # row stride above pair stride
    assert ears_first.stride(1) > ears_first.stride(0)
    same_bits(whole, sb.run(ears_first, **IACF))


def test_dead_pairs_between_live_ones(mod, five):
    x = np.zeros((8,) + five.shape[1:], np.float32)
    x[[0, 2, 4, 6, 7]] = five
    x[3] = five[0]
    x[3, 0, TL + 1] = np.nan                                         # a NaN in l
    x[5] = five[1]
    x[5, 1, 2 * TL + 2] = np.inf                                     # an Inf in r, on the last sample
    sb = batch_for(mod, 48)
    res = host(sb.run(x, **IACF))
    for i in (1, 3, 5):
        for name, v in zip(res._fields, res):
            assert np.all(v[i] == -1) if v.dtype == np.int64 else np.all(np.isnan(v[i])), (i, name)
    same_bits(pick(res, [0, 2, 4, 6, 7]), sb.run(five, **IACF))


def test_given_onsets_equal_to_the_found_ones(mod, five):
    import torch
    sb = batch_for(mod, 48)
    found = sb.run(five, **IACF)
    same_bits(found, sb.run(five, onset=found.onset, **IACF))
    dev = torch.from_numpy(np.array(five)).cuda()
    same_bits(found, sb.run(dev, onset=torch.from_numpy(found.onset).cuda(), **IACF))


# ---- composition -----------------------------------------------------------------------------------------------------------------------

def test_lateral_fractions_against_the_window_sums(mod):
    x = np.stack([sh.pair(3 * TL + 100, 600 + i, 40 * i, delay=0, rt=0.25) for i in range(3)])
    res = mod.lateral_fractions(x, ref_energy=3.0)
    refs = sh.restate_pairs(x, max_lag=0, windows=((0, 3840), (240, 3840), (3840, -1), (0, -1)))
    sh.check_gaps(refs)
    lf = np.array([r["energy"][1, 1] / r["energy"][0, 0] for r in refs])
    lfc = np.array([r["cross_abs"][1] / r["energy"][0, 0] for r in refs])
    late = np.array([r["energy"][2, 1] for r in refs])
    d = [sh.rel_distance(res.lf, lf), sh.rel_distance(res.lfc, lfc), sh.rel_distance(res.late_lateral, late),
         sh.abs_distance(res.lj, 10 * np.log10(late / 3.0))]
    print(f"lateral_fractions: lf {d[0]:.3g}, lfc {d[1]:.3g}, late {d[2]:.3g} relative (bar {3 * sh.ENERGY_BAR:g}), lj {d[3]:.3g} dB")
    assert max(d[:3]) <= 3 * sh.ENERGY_BAR and d[3] <= 1e-9          # a ratio of two sums within 1e-10 each; 10 log10: 4.3 dB per unit
    import torch
    dev = mod.lateral_fractions(torch.from_numpy(x).cuda(), ref_energy=3.0)
    assert dev.lf.is_cuda and dev.lj.is_cuda
    same_bits(res._replace(lj=None), dev._replace(lj=None))          # the ratios divide the same bits; log10 is numpy's here, torch's there
    assert sh.abs_distance(dev.lj.cpu().numpy(), res.lj) <= 1e-12
    one = mod.lateral_fractions(x[2])
    assert one.lj is None and one.lf == res.lf[2] and one.lfc == res.lfc[2]


def test_binaural_acoustics_butterworth_against_the_calls_by_hand(mod):
    from friture_amd import decay, sosfilter
    T = 1 << 13
    x = np.stack([sh.pair(T, 300 + i, 100 * i, delay=2 - 4 * i, rt=0.3) for i in range(2)])
    res = mod.binaural_acoustics(x, filters="butterworth", **IACF)
    centres, edges = decay.band_edges("octave")
    sb = mod.SpatialBatch()
    broadband = sb.run(x, **IACF)
    same_bits(res.broadband, broadband)
    sos = np.stack([sosfilter.butter_band_sos(lo, hi, 48000, 3) for lo, hi in edges])
    ears = np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape(4, T)
    y = sosfilter.SosBatch(sos).run(ears, fan=True, dtype="float64").y                          # [4, 6, T]
    assert y.shape == (4, 6, T)
    for s in range(2):
        for b in range(6):
            by_hand = sb.run(np.stack([y[s, b], y[2 + s, b]]), onset=broadband.onset[s:s + 1], **IACF)
            same_bits(type(by_hand)(*[v[s, b] for v in res.bands]), by_hand)
    i = res.bands.iacc
    assert np.array_equal(res.iacc_e3, (i[:, 2, 0] + i[:, 3, 0] + i[:, 4, 0]) / 3) and np.array_equal(res.centres, centres)
    assert res.bands.iacf.shape == (2, 6, 3, 97) and np.all(res.bands.iacc[:, 2:5, 0] > 0) and np.all(res.bands.iacc <= 1 + 1e-12)


def test_binaural_acoustics_fir_reads_the_band_rows_in_place(mod):
    from friture_amd import convolve, decay
    T = 1 << 13
    x = np.stack([sh.pair(T, 350 + i, 100 * i, delay=3 * i - 2, rt=0.3) for i in range(3)])
    bands = ((1000.0, 2000.0), (2000.0, 4000.0))
    res = mod.binaural_acoustics(x, bands=bands, max_lag=20, **IACF)
    assert res.iacc_e3 is None and res.bands.iacc.shape == (3, 2, 3)
    sb = mod.SpatialBatch(max_lag=20)
    for b, (lo, hi) in enumerate(bands):
        h = decay.band_filter(lo, hi)
        m = (len(h) - 1) // 2
        y = convolve.ConvolveBatch(h).run(x.reshape(6, T)).y[:, m:m + T].reshape(3, 2, T)
        same_bits(type(res.bands)(*[v[:, b] for v in res.bands]), sb.run(np.ascontiguousarray(y), onset=res.broadband.onset, **IACF))
    one = mod.binaural_acoustics(x[1], bands=bands, max_lag=20, **IACF)
    same_bits(one.bands, type(res.bands)(*[v[1] for v in res.bands]))


# ---- the tile loop's second trip ---------------------------------------------------------------------------------------------------------

def test_a_workgroup_takes_a_second_tile(mod):
    """512 pairs in one launch: tile_groups = max(16, ceil(8192 / 512)) = 16 workgroups per pair for 17 tiles, so every pair's first
    workgroup comes round again (tests/test_spatial_cpu.py checks the arithmetic).  Pair i is probe i % 4; with 511 pairs, and
    with one pair per launch, every tile has a workgroup of its own: the same bits."""
    import torch
    x, onset, refs = sh.second_trip_case()
    sb = batch_for(mod, sh.SECOND_TRIP_LAG, ((0, -1),))
    probes = host(sb.run(x, onset=onset, **IACF))
    sh.compare(probes, refs, "4 probes of 17 tiles")
    batch = torch.from_numpy(np.array(x)).cuda().repeat(sh.SECOND_TRIP_PAIRS // 4, 1, 1)
    res = host(sb.run(batch, onset=torch.zeros(sh.SECOND_TRIP_PAIRS, dtype=torch.int64, device="cuda"), **IACF))
    same_bits(res, type(probes)(*[np.concatenate([v] * (sh.SECOND_TRIP_PAIRS // 4)) for v in probes]))
    fewer = host(sb.run(batch[:sh.SECOND_TRIP_PAIRS - 1], onset=torch.zeros(sh.SECOND_TRIP_PAIRS - 1, dtype=torch.int64, device="cuda"), **IACF))
    same_bits(fewer, pick(res, slice(0, sh.SECOND_TRIP_PAIRS - 1)))
