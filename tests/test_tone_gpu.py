"""ToneBatch on the device against the longdouble restatement of tests/tone_helpers.py (the definition X9), and against itself bit
for bit where X9 promises the same bits.

The bars (tone_helpers.power_bars).  On each power P the larger of 64 times the float64 restatement's own distance from the
longdouble one for that quantity and 1e-13 sqrt(P P_total), the scale of a transform rounding error against the loudest line;
on kappa the larger of 64 times the float64 restatement's own distance and 1e-10 bins.  A quantity is kappa, P1, R, each order's
P_h and each column of the totals on its own, so a quiet order or total is never measured with a loud one's error.  peak_bin, valid, n_valid and the NaN
pattern are equal: every case asserts on its own reference that the float64 and the longdouble restatements agree on every
integer.  Every parity test prints its distances before it asserts."""
import numpy as np
import pytest

import tone_helpers as th

pytestmark = pytest.mark.gpu

FS = th.FS


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import distortion
    return distortion


def hops(N):
    return {"quarter": N // 4, "half": N // 2, "odd": 3 * N // 8 + 1, "gap": N + N // 8 + 3}


def compare(tb, res, r64, rld):
    """The parity of one result with the restatements of its recording; prints the distances and the largest ratio to a bar."""
    got = th.result_arrays(tb, res)
    assert np.array_equal(got["peak_bin"], rld["peak_bin"])
    assert np.array_equal(got["valid"], rld["valid"])
    assert np.array_equal(got["n_valid"], rld["n_valid"])
    bars = th.power_bars(r64, rld)
    worst = {}
    for name in ("kappa",) + th.POWERS + ("totals",):
        ref = np.asarray(rld[name], np.float64)
        assert np.array_equal(np.isnan(got[name]), np.isnan(ref)), name
        d = np.abs(np.asarray(got[name], th.LD) - rld[name]).astype(np.float64)
        ok = ~np.isnan(ref)
        with np.errstate(divide="ignore", invalid="ignore"):                     # an exact value meets any bar, a bar of 0 too
            ratio = np.where(d[ok] == 0, 0.0, d[ok] / np.broadcast_to(bars[name], d.shape)[ok])
        worst[name] = float(ratio.max()) if ratio.size else 0.0
    print("distances", th.distances(got, rld), "float64 restatement", th.distances(r64, rld), "largest ratio to the bar", worst)
    for name, ratio in worst.items():
        assert ratio <= 1.0, (name, ratio)


# ---- parity with the longdouble restatement -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["float64 numpy", "float32 cuda"])
@pytest.mark.parametrize("hop", ["quarter", "half", "odd", "gap"])
@pytest.mark.parametrize("N", [512, 1024, 2048, 16384])
def test_parity(mod, N, hop, kind):
    """N = 512: two frames per wavefront; 2048: the first workgroup-wide transform; 16384: the LDS limit.  5 frames (3 at 16384),
    so that a half-empty wavefront occurs."""
    import torch
    frames = 3 if N == 16384 else 5
    shape = dict(L=4, beta=9.0) if N == 512 else {}
    dtype, streams = ("float64", 1) if kind == "float64 numpy" else ("float32", 3)
    x, settings, r64, rld = th.standard_case(N, hops(N)[hop], frames, streams, dtype=dtype, **shape)
    assert rld["fund"].shape == (streams, frames)
    tb = mod.ToneBatch(**settings)
    res = tb.run(x.copy() if dtype == "float64" else torch.from_numpy(x.copy()).cuda())
    assert isinstance(res.fund, np.ndarray) == (dtype == "float64")
    compare(tb, res, r64, rld)
    # the derived figures are those of the powers
    got = th.host(res.thdn_db)
    P = np.asarray(rld["fund"], np.float64)
    want = 10 * np.log10((np.nansum(np.asarray(rld["harmonics"], np.float64), -1) + np.asarray(rld["resid"], np.float64)) / P)
    assert np.abs(got - want).max() <= 1e-6
    if N > 512:                  # Kaiser 20: the skirts lie below -190 dB; orders 2, 3, 5 at 1e-3, 1e-5, 1e-4 make the THD
        assert np.abs(th.host(res.total.thd_db) - 10 * np.log10(1e-6 + 1e-10 + 1e-8)).max() <= 0.02


def case(mod, x, **settings):
    """Run x [S, T] float64 through ToneBatch(**settings) and compare with the restatements; the result."""
    tb = mod.ToneBatch(**settings)
    args = (x, tb.fft_size, tb.hop, tb.window, tb.lobe, tb.harmonics, tb.ka, tb.kb, tb.klo, tb.khi, tb.gate)
    r64, rld = th.restate(*args, real=np.float64), th.restate(*args, real=th.LD)
    for name in ("peak_bin", "centres", "valid", "n_valid"):
        assert np.array_equal(r64[name], rld[name]), name
    res = tb.run(x)
    compare(tb, res, r64, rld)
    return tb, res, rld


N0, T0 = 1024, 1024 + 2 * 512 + 100                # the seams: 3 frames of 1024 at hop 512, Kaiser 20, L = 8


def test_fundamental_at_both_ends_of_the_search_range(mod):
    x = np.stack([th.tone(17.2, N0, T0, 1), th.tone(503.8, N0, T0, 2, amplitudes={})])
    tb, res, rld = case(mod, x, fft_size=N0)
    assert tb.klo[0] == 17 and tb.khi[0] == 504
    assert np.all(res.peak_bin[0] == 17) and np.all(res.peak_bin[1] == 504)
    assert np.isnan(res.harmonics[1]).all() and not np.isnan(res.harmonics[0]).any()


@pytest.mark.parametrize("kb, present", [(129, True), (128, False)])
def test_an_order_at_the_band_edge_is_present_and_one_bin_later_absent(mod, kb, present):
    """kappa = 40.3: c_3 = 121, and c_3 + L = 129 = kb is present; with kb = 128 it is absent: NaN and not in the sums."""
    x = th.tone(40.3, N0, T0, 3)[None]
    tb, res, rld = case(mod, x, fft_size=N0, harmonics=4, band=(0.0, (kb + 0.5) * FS / N0))
    assert tb.kb == kb and np.all(rld["centres"][0, :, 1] == 81)
    assert np.all((rld["centres"][0, :, 2] == 121) == present)
    assert np.all(np.isnan(res.harmonics[0, :, 1]) != present) and np.isnan(res.harmonics[0, :, 2]).all()
    totals = tb.state_parts(res.state)["totals"]
    assert (totals[0, 4] > 0) == present and totals[0, 5] == 0.0


def test_overlapping_lobes_count_each_bin_once(mod):
    """kappa = 16.6, just below c1 = 2 L + 1 = 17: c_2 = 33 and its lobe starts at 26, not at 25.  The second harmonic is quiet
    (P_2 = 5e-15, its bar 5e-21), so that the fundamental's skirt in bin 25 (above 1e-20) would show in P_2."""
    x = th.tone(16.6, N0, T0, 4, amplitudes={2: 1e-7})[None]
    tb, res, rld = case(mod, x, fft_size=N0, harmonics=3)
    assert np.all(rld["centres"][0, :, :2] == [17, 33])
    Q = th.spectrum(x[0, :N0], tb.window, th.LD)
    assert th.lobes(Q, 17, 8, 3, tb.kb)[3][:2] == [(9, 25), (26, 41)] and Q[25] > 1e-20


def test_band_cuts_the_residual(mod):
    x = (th.tone(60.3, N0, T0, 5) + 1e-3 * np.sin(2 * np.pi * 400.25 / N0 * np.arange(T0)))[None]
    _, cut, _ = case(mod, x, fft_size=N0, harmonics=5, band=(1000.0, 16000.0))
    _, full, _ = case(mod, x, fft_size=N0, harmonics=5)
    assert np.all(cut.resid < 1e-3 * full.resid) and np.all(full.resid > 4e-7)


def test_f0_steers_the_search_to_the_quieter_tone(mod):
    t = np.arange(T0)
    x = np.stack([np.sin(2 * np.pi * 50.3 / N0 * t) + 0.1 * np.sin(2 * np.pi * 131.7 / N0 * t + 1.0)] * 2)
    f0 = [131.7 * FS / N0, 50.3 * FS / N0]
    tb, res, _ = case(mod, x, fft_size=N0, harmonics=2, f0=f0)
    assert np.all(res.peak_bin[0] == 132) and np.all(res.peak_bin[1] == 50)
    assert np.abs(res.freq[0] - f0[0]).max() < 0.01 and np.abs(res.fund[0] - 0.005).max() < 1e-6


@pytest.mark.parametrize("H", [2, 32])
def test_the_lowest_and_the_highest_order_count(mod, H):
    x = np.stack([th.tone(13.27 + 2 * 8 + 3, N0, T0, 6), th.tone(18.27, N0, T0, 7)])
    tb, res, rld = case(mod, x, fft_size=N0, harmonics=H)
    assert res.harmonics.shape == (2, 3, H - 1)
    if H == 32:
        assert (rld["centres"][1, 0] >= 0).sum() >= 27 and (rld["centres"][0, 0] >= 0).sum() < 20


def test_an_array_window_with_an_explicit_lobe(mod):
    w = np.blackman(N0) * (1 + 0.01 * np.cos(np.arange(N0)))
    x = th.tone(44.31, N0, T0, 8)[None]
    case(mod, x, fft_size=N0, window=w, lobe=4, harmonics=6)


# ---- dead and gated frames ------------------------------------------------------------------------------------------------------

def dead_recording(N):
    """9 frames at hop N: live, silent, live, NaN, live, Inf, quiet, quiet, live."""
    x = th.tone(31.3, N, 9 * N, 9).reshape(9, N).copy()
    x[1] = 0.0
    x[3, 100] = np.nan
    x[5, N - 1] = -np.inf
    x[6:8] *= 1e-4
    return x.reshape(-1)


def test_dead_and_gated_frames(mod):
    N = 1024
    x = dead_recording(N)
    tb = mod.ToneBatch(fft_size=N, hop=N, gate_db=-40.0)
    res = tb.run(x)
    dead, gated = [1, 3, 5], [6, 7]
    assert res.peak_bin[dead].tolist() == [-1, -1, -1] and np.all(np.delete(res.peak_bin, dead) == 31)
    assert res.valid.tolist() == [True, False, True, False, True, False, False, False, True]
    for a in (res.freq, res.fund, res.resid):
        assert np.isnan(a[dead]).all() and not np.isnan(np.delete(a, dead)).any()
    assert np.isnan(res.harmonics[dead]).all() and not np.isnan(res.harmonics[gated]).any()
    assert np.abs(res.fund[gated] - 0.5e-8).max() < 1e-12 and np.isnan(res.thd_db[dead]).all()
    assert res.total.n_valid == 4
    live = res.valid
    totals = tb.state_parts(res.state)["totals"][0]
    assert totals[1] == th.fold(res.fund[live], np.float64) and totals[2] == th.fold(res.resid[live], np.float64)
    assert totals[3] == th.fold(res.harmonics[live, 0], np.float64) and totals[-1] == 4.0
    # the same recording with other samples in the dead frames
    y = x.reshape(9, N).copy()
    y[1] = -0.0
    y[3] = np.where(np.arange(N) % 3 == 0, np.nan, 1e300)
    y[5] = np.inf
    other = tb.run(y.reshape(-1))
    assert th.same_bits(res, other) == []
    # and against the restatement, gate included
    case(mod, x[None], fft_size=N, hop=N, gate_db=-40.0)


def test_an_all_dead_stream_has_no_valid_frame(mod):
    tb = mod.ToneBatch(fft_size=512, window=("kaiser", 9.0), lobe=4)
    res = tb.run(np.zeros((2, 2048), np.float32))
    assert res.total.n_valid.tolist() == [0, 0] and np.isnan(res.total.fund).all() and not res.valid.any()
    assert np.all(res.peak_bin == -1) and np.isnan(res.fund).all()


# ---- what must not matter -------------------------------------------------------------------------------------------------------

SHORT = dict(fft_size=512, hop=3 * 512 // 8 + 1, window=("kaiser", 9.0), lobe=4, harmonics=6)


def short_recording(streams=1, frames=3, extra=57):
    T = 512 + (frames - 1) * SHORT["hop"] + extra
    return np.stack([th.tone(21.37 + 5 * s, 512, T, 20 + s) for s in range(streams)])


def in_pieces(tb, x, cuts):
    """The results of x [S, T] run in the pieces between `cuts`, joined; the last state."""
    state, parts = None, []
    for a, b in zip([0] + list(cuts), list(cuts) + [x.shape[-1]]):
        r = tb.run(x[..., a:b], state=state)
        state = r.state
        parts.append(r)
    return parts


def joined_same(whole, parts):
    bad = []
    for name in ("freq", "fund", "resid", "harmonics", "peak_bin", "valid"):
        joined = np.concatenate([th.host(getattr(p, name)) for p in parts], axis=1)
        if joined.tobytes() != th.host(getattr(whole, name)).tobytes():
            bad.append(name)
    last = parts[-1]
    if th.host(last.state.data).tobytes() != th.host(whole.state.data).tobytes() or tuple(last.state[1:4]) != tuple(whole.state[1:4]):
        bad.append("state")
    for name in ("n_valid", "fund", "resid", "harmonics", "freq"):
        if th.host(getattr(last.total, name)).tobytes() != th.host(getattr(whole.total, name)).tobytes():
            bad.append("total." + name)
    return bad


def test_a_cut_at_any_sample_gives_the_bits_of_one_call(mod):
    x = short_recording(streams=2)
    tb = mod.ToneBatch(**SHORT)
    whole = tb.run(x)
    assert whole.fund.shape == (2, 3) and whole.valid.all()
    for cut in range(1, x.shape[1]):
        assert joined_same(whole, in_pieces(tb, x, [cut])) == [], cut
    assert joined_same(whole, in_pieces(tb, x, range(1, x.shape[1]))) == []          # one-sample pieces
    assert joined_same(whole, in_pieces(tb, x, [0, 5, 5, 700])) == []                # empty pieces


def test_a_cut_at_any_sample_with_a_hop_above_the_frame(mod):
    settings = dict(SHORT, hop=512 + 512 // 8 + 3)
    tb = mod.ToneBatch(**settings)
    x = short_recording(frames=1, extra=2 * settings["hop"] + 9)
    whole = tb.run(x)
    assert whole.fund.shape == (1, 3)
    for cut in range(1, x.shape[1], 7):
        assert joined_same(whole, in_pieces(tb, x, [cut])) == [], cut
    assert joined_same(whole, in_pieces(tb, x, range(13, x.shape[1], 13))) == []


def test_fewer_samples_than_a_frame_give_no_frame_and_a_state(mod):
    tb = mod.ToneBatch(**SHORT)
    x = short_recording()[:, :300]
    res = tb.run(x)
    assert res.fund.shape == (1, 0) and res.harmonics.shape == (1, 0, 5) and res.state.n_in == 300 and res.state.pending == 300
    assert np.array_equal(tb.state_parts(res.state)["row"], x) and res.total.n_valid.tolist() == [0]


@pytest.mark.parametrize("N", [512, 2048])
def test_slabs_shapes_strides_batches_kinds_and_dtypes_do_not_matter(mod, N):
    import torch
    settings = SHORT if N == 512 else dict(fft_size=N, hop=N // 4)
    tb = mod.ToneBatch(**settings)
    T = N + 6 * tb.hop + 11
    x = np.stack([th.tone(30.3 + 4 * s, N, T, 40 + s) for s in range(3)]).astype(np.float32)
    whole = tb.run(x)
    assert whole.fund.shape == (3, 7)
    assert th.same_bits(whole, tb.run(x, scratch_bytes=0)) == []                     # one frame group per launch
    assert th.same_bits(whole, tb.run(x, scratch_bytes=3 * 3 * (3 + tb.harmonics) * 8)) == []
    assert th.same_bits(whole, tb.run(x.astype(np.float64))) == []
    dev = tb.run(torch.from_numpy(x).cuda())
    assert dev.fund.is_cuda and dev.peak_bin.dtype == torch.int32 and dev.valid.dtype == torch.bool
    assert th.same_bits(whole, dev) == []
    assert th.same_bits(whole, tb.run(torch.from_numpy(x).cuda().double(), scratch_bytes=0)) == []
    wide = np.zeros((3, 2, T + 5), np.float32)
    wide[:, 1, 3:3 + T] = x
    assert th.same_bits(whole, tb.run(wide[:, 1, 3:3 + T])) == []                    # strided views against copies
    assert th.same_bits(whole, tb.run(torch.from_numpy(wide).cuda()[:, 1, 3:3 + T])) == []
    for s in range(3):                                                               # a stream alone; [T] against [1, T]
        alone, flat = tb.run(x[s:s + 1]), tb.run(x[s])
        assert flat.fund.shape == (7,) and flat.harmonics.shape == (7, tb.harmonics - 1) and flat.total.fund.shape == ()
        for name in ("freq", "fund", "resid", "harmonics", "peak_bin", "valid"):
            a = getattr(alone, name)
            assert a[0].tobytes() == getattr(flat, name).tobytes() == getattr(whole, name)[s].tobytes(), name
        assert alone.state.data.tobytes() == flat.state.data.tobytes()
        assert np.array_equal(tb.state_parts(alone.state)["totals"][0], tb.state_parts(whole.state)["totals"][s])
        assert np.array_equal(tb.state_parts(alone.state)["row"][0], tb.state_parts(whole.state)["row"][s])


def test_one_shot_helper(mod):
    x = short_recording(streams=2)
    total = mod.tone_distortion(x, **SHORT)
    want = mod.ToneBatch(**SHORT).run(x).total
    assert total.n_valid.tolist() == [3, 3] and total.thdn_db.tobytes() == want.thdn_db.tobytes()
    assert np.all(np.abs(total.level_db) < 0.01) and np.all(np.abs(total.freq - np.array([21.37, 26.37]) * FS / 512) < 0.5)
