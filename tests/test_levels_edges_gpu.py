"""levels.hip at the operating points test_levels_gpu.py leaves out: every Ndec 1 .. 13 with rows cut at the tile seams, the
Subsampler with several channels and padded rows, the meters at other chunk sizes (one sample .. longer than the smoothing
kernel), NaN and Inf chunks, a history ring that wraps, a change of Ndec with samples carried, a change of channel count, and the
refusals.  Every comparison is against tests/levels_helpers.py (MetersCPU, LongLevelsRef, SubsamplerCPU), which
test_levels_edges_cpu.py holds to the reference's recorded values.  Long-level values are compared bit for bit, dB values to
1e-12 (the device's log10 against numpy's)."""
import ctypes
import math

import numpy as np
import pytest

import levels_helpers as L
from oracle import levels as H

pytestmark = pytest.mark.gpu
_DP = ctypes.POINTER(ctypes.c_double)
FIELDS = 6
SENTINEL = -12345.678


def _addr(a, offset=0):
    """The address of element `offset` of a float64 numpy array or CUDA tensor."""
    base = a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
    return base + 8 * offset


def _levels_run(h, addr, n, ld, chunk=512, meters=False, long=True, dtype=1):
    """frt_levels_run on n samples per channel at `addr` (host or device, None for none) with row stride ld."""
    from friture_amd import _lib
    nb = h.blocks_for(n) if long else 0
    m = np.full((h.channels, -(-n // chunk), FIELDS), np.nan) if meters else None
    lo = np.full((h.channels, nb, 2), np.nan) if long else None
    got = ctypes.c_int64(-1)
    _lib.check(h.lib.frt_levels_run(h.h, addr, dtype, n, ld, chunk, None if m is None else m.ctypes.data,
                                    None if lo is None else lo.ctypes.data, ctypes.byref(got)))
    assert got.value == nb
    return m, lo


def _last_error(lib):
    return lib.frt_last_error().decode(errors="replace")


def _check_long(got, want, what=""):
    """got [nb, 2] of the GPU against the reference's: the level bit for bit, the dB to 1e-12."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[:, 0], want[:, 0], equal_nan=True), what
    assert L.db_close(got[:, 1], want[:, 1]), what


# ---- 1. long levels, every Ndec ---------------------------------------------------------------------------------------------------

def _pieces_random(n, B, rng):
    sizes, pos = [0, B - 1], B - 1                                   # an empty call, then one that completes no block
    while pos < n:
        k = min(int(rng.integers(0, 3 * B + 7)), n - pos)
        sizes.append(k)
        pos += k
    return sizes


@pytest.mark.parametrize("ndec", range(1, 14))
def test_long_levels_every_ndec(ndec):
    """Two full tiles of the last decimation kernel and a third of two blocks, whole (host rows with a padded stride), in random
    pieces (device rows read in place with that stride) and one block per call; then with a third tile of one block."""
    import torch
    from friture_amd.levels import _Handle
    B, hist = 1 << ndec, 5
    lens = L.seam_lengths(ndec)
    n = lens["levels"]
    rng = np.random.default_rng(100 + ndec)
    x = np.full((2, n + 3), np.nan)                                   # the padding is never read
    x[0, :n] = 0.1 * rng.standard_normal(n)
    x[1, :n] = H.sine(n, 440., 0.3) * (0.25 + rng.random(n))
    want = [L.LongLevelsRef(ndec).push(x[c, :n]) for c in range(2)]
    assert want[0].shape == (n >> ndec, 2)

    whole = _Handle(2, ndec, hist)
    _, lo = _levels_run(whole, _addr(x), n, n + 3)
    for c in range(2):
        _check_long(lo[c], want[c], f"whole, channel {c}")
    assert np.array_equal(whole.history(hist), lo[:, -hist:, 1])

    xd = torch.from_numpy(x).cuda()
    rand = _Handle(2, ndec, hist)
    outs, pos, empty = [], 0, 0
    for k in _pieces_random(n, B, rng):
        _, lo = _levels_run(rand, _addr(xd, pos) if k else None, k, n + 3)
        empty += lo.shape[1] == 0
        outs.append(lo)
        pos += k
    assert pos == n and empty >= 2
    lo = np.concatenate(outs, axis=1)
    for c in range(2):
        _check_long(lo[c], want[c], f"random pieces, channel {c}")
    assert np.array_equal(rand.history(hist), lo[:, -hist:, 1])

    one = _Handle(2, ndec, hist)
    first = max(1, B // 2)                                           # completes no block; then every call completes one
    outs = [_levels_run(one, _addr(x), first, n + 3)[1], _levels_run(one, None, 0, 0)[1]]
    assert outs[0].shape[1] == 0 and outs[1].shape[1] == 0
    pos = first
    while pos < n:
        k = min(B, n - pos)
        outs.append(_levels_run(one, _addr(x, pos), k, n + 3)[1])
        assert outs[-1].shape[1] == (1 if k == B else (first + k) // B)
        pos += k
    lo = np.concatenate(outs, axis=1)
    for c in range(2):
        _check_long(lo[c], want[c], f"one block per call, channel {c}")
    state = whole.get_state()
    assert np.array_equal(rand.get_state(), state) and np.array_equal(one.get_state(), state)

    short = _Handle(2, ndec, hist)                                   # the third tile holds one block
    _, lo = _levels_run(short, _addr(x), lens["levels_one"], n + 3)
    for c in range(2):
        _check_long(lo[c], want[c][:-1], f"one block less, channel {c}")


# ---- 2. Subsampler seams ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ndec", [1, 4, 5, 6, 8, 13])
def test_subsampler_seams(ndec):
    """Three channels, rows padded by 5 (NaN in the input's padding, a sentinel behind the output), from host memory and on
    device pointers; after each length pushes of 1, 9, 10 and 11 samples read the carried state back."""
    import torch
    from friture_amd import _lib
    from friture_amd.levels import _Handle
    C, pad = 3, 5
    lens = L.seam_lengths(ndec)
    rng = np.random.default_rng(200 + ndec)
    for kind in ("odd", "even", "short", "ragged"):
        pushes = [lens[kind], 1, 9, 10, 11]
        xs = [np.stack([(s * rng.standard_normal(k)) ** 2 for s in (0.2, 1.0, 3e-4)]) for k in pushes]
        subs = [H.SubsamplerCPU(ndec) for _ in range(C)]
        want = [np.stack([subs[c].push(x[c]) for c in range(C)]) for x in xs]
        for device in (False, True):
            h = _Handle(C, ndec, 1)
            for x, w in zip(xs, want):
                k = x.shape[1]
                m = int(h.lib.frt_levels_subsample_length(h.h, k))
                assert m == w.shape[1], (kind, k)
                xp = np.full((C, k + pad), np.nan)
                xp[:, :k] = x
                out = np.full(C * m + 7, SENTINEL)
                if device:
                    xp, out = torch.from_numpy(xp).cuda(), torch.from_numpy(out).cuda()
                got = ctypes.c_int64(-1)
                _lib.check(h.lib.frt_levels_subsample(h.h, _addr(xp), 1, k, k + pad, _addr(out), ctypes.byref(got)))
                if device:
                    out = out.cpu().numpy()
                assert got.value == m
                assert np.array_equal(out[:C * m].reshape(C, m), w), (kind, k, device)
                assert np.all(out[C * m:] == SENTINEL), (kind, k, device)


# ---- 3. meters at other chunk sizes ----------------------------------------------------------------------------------------------

def _meter_rows(T, seed):
    """[3, T]: noise, a 1 kHz burst in silence (from 2/5 to 3/5 of the row, across chunk boundaries), silence."""
    rng = np.random.default_rng(seed)
    x = np.zeros((3, T))
    x[0] = 0.1 * rng.standard_normal(T)
    a, b = (2 * T) // 5, (3 * T) // 5 + 1
    x[1, a:b] = H.sine(b - a, 1000., 0.5, a)
    return x


def _check_meters(lb, x, m, chunk, prev_rms=None):
    """m [C, nchunks, 6] of the GPU for the rows x cut into `chunk`-sample chunks, against a fresh MetersCPU per channel.
    Returns the largest |got_k - rms_step(got_{k-1}, y_k)| over its bound."""
    sizes = L.chunk_sizes(x.shape[1], chunk)
    worst = 0.0
    for c in range(x.shape[0]):
        cpu = L.MetersCPU(lb.alpha, lb.kernel, lb.alpha2)
        want = cpu.run(x[c], sizes)
        got = m[c]
        assert got.shape == want.shape
        assert np.array_equal(got[:, 1], want[:, 1]), (chunk, c)                          # old_max
        assert np.array_equal(got[:, 5], want[:, 5]), (chunk, c)                          # branch
        peak, branch = L.ballistic_replay(got[:, 2], got[:, 3])
        assert np.array_equal(got[:, 4], peak) and np.array_equal(got[:, 5], branch), (chunk, c)
        assert L.db_close(got[:, 3], want[:, 3]) and L.db_close(got[:, 2], want[:, 2]), (chunk, c)
        prev, pos = 1e-30, 0
        for k, size in enumerate(sizes):
            ref = cpu.rms_step(prev, x[c, pos:pos + size])
            bound = (math.ceil(min(size, lb.kernel.shape[0]) / 64) + 12) * 2.0 ** -53 * ref
            err = abs(np.longdouble(got[k, 0]) - ref) if L.EXTENDED else abs(got[k, 0] - ref)
            assert err <= bound, (chunk, c, k, float(err), float(bound))
            if bound > 0:
                worst = max(worst, float(err / bound))
            prev, pos = got[k, 0], pos + size
    return worst


@pytest.mark.parametrize("chunk", [1, 7, 64, 511, 513, 2048, 2049, 5000, 72000, 72001, 500000])
def test_meters_at_chunk_sizes(chunk):
    """Five chunks and a third of one (one chunk when it is longer than the row) of noise, a burst and silence.  The RMS bound
    of _check_meters is derived, not measured: two roundings per product, ceil(used / 64) - 1 adds per lane, six in the shuffle
    tree, three in alpha S + prev a, the rest for pow and the reference's own products; all terms are non-negative.  Observed on
    an MI355X, as a fraction of the bound: 0.107 (chunk 1), 0.107 (7), 0.072 (64), 0.052 (511), 0.071 (513), 0.055 (2048),
    0.035 (2049), 0.019 (5000), 0.002 (72 000), 0.001 (72 001), under 0.001 (500 000)."""
    from friture_amd.levels import LevelsBatch
    T = min(5 * chunk + chunk // 3, 399999)
    x = _meter_rows(T, 300 + chunk % 97)
    lb = LevelsBatch(3, 1, chunk)
    assert lb.kernel.shape[0] == 72000
    m, _ = lb.run(x, long=False)
    ratio = _check_meters(lb, x, m, chunk)
    print(f"chunk {chunk}: largest RMS step error / bound = {ratio:.3f}")
    # two calls cut at a chunk boundary (an empty first call when the row is one chunk)
    cut = (m.shape[1] // 2) * chunk
    two = LevelsBatch(3, 1, chunk)
    ma, _ = two.run(x[:, :cut], long=False)
    mb, _ = two.run(x[:, cut:], long=False)
    assert np.array_equal(np.concatenate([ma, mb], axis=1), m)
    assert np.array_equal(two.get_state(), lb.get_state())


@pytest.mark.parametrize("chunk,rt,T", [(100000, 1, 350000), (1, 20, 8492)])
def test_meters_and_long_levels_share_a_grid(chunk, rt, T):
    """Meters and long levels in one call: far more front tiles than chunk groups (chunk 100 000 at Ndec 8: 171 tiles, one
    group), and more chunk groups than front tiles (chunk 1 at Ndec 13: five groups of 2048 chunks, four tiles)."""
    from friture_amd.levels import LevelsBatch
    x = _meter_rows(T, 350)
    lb = LevelsBatch(3, rt, chunk)
    m, lo = lb.run(x)
    _check_meters(lb, x, m, chunk)
    assert lo.shape[1] == T >> lb.ndec and lo.shape[1] >= 1
    for c in range(3):
        _check_long(lo[c], L.LongLevelsRef(lb.ndec).push(x[c]), f"channel {c}")


# ---- 4. NaN and Inf chunks -------------------------------------------------------------------------------------------------------

def _special_rows():
    """[2, 48 chunks]: channel 0 holds a NaN beside a sample louder than the held peak (chunk 9), a NaN alone (chunk 12) and an Inf
    (chunk 30); channel 1 holds the Inf first (chunk 5), then a NaN in the lane-0 column and one in the last sample of a chunk."""
    x = 0.05 * np.random.default_rng(40).standard_normal((2, 48 * H.CHUNK))
    x[0, 9 * H.CHUNK + 100] = np.nan
    x[0, 9 * H.CHUNK + 301] = 0.9
    x[0, 12 * H.CHUNK + 77] = np.nan
    x[0, 30 * H.CHUNK + 5] = np.inf
    x[1, 5 * H.CHUNK + 200] = -np.inf
    x[1, 12 * H.CHUNK + 64] = np.nan
    x[1, 12 * H.CHUNK + 65] = -0.8
    x[1, 20 * H.CHUNK + H.CHUNK - 1] = np.nan
    return x


def _check_special(got, want, what):
    """got, want [steps, 6]"""
    assert np.array_equal(got[:, 1], want[:, 1]), what                                    # old_max: decays through a NaN chunk
    assert np.array_equal(np.isnan(got[:, 0]), np.isnan(want[:, 0])), what
    assert np.array_equal(np.isnan(got[:, 2]), np.isnan(want[:, 2])), what
    assert np.isnan(want[:, 0]).any() and not np.isnan(want[:, 0]).all() and np.isinf(want[:, 1]).any()
    ok = np.isfinite(want[:, 0])
    assert np.array_equal(np.isfinite(got[:, 0]), ok) and np.array_equal(got[~ok, 0], want[~ok, 0], equal_nan=True), what
    assert np.max(np.abs(got[ok, 0] / want[ok, 0] - 1)) <= 1e-13, what
    assert L.db_close(got[:, 2], want[:, 2]) and L.db_close(got[:, 3], want[:, 3]), what
    assert np.array_equal(got[:, 5], want[:, 5]), what                                    # branch
    peak, branch = L.ballistic_replay(got[:, 2], got[:, 3])
    assert np.array_equal(got[:, 4], peak) and np.array_equal(got[:, 5], branch), what
    assert L.db_close(got[:, 4], want[:, 4]), what


def test_nan_and_inf_chunks():
    """numpy's max is NaN when a sample is, so the reference's peak decays through such a chunk whatever else it holds."""
    from friture_amd.levels import Levels, LevelsBatch
    x = _special_rows()
    sizes = L.chunk_sizes(x.shape[1], H.CHUNK)
    lv = Levels()
    widget = np.stack([lv.handle_new_data(x[:, s:s + n]).copy() for s, n in H.chunks(x.shape[1])], axis=1)
    lb = LevelsBatch(2, 1)
    batch, lo = lb.run(x)
    for c in range(2):
        want = L.MetersCPU(lb.alpha, lb.kernel, lb.alpha2).run(x[c], sizes)
        _check_special(widget[c], want, f"Levels, channel {c}")
        _check_special(batch[c], want, f"LevelsBatch, channel {c}")
        ref = L.LongLevelsRef(lb.ndec).push(x[c])
        assert np.isnan(ref[:, 0]).any() and np.isinf(ref[:, 0]).any() and np.isfinite(ref[:, 0]).any()
        _check_long(lo[c], ref, f"long levels, channel {c}")


# ---- 5. history ring wrap ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hist", [1, 7, 18])
def test_history_ring_wraps(hist):
    from friture_amd.levels import _Handle
    ndec, B = 8, 256
    h = _Handle(2, ndec, hist)
    rng = np.random.default_rng(500 + hist)
    for round_ in range(2):
        seen = np.zeros((2, 0))
        calls = [100] + [k * B for k in (1, hist - 1, hist, hist + 1, 3 * hist + 2)]      # 100 samples stay pending throughout
        for i, n in enumerate(calls):
            x = np.stack([0.1 * rng.standard_normal(n), 0.01 * rng.standard_normal(n)])
            _, lo = _levels_run(h, _addr(x) if n else None, n, n)
            assert lo.shape[1] == ([0, 1, hist - 1, hist, hist + 1, 3 * hist + 2][i])
            seen = np.concatenate([seen, lo[:, :, 1]], axis=1)
            for count in {1, hist}:
                want = np.concatenate([np.zeros((2, count)), seen], axis=1)[:, -count:]   # zeros before `count` blocks exist
                assert np.array_equal(h.history(count), want), (round_, i, count)
        assert seen.shape[1] > hist and not np.any(seen == 0.0)
        h.reset()
        assert np.array_equal(h.history(hist), np.zeros((2, hist)))
    buf = np.zeros((2, hist + 1))
    for count in (hist + 1, -1):
        assert h.lib.frt_levels_history(h.h, count, buf.ctypes.data) == -1
        assert "frt_levels_history" in _last_error(h.lib) and str(count) in _last_error(h.lib)


# ---- 6. Ndec change with carried samples ---------------------------------------------------------------------------------------

NDEC_STEPS = [(13, 20, 8191, 0), (8, 1, 0, 31), (3, 0.02, 5, 32), (13, 20, 20000, 2), (12, 10, 1, 0), (12, 10, 5000, 2)]


def test_ndec_change_with_carried_samples():
    """(Ndec, its response time, samples pushed, blocks returned): 13 -> 8 makes 31 blocks out of carried samples alone; through
    LongLevels (setresptime) and through frt_levels_run with n == 0 and a null input pointer."""
    from friture_amd.levels import _Handle, ndec_for
    from friture_amd.longlevels import LongLevels
    x = 0.1 * np.random.default_rng(60).standard_normal((1, sum(n for _, _, n, _ in NDEC_STEPS)))
    ref = L.LongLevelsRef(13)
    ll = LongLevels(20, length_seconds=10)
    h = _Handle(1, 13, 4)
    pos = 0
    for step, (ndec, rt, n, nb) in enumerate(NDEC_STEPS):
        assert ndec_for(rt) == ndec
        if step:
            ref.set_ndec(ndec)
            ll.setresptime(rt)
            h.set_ndec(ndec)
        seg = np.ascontiguousarray(x[:, pos:pos + n])
        want = ref.push(seg[0])
        assert want.shape[0] == nb, step
        _check_long(ll.handle_new_data(seg)[0], want, f"LongLevels, step {step}")
        _check_long(_levels_run(h, _addr(seg) if n else None, n, n)[1][0], want, f"frt_levels_run, step {step}")
        if nb:
            assert abs(ll.level_rms - want[-1, 1]) <= 1e-12 and abs(h.history(1)[0, 0] - want[-1, 1]) <= 1e-12
        assert h.lib.frt_levels_pending(h.h) == ll._h.lib.frt_levels_pending(ll._h.h) == ref.pending()
        pos += n


# ---- 7. channel count changes ---------------------------------------------------------------------------------------------------

def test_channel_count_changes():
    """6 stereo chunks, 5 mono chunks, 6 stereo chunks: channel 1's state waits through the mono calls (the scan kernel copies
    its meter entries, the FIR kernel the rest)."""
    from friture_amd.levels import Levels
    rng = np.random.default_rng(70)
    x = np.stack([0.2 * rng.standard_normal(17 * H.CHUNK), H.sine(17 * H.CHUNK, 440., 0.05) + 0.01 * rng.standard_normal(17 * H.CHUNK)])
    lv = Levels()
    cpu = [L.MetersCPU(lv.alpha, lv.kernel, lv.alpha2) for _ in range(2)]
    got, want = [[], []], [[], []]
    for k, (s, n) in enumerate(H.chunks(x.shape[1])):
        stereo = not 6 <= k < 11
        if k == 8:                                                   # an empty mono chunk: the previous values, no peak update
            before = lv.get_state()
            m = lv.handle_new_data(x[:1, :0])
            got[0].append(m[0].copy())
            want[0].append(cpu[0].step(x[0, :0]))
            assert np.array_equal(lv.get_state()[2:4], before[2:4])                        # old_max and old_rms of channel 0
        before = lv.get_state()
        m = lv.handle_new_data(x[:2 if stereo else 1, s:s + n])
        assert m.shape[0] == (2 if stereo else 1) and lv.two_channels == stereo
        after = lv.get_state()
        per = (after.shape[0] - 2) // 2
        assert np.array_equal(after[:2], before[:2])
        if not stereo:
            assert np.array_equal(after[2 + per:], before[2 + per:])                       # channel 1 untouched
            changed = np.flatnonzero(after[2:2 + per] != before[2:2 + per])
            assert changed.size and changed.max() < 8                                      # channel 0: meter entries only
        for c in range(m.shape[0]):
            got[c].append(m[c].copy())
            want[c].append(cpu[c].step(x[c, s:s + n]))
    assert len(got[0]) == 18 and len(got[1]) == 12
    for c in range(2):
        g, w = np.array(got[c]), np.array(want[c])
        assert np.array_equal(g[:, 1], w[:, 1]), c
        assert np.max(np.abs(g[:, 0] / w[:, 0] - 1)) <= 1e-13, c
        assert L.db_close(g[:, 2], w[:, 2]) and L.db_close(g[:, 3], w[:, 3]) and L.db_close(g[:, 4], w[:, 4]), c
        assert np.array_equal(g[:, 5], w[:, 5]), c


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------

def _create(lib, channels, ndec, hist):
    from friture_amd.levels import PEAK_DECAY_RATE
    kernel, g11, g41 = np.ones(4), np.array(H.gauss(11, 2.)), np.array(H.gauss(41, 8.))
    h = ctypes.c_void_p()
    rc = lib.frt_levels_create(ctypes.byref(h), channels, ndec, hist, kernel.ctypes.data_as(_DP), 4, 0.5, 0.5,
                               g11.ctypes.data_as(_DP), g41.ctypes.data_as(_DP), PEAK_DECAY_RATE)
    return rc, h


@pytest.mark.parametrize("channels,ndec,hist,word", [(0, 8, 4, "0 channels"), (65536, 8, 4, "65536 channels"), (2, 0, 4, "Ndec 0"),
                                                     (2, 14, 4, "Ndec 14"), (2, 8, 0, "history of 0")])
def test_create_refusals(hip, channels, ndec, hist, word):
    rc, h = _create(hip, channels, ndec, hist)
    assert rc == -1 and not h.value
    assert "frt_levels_create" in _last_error(hip) and word in _last_error(hip)


def test_run_push_and_state_refusals(hip):
    from friture_amd.levels import _Handle
    h = _Handle(2, 8, 4)
    x = np.zeros((2, 600))
    lo = np.zeros((2, 4, 2))
    m = np.zeros((2, 600, FIELDS))
    got = ctypes.c_int64(0)
    before = h.get_state()
    for (dtype, n, ld, chunk), word in [((1, 600, 599, 512), "ld 599"), ((1, 600, 600, 0), "chunk 0"), ((2, 600, 600, 512), "dtype 2")]:
        assert hip.frt_levels_run(h.h, x.ctypes.data, dtype, n, ld, chunk, m.ctypes.data, lo.ctypes.data, ctypes.byref(got)) == -1
        assert "frt_levels_run" in _last_error(hip) and word in _last_error(hip)
    assert hip.frt_levels_push(h.h, x.ctypes.data, 1, 600, None, lo.ctypes.data, ctypes.byref(got)) == -1
    assert "frt_levels_push" in _last_error(hip) and "all 2 channels" in _last_error(hip)
    for pending, ndec in [(8192.5, 8.0), (8191.0, 8.0), (16384.0, 8.0), (8192.0, 14.0), (8192.0, 0.0)]:
        s = before.copy()
        s[0], s[1] = pending, ndec
        assert hip.frt_levels_set_state(h.h, s.ctypes.data_as(_DP)) == -1
        assert "frt_levels_set_state" in _last_error(hip) and "bad header" in _last_error(hip)
    assert np.array_equal(h.get_state(), before)                      # a refused call changes nothing
    _, lo = _levels_run(h, _addr(x), 600, 600)
    assert lo.shape == (2, 2, 2)
