"""LoudnessBatch without a GPU: the definition (tests/loudness_helpers.py) on the standard's anchors, the gates, the loudness
range's rank rule, the cell decomposition of loudness.hip against the sequential recurrence, and the host side of
friture_amd/loudness.py: presets, counts, the state's layout and its rejections, the row view of [P, C, T]."""
import math

import numpy as np
import pytest

import loudness_helpers as lh
from friture_amd import loudness as ld
from friture_amd.resample import Resampler


def measure(x, weights):
    """(z400 [P, n], z3s [P, n]) of the whole recording x [S, T], float64, row by row."""
    y = np.stack([lh.kweight_row(r) for r in np.asarray(x, np.float64)])
    e = lh.energies(y)
    return lh.block_powers(e, weights, 4), lh.block_powers(e, weights, 30)


def prototype(zeros):
    return Resampler(48000, 192000, zeros=zeros).prototype


# ---- the anchors ----------------------------------------------------------------------------------------------------------------

def test_997_hz_at_full_scale_reads_minus_3_01():
    z400, _ = measure(lh.sine(997.0, 96000)[None], lh.PRESETS["mono"])
    assert abs(lh.integrated(z400)[0] - (-3.01)) < 0.01
    assert np.all(np.abs(lh.lkfs(z400[0, 2:]) - (-3.01)) < 0.01)          # momentary too, once the filter has settled


def test_stereo_1_khz_at_minus_23_dbfs_reads_minus_23():
    row = lh.sine(1000.0, 96000, lh.dbfs(-23.0))
    z400, _ = measure(np.stack([row, row]), lh.PRESETS["stereo"])
    assert abs(lh.integrated(z400)[0] - (-23.0)) < 0.1


@pytest.mark.parametrize("zeros, low, high", [(16, -0.001, 0.001), (12, -0.01, -0.005)])
def test_quarter_rate_sine_at_45_degrees_peaks_between_the_samples(zeros, low, high):
    """fs / 4 at 45 degrees: every sample is at -3.01 dBFS, the peaks of the wave lie between them.  16 zero crossings a side
    find them within 0.001 dB; 12 read 0.0068 dB low, which is why 16 is the default.  Read in the middle sub-block: the first
    and the last also hold the overshoot of a sine switched on and off (+0.09 dB), which is a true peak of THAT signal."""
    x = lh.sine(12000.0, 3 * lh.B, 1.0, np.pi / 4)[None]
    assert abs(20 * np.log10(lh.sample_peaks(x, 3)[0, 1]) - (-3.0103)) < 1e-3
    peaks = 20 * np.log10(lh.true_peaks(x, zeros, prototype(zeros), 3)[0])
    assert low < peaks[1] < high, peaks
    assert peaks[0] > peaks[1] and peaks[2] > peaks[1]


# ---- the gates ------------------------------------------------------------------------------------------------------------------

def mono_amplitude(lufs):
    return 10.0 ** ((lufs + 3.01) / 20.0)       # a 1 kHz sine: the K-weighting's gain there cancels the -0.691


def test_relative_gate_drops_the_quiet_ends():
    """2 s at -36, 6 s at -23, 2 s at -36: the ungated mean is about -25.1, so Gamma is about -35.1 and the -36 blocks drop out;
    what stays is 57 loud blocks and the three mixed ones on either side: -23.2.  Without the relative gate: 2 LU lower."""
    amp = np.concatenate([np.full(96000, mono_amplitude(-36.0)), np.full(288000, mono_amplitude(-23.0)), np.full(96000, mono_amplitude(-36.0))])
    z400, z3s = measure((amp * lh.sine(1000.0, 480000))[None], lh.PRESETS["mono"])
    got = lh.integrated(z400)[0]
    loud, quiet = 10 ** -2.3, 10 ** -3.6
    expect = 10 * np.log10((57 * loud + 2 * (1.5 * loud + 1.5 * quiet)) / 63)
    assert abs(got - expect) < 0.05, (got, expect)
    ungated = lh.lkfs(np.mean(z400[0]))
    assert 1.5 < got - ungated < 2.5, (got, ungated)
    absolute, gamma, keep = lh.gated(z400[0], 10.0)
    assert absolute.all() and keep.sum() == 63 and abs(gamma - (ungated - 10.0)) < 1e-9
    assert lh.gate_margin(z400, 10.0) > 1e-6
    assert lh.loudness_range(z3s)[0] > 1.0


def test_silence_reads_minus_infinity_and_no_range():
    z400, z3s = measure(np.zeros((2, 40 * lh.B)), lh.PRESETS["stereo"])
    assert z400.shape == (1, 37) and z3s.shape == (1, 11)
    assert np.all(lh.lkfs(z400) == -np.inf) and lh.integrated(z400)[0] == -np.inf and lh.loudness_range(z3s)[0] == 0.0
    assert ld.loudness_range(z3s)[0] == 0.0 and ld.loudness_range(z3s[0]) == 0.0


def test_loudness_range_rank_rule():
    """20 short-term values -30 .. -11 LUFS, all above Gamma (about -37.6): v[floor(19 * 0.95 + 0.5)] - v[floor(19 * 0.10 + 0.5)] =
    v[18] - v[2] = -12 - -28 = 16.  A value under the absolute gate and one under Gamma change nothing; order does not matter."""
    l = np.arange(-30.0, -10.0)
    z = 10.0 ** ((l + 0.691) / 10.0)
    rng = np.random.default_rng(3)
    for series in (z, rng.permutation(z), rng.permutation(np.concatenate([z, 10.0 ** ((np.array([-80.0, -45.0]) + 0.691) / 10.0)]))):
        for f in (lh.loudness_range, ld.loudness_range):
            assert abs(f(series[None])[0] - 16.0) < 1e-9
    assert ld.loudness_range(z[:1][None])[0] == 0.0                      # n < 2
    assert abs(ld.loudness_range(z[:2][None])[0] - 1.0) < 1e-9          # n = 2: v[1] - v[0]
    two = np.stack([z, z[::-1] * 0.5])
    assert np.allclose(ld.loudness_range(two), [16.0, 16.0], atol=1e-9) and ld.loudness_range(two).shape == (2,)


# ---- the host side of the product ------------------------------------------------------------------------------------------------

def test_weight_presets():
    assert ld.PRESETS == lh.PRESETS
    assert ld.channel_weights("5.1") == (1.0, 1.0, 1.0, 0.0, 1.41, 1.41) and ld.channel_weights("5.0") == (1.0, 1.0, 1.0, 1.41, 1.41)
    assert ld.channel_weights("mono") == (1.0,) and ld.channel_weights("stereo") == (1.0, 1.0)
    assert ld.channel_weights([1, 0.5]) == (1.0, 0.5)
    assert ld.LoudnessBatch("5.1").channels == 6 and ld.LoudnessBatch().weights == (1.0, 1.0)
    for bad in ("7.1", [], [1.0, -1.0], [float("nan")], [1.0] * 65):
        with pytest.raises(ValueError):
            ld.channel_weights(bad)
    for bad in (0, 513, 1.5, True):
        with pytest.raises(ValueError):
            ld.LoudnessBatch(tp_zeros=bad)


def test_the_interpolator_is_the_resamplers_prototype():
    b = ld.LoudnessBatch(tp_zeros=12)
    r = Resampler(48000, 192000, zeros=12)
    assert (r.L, r.M, r.C, r.K) == (4, 1, 48, 25) and np.array_equal(b.prototype, r.prototype) and b.prototype.shape == (97,)


@pytest.mark.parametrize("R", [1, 12, 16])
def test_emitted_counts_around_every_sub_block_edge(R):
    """A sub-block is out once the sample R past its end is in: b is emitted after N samples iff (b + 1) 4800 + R <= N."""
    b = ld.LoudnessBatch("mono", tp_zeros=R)
    Ts = sorted({max(0, k * 4800 + d) for k in range(4) for d in (-R - 1, -R, -R + 1, -1, 0, 1, R - 1, R, R + 1)})
    for T in Ts:
        brute = sum(1 for blk in range(5) if (blk + 1) * 4800 + R <= T)
        assert b.emitted(T, False) == (brute, brute) == lh.emitted(T, R, False), T
        whole, peaks = sum(1 for blk in range(5) if (blk + 1) * 4800 <= T), sum(1 for blk in range(5) if blk * 4800 < T)
        assert b.emitted(T, True) == (whole, peaks) == lh.emitted(T, R, True), T


def test_state_layout_and_rejections():
    b = ld.LoudnessBatch("stereo", tp_zeros=16)
    S, n_in = 4, 33 * 4800 + 7
    e = b.emitted(n_in, False)[0]
    assert e == 32
    layout, length = ld.state_layout(S, 2, 16, n_in, e)
    assert [layout[k][1] for k in ("filter", "samples", "energy_tail", "z400", "z3s")] == [(4, 4), (4, 4800 + 7 + 16), (4, 29), (2, 29), (2, 3)]
    assert length == 4 * (4 + 4823 + 29) + 2 * 32
    good = ld.LoudnessState(np.arange(length, dtype=np.float64), S, n_in, e)
    data, n, blocks = b._check_state(good, S)
    assert data is good.data and (n, blocks) == (n_in, e)
    parts = b.state_parts(good)
    assert parts["filter"].shape == (4, 4) and parts["z3s"].shape == (2, 3) and parts["z3s"][1, 2] == length - 1
    assert b._check_state(None, S) == (None, 0, 0)
    fresh_len = ld.state_layout(S, 2, 16, 0, 0)[1]
    assert fresh_len == S * (4 + 16)
    assert b._check_state(ld.LoudnessState(np.zeros(fresh_len), S, 0, 0), S)[1:] == (0, 0)      # an empty stream, flushed or not
    with pytest.raises(ValueError, match="state of another shape: 4 streams"):
        b._check_state(good, 2)
    with pytest.raises(ValueError, match="state of another shape: data"):
        b._check_state(good._replace(data=good.data[:-1]), S)
    with pytest.raises(ValueError, match="state of another shape: data"):
        b._check_state(good._replace(data=good.data.reshape(2, -1)), S)
    with pytest.raises(ValueError, match="state of another stream: 31 sub-blocks"):
        b._check_state(good._replace(n_blocks=31), S)
    with pytest.raises(ValueError, match="state of another stream"):
        b._check_state(good._replace(n_in=-1), S)
    with pytest.raises(ValueError, match="the state is final"):
        b._check_state(good._replace(n_blocks=34), S)
    flushed_len = ld.state_layout(S, 2, 16, n_in, 33)[1]
    final = ld.LoudnessState(np.zeros(flushed_len), S, n_in, 34)
    assert b.state_parts(final)["samples"].shape == (4, 7 + 16) and b.state_parts(final)["z3s"].shape == (2, 4)


def test_rows_of_programmes_are_read_in_place():
    b = ld.LoudnessBatch("stereo")
    base = np.arange(2 * 3 * 2 * 50, dtype=np.float32).reshape(3, 4, 50)
    # evenly spaced rows are views; two of a programme's four rows are not evenly spaced over the programmes: one copy
    for x, view in ((base[:, ::2, 5:], True), (base[:1, 1:3], True), (np.ascontiguousarray(base[:, :2]), True), (base[:, :2, :40], False)):
        rows, is_np, squeeze = b._rows(x)
        assert is_np and not squeeze and rows.shape == (2 * x.shape[0], x.shape[2]) and np.array_equal(rows, x.reshape(-1, x.shape[2]))
        assert np.shares_memory(rows, x) == view
    rows, _, _ = b._rows(base[::-1][:, :2])                                # a negative programme stride: one copy
    assert np.array_equal(rows, base[::-1][:, :2].reshape(6, 50))
    assert b._rows(base[0])[0].shape == (4, 50)
    mono = ld.LoudnessBatch("mono")
    assert mono._rows(base[0, 0])[2] and mono._rows(base[:, :1])[0].shape == (3, 50)
    for bad in (base[0, :3], base[:, :3], base[0, 0], np.zeros((2, 2, 2, 2), np.float32)):
        with pytest.raises(ValueError):
            b._rows(bad)
    with pytest.raises(TypeError):
        b._rows(base.astype(np.int16)[0])
    with pytest.raises(TypeError):
        b._rows([[0.0, 1.0]])


def test_binding_table_has_the_entry_points():
    from friture_amd import _lib
    assert {"frt_loudness_create", "frt_loudness_destroy", "frt_loudness_set_stream", "frt_loudness_run", "frt_loudness_state_length"} <= set(_lib.SIGNATURES)
    from friture_amd import build
    assert build.EXTRA_FLAGS["loudness.hip"] == ["-ffp-contract=off"]


# ---- the cell decomposition ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cell_case():
    rng = np.random.default_rng(11)
    n = 2 * lh.B + 301
    x = np.stack([0.25 * rng.standard_normal(n), 0.9 + 1e-4 * rng.standard_normal(n), lh.sine(40.0, n, 0.7)])
    return x, lh.kweight(x, np.float64), lh.kweight(x, np.longdouble)


def test_row_loop_is_the_batch_loop(cell_case):
    x, y64, _ = cell_case
    assert np.array_equal(lh.kweight_row(x[1]), y64[1]) and np.array_equal(lh.kweight_row(x[0]), y64[0])


def test_cell_form_is_the_sequential_recurrence_to_rounding(cell_case):
    """The energies of the cell form against the longdouble sequential replay, on the issue's bar 1e-10 * 4800 * max|x|^2, and
    against the float64 sequential loop relatively; the carried filter state against the sequential one."""
    x, y64, yld = cell_case
    e, state = lh.cell_energies(x)
    ref, seq = lh.energies(yld), lh.energies(y64)
    assert e.shape == ref.shape == (3, 2)
    for s in range(3):
        bar = 1e-10 * lh.B * np.max(np.abs(x[s])) ** 2
        assert np.max(np.abs(e[s] - ref[s])) <= bar * 1e-2, (s, np.max(np.abs(e[s] - ref[s])), bar)      # two decades inside
    assert np.max(np.abs(e[0] - seq[0]) / seq[0]) < 1e-12
    s = [np.zeros(3) for _ in range(4)]
    lh.kweight(x[:, :2 * lh.B], np.float64, s)
    assert np.max(np.abs(state - np.stack(s, axis=1))) <= 1e-11 * np.max(np.abs(np.stack(s, axis=1)))


def test_cell_form_continues_from_a_carried_state(cell_case):
    """Sub-block by sub-block from the carried state: the bits of the whole."""
    x, _, _ = cell_case
    e, state = lh.cell_energies(x)
    e0, s0 = lh.cell_energies(x[:, :lh.B + 100])
    e1, s1 = lh.cell_energies(x[:, lh.B:], s0)
    assert np.array_equal(np.concatenate([e0, e1], axis=1), e) and np.array_equal(s1, state)


def test_powers_are_the_definition_run_on_unit_states():
    pw = lh.powers()
    assert np.array_equal(pw[0], np.eye(4))
    s = [np.float64(0.0), np.float64(1.0), np.float64(0.0), np.float64(0.0)]
    for _ in range(lh.CELL * lh.CELLS):
        lh.step(np.float64(0.0), s)
    assert np.array_equal(pw[lh.CELLS][:, 1], s)
    assert np.max(np.abs(pw[2] - pw[1] @ pw[1])) < 1e-12 * np.max(np.abs(pw[2]))
