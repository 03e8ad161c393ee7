"""tests/levels_helpers.py against the reference's recorded values (tests/golden/levels.npz) and against the constants levels.hip
declares, without a GPU: the helpers are pinned here before test_levels_edges_gpu.py holds the kernels to them."""
from pathlib import Path

import numpy as np
import pytest

import levels_helpers as L
from oracle import levels as H

GOLDEN = Path(__file__).resolve().parent / "golden" / "levels.npz"


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", ["noise", "bursts", "impulse", "stereo", "irregular"])
def test_meters_cpu_matches_reference(g, name):
    """MetersCPU per channel against the recorded widget, with the tolerances test_levels_gpu.py holds the GPU to."""
    from friture_amd.levels import meter_coefficients
    x = H.signal(name)
    ref = g[f"meters_{name}"]
    sizes = [n for _, n in H.chunks(x.shape[1], H.IRREGULAR_CHUNKS if name == "irregular" else None)]
    got = np.stack([L.MetersCPU(*meter_coefficients()).run(x[c], sizes) for c in range(x.shape[0])])
    assert got.shape[:2] == ref.shape[:2]
    assert np.array_equal(got[..., 1], ref[..., 1])                                       # old_max
    assert np.max(np.abs(got[..., 3] - ref[..., 3])) <= 1e-12                              # level_max
    assert np.max(np.abs(got[..., 0] / ref[..., 0] - 1)) <= 1e-13                          # rms
    assert np.max(np.abs(got[..., 2] - ref[..., 2])) <= 1e-12
    assert np.array_equal(got[..., 5], ref[..., 5])                                       # ballistic branches
    assert np.max(np.abs(got[..., 4] - ref[..., 4])) <= 1e-12
    for c in range(x.shape[0]):
        peak, branch = L.ballistic_replay(got[c, :, 2], got[c, :, 3])
        assert np.array_equal(peak, got[c, :, 4]) and np.array_equal(branch, got[c, :, 5])


def test_rms_step_brackets_the_reference_dot():
    """rms_step (extended precision) and exp_smoothed_value (numpy's dot) agree far inside the bound the GPU is held to; an empty
    chunk returns the previous value and leaves the peak alone; a chunk longer than the kernel forgets the previous value."""
    from friture_amd.levels import meter_coefficients
    alpha, kernel, alpha2 = meter_coefficients()
    m = L.MetersCPU(alpha, kernel, alpha2)
    rng = np.random.default_rng(21)
    for n in (1, 63, 64, 65, 512, 5000, 72000, 72001, 80000):
        y = 0.1 * rng.standard_normal(n)
        want = m.rms_step(0.25, y)
        got = m.exp_smoothed_value(y ** 2, 0.25)
        assert abs(got - want) <= 8 * 2.0 ** -53 * want, n
        if n > 72000:
            assert m.rms_step(0.25, y) == m.rms_step(1e9, y)
            assert m.rms_step(0.25, y) == m.rms_step(0.0, y[:72000])         # the first Nk samples against the whole kernel
    before = (m.old_max, m.old_rms)
    row = m.step(np.zeros(0))
    assert (m.old_max, m.old_rms) == before and row[0] == before[1] and row[5] == L.HOLD
    assert m.rms_step(0.25, np.zeros(0)) == 0.25


def test_meters_cpu_nan_decays_the_peak():
    """numpy's max is NaN when any sample is; `value_max > old_max (1 - alpha2)` is then false and the peak decays."""
    from friture_amd.levels import meter_coefficients
    m = L.MetersCPU(*meter_coefficients())
    m.step(np.full(16, 0.5))
    held = m.old_max
    row = m.step(np.array([0.1, np.nan, 0.9]))
    assert row[1] == held * (1. - m.alpha2) and np.isnan(row[0]) and np.isnan(row[2]) and np.isfinite(row[4])
    row = m.step(np.array([0.1, np.inf]))
    assert row[1] == np.inf and np.isnan(row[0])


class _RefHandle:
    """friture_amd.levels._Handle's long-level calls served by LongLevelsRef."""

    def __init__(self, channels, ndec, history_len):
        assert channels == 1
        self.ref = L.LongLevelsRef(ndec)

    def set_ndec(self, ndec):
        self.ref.set_ndec(ndec)

    def push(self, x, meters=True, long=False):
        assert long and not meters
        return None, self.ref.push(x[0])[None]


def test_long_levels_ref_set_ndec_matches_curve_fixture(g, monkeypatch):
    """LongLevels' host code over LongLevelsRef in place of the device handle, driven by CURVE_STEPS (Ndec 10 -> 8 -> 13 with
    samples pending): the curves the reference widget drew."""
    from friture_amd import longlevels
    monkeypatch.setattr(longlevels, "_Handle", _RefHandle)
    x = H.signal("curve")
    ll = longlevels.LongLevels(4)
    ll.setduration(30)
    pos, k = 0, 0
    for step, v in H.CURVE_STEPS:
        if step == "push":
            for _ in range(v):
                ll.handle_new_data(x[:, pos:pos + H.CHUNK])
                pos += H.CHUNK
            t, y = ll.curve()
            assert np.array_equal(t, g[f"curve_{k}_t"]), k
            assert np.max(np.abs(y - g[f"curve_{k}_y"])) <= 1e-12, k
            k += 1
        else:
            getattr(ll, step)(v)
    assert k == 6


def test_long_levels_ref_carried_samples():
    """13 with 8191 samples pending, then 8: 31 blocks out of carried samples alone."""
    x = 0.1 * np.random.default_rng(22).standard_normal(8191)
    ref = L.LongLevelsRef(13)
    assert ref.push(x).shape == (0, 2) and ref.pending() == 8191
    ref.set_ndec(8)
    out = ref.push(np.zeros(0))
    assert out.shape == (31, 2) and ref.pending() == 8191 - 31 * 256
    # the blocks are those of a stream that ran at Ndec 8 from the start of the carried samples on, behind a zero state
    fresh = L.LongLevelsRef(8)
    assert np.array_equal(fresh.push(x), out)


def test_kernel_constants_are_the_expected_ones():
    assert L.kernel_constants() == L.EXPECTED_CONSTANTS
    with pytest.raises(AssertionError):
        L.kernel_constants("constexpr int kFrontJ = 64;")


def test_levels_block_counts():
    """(129 << Ndec) + 2^Ndec samples for Ndec <= 5, ((2 Bt + 1) << Ndec) + 2^Ndec above."""
    blocks = [L.seam_lengths(ndec)["levels"] >> ndec for ndec in range(1, 14)]
    assert blocks == [130] * 5 + [2050, 1026, 514, 258, 130, 66, 34, 18]
    for ndec in range(1, 14):
        n = L.seam_lengths(ndec)["levels"]
        assert n == ((129 << ndec) + (1 << ndec) if ndec <= 5 else
                     ((2 * max(8, 2048 >> (ndec - 5)) + 1) << ndec) + (1 << ndec))
        assert n <= 150000


@pytest.mark.parametrize("ndec", range(1, 14))
def test_seam_lengths_are_in_their_classes(ndec):
    s = L.seam_lengths(ndec)
    last = "front" if ndec <= 5 else "tail"
    per = 64 if ndec <= 5 else max(8, 2048 >> (ndec - 5))
    # frt_levels_run: whole blocks only, so every stage length but the last is even
    p = L.tile_plan(ndec, s["levels"])
    assert p[f"{last}_tiles"] == 3 and p[f"{last}_last"] == 2 and (p["J"] if ndec <= 5 else p["Bt"]) == per
    assert all(e % 2 == 0 for e in p["E"][:-1])
    if ndec > 5:
        assert p["front_tiles"] >= 2 and (ndec >= 10 or p["front_last"] < 64)   # below Ndec 10 the front's last tile is ragged too
    p = L.tile_plan(ndec, s["levels_one"])
    assert p[f"{last}_tiles"] == 3 and p[f"{last}_last"] == 1
    # frt_levels_subsample
    p = L.tile_plan(ndec, s["odd"])
    assert all(e % 2 == 1 for e in p["E"])
    assert p["front_last"] == 1 and p["E"][p["S"]] % 64 == 1
    if ndec > 5:
        assert p["tail_last"] == 1 and p["E"][ndec] % p["Bt"] == 1 and p["tail_tiles"] == 3
    p = L.tile_plan(ndec, s["even"])
    assert all(e % 2 == 0 for e in p["E"])
    assert p["front_last"] == 64 and (ndec <= 5 or (p["tail_last"] == p["Bt"] and p["tail_tiles"] == 2))
    p = L.tile_plan(ndec, s["short"])
    assert p["E"][0] % 2 == 1 and p["E"][1:] == L.tile_plan(ndec, s["even"])["E"][1:]
    p = L.tile_plan(ndec, s["ragged"])
    assert p["E"][p["S"]] % 64 == 63 and p["front_last"] == 63 and (ndec <= 5 or p["tail_last"] == p["Bt"])
    assert p["E"][p["S"] + 1:] == L.tile_plan(ndec, s["even"])["E"][p["S"] + 1:]
    assert max(s.values()) <= 150000
