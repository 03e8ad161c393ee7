"""MtfBatch where test_sti_gpu.py never took it: the tile loop of mtf_tiles past its first trip, intervals of exactly 64 and 65
live tiles, sample rates that are not 48000 (one of them no integer), modulation frequencies next to fs / 2 and far below 1 Hz,
nine frequencies (mtf_finish's eight wavefronts partly filled on their second trip), and the absolute scale.  The references are
the longdouble restatements of tests/sti_helpers.py; the cases are its builders, which test_sti_edges_cpu.py proves on the
reference alone.  The bars are sh.compare's: 1e-10 absolute on m, 1e-10 relative on energy.  test_sti_gpu.py derives them from
(n - 1) 2^-53 for n <= 2^17; the strided case has n = 66 * 4096 + 5, where that bound is 3e-11: still under the bar.  Every
parity test prints its distances before it asserts."""
import time

import numpy as np
import pytest

import decay_helpers as dh
import sti_helpers as sh

pytestmark = pytest.mark.gpu

TL = sh.TILE


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import sti
    assert sti.TILE == TL and hip.frt_mtf_tile() == TL and sti.MOD_FREQS == sh.MOD_FREQS
    return sti


def host(res):
    """A result tuple with numpy fields."""
    return type(res)(*[v.cpu().numpy() if hasattr(v, "cpu") else v for v in res])


def same_bits(a, b):
    a, b = host(a), host(b)
    for f in a._fields:
        u, v = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), f


def pick(res, rows):
    res = host(res)
    return type(res)(*[v[rows] for v in res])


# ---- A. the tile loop past its first trip -----------------------------------------------------------------------------------------

def test_strided_probes_against_the_reference(mod):
    """Four rows of 66 TL + 5 samples: tile_groups = min(ceil(67 / 4), max(16, ceil(8192 / 4))) = 17 workgroups of 4 wavefronts
    cover the 67 tiles in one trip.  The batch tests below hold 520 rows to these four."""
    x, start, ref = sh.strided_case()
    assert not any(dh.strided(n, len(x)) for n in dh.live_tiles(start, [x.shape[1]] * 4, TL))
    sh.compare(host(mod.MtfBatch().run(x, start=start)), ref, "4 probes of 66 tiles and 5 samples")


def _strided_batch(mod, label, **kw):
    import torch
    x, start, ref = sh.strided_case()
    mb = mod.MtfBatch()
    probes = host(mb.run(x, start=start))
    reps = sh.STRIDED_ROWS // 4
    batch = torch.from_numpy(np.array(x)).cuda().repeat(reps, 1)     # row i is probe i % 4; made on the device
    lo = torch.from_numpy(np.array(start)).cuda().repeat(reps)
    assert batch.shape == (sh.STRIDED_ROWS, sh.STRIDED_T) and batch.dtype == torch.float32
    torch.cuda.synchronize()
    began = time.perf_counter()
    res = mb.run(batch, start=lo, **kw)
    torch.cuda.synchronize()
    print(f"{label}: {sh.STRIDED_ROWS} rows of {sh.STRIDED_T} samples in {1e3 * (time.perf_counter() - began):.2f} ms")
    same_bits(res, type(probes)(*[np.concatenate([v] * reps) for v in probes]))
    sh.compare(pick(res, slice(sh.STRIDED_ROWS - 4, None)), ref, label)


def test_strided_batch_takes_a_second_trip(mod):
    """520 rows in one launch (the default scratch_bytes holds them all): tile_groups = max(16, ceil(8192 / 520)) = 16, 64
    wavefronts per row for 67 and 66 live tiles, so the first wavefronts come round again.  Every row has the bits of its probe."""
    _, start, _ = sh.strided_case()
    per_row = -(-sh.STRIDED_T // TL) * (1 + 2 * 14) * 8              # mtf.hip: 1 + 2 nf doubles per tile
    assert (1 << 28) // per_row >= sh.STRIDED_ROWS                   # one slab
    spans = dh.live_tiles(start, [sh.STRIDED_T] * 4, TL)
    groups = dh.tile_groups(sh.STRIDED_ROWS, -(-sh.STRIDED_T // TL))
    assert groups == 16 and all(n > 4 * groups for n in spans) and spans.tolist() == [67, 67, 66, 67]
    _strided_batch(mod, "one launch of 520 rows, two trips")


def test_strided_batch_in_slabs_of_one_trip(mod):
    """The same 520 rows at a scratch_bytes of 101 rows per launch: tile_groups = min(17, max(16, ceil(8192 / 101))) = 17, one
    trip again (and the last slab of 15 rows likewise); the same bits."""
    per_row = -(-sh.STRIDED_T // TL) * (1 + 2 * 14) * 8
    scratch = 101 * per_row + 8
    slab = scratch // per_row
    groups = [dh.tile_groups(rows, 67) for rows in (slab, sh.STRIDED_ROWS % slab)]
    assert slab == 101 and groups == [17, 17] and not 67 > 4 * min(groups)
    _strided_batch(mod, "slabs of 101 rows, one trip", scratch_bytes=scratch)


def test_live_spans_of_64_and_65_tiles(mod):
    """The lane edge of tile_sum's J0 + lane stride in mtf_finish: intervals of exactly 64 and 65 live tiles."""
    x, start, stop, ref = sh.live_span_case()
    assert dh.live_tiles(start, stop, TL).tolist() == [64, 65, 64, 65, 64, 65]
    sh.compare(host(mod.MtfBatch().run(x, start=start, stop=stop)), ref, "live spans of 64 and 65 tiles")


# ---- C. off the defaults ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs,freqs", sh.OFF_DEFAULT)
def test_parity_at_other_rates_and_frequencies(mod, fs, freqs):
    """The exact integer reduction of phasor() at other exponents of F and fs: F next to fs / 2 (half a cycle per sample), F =
    0.001 Hz, fs = 100 (the lowest), a fs and an F that are no integers; and nf = 9 at 48000, where one of mtf_finish's eight
    wavefronts takes a second frequency and seven do not."""
    mb = mod.MtfBatch(freqs, fs=fs)
    for f32 in (False, True):
        x, ref = sh.off_default_case(fs, freqs, f32)
        res = host(mb.run(x))
        assert res.m.shape == (3, len(freqs))
        sh.compare(res, ref, f"fs {fs:g}, F {freqs} {'float32' if f32 else 'float64'}")


def test_far_positions_at_44100_against_the_two_sample_form(mod):
    """Two unit samples, the second near the end of a row of 2^24: |1 + exp(-2 pi i F a / fs)| / 2 at fs = 44100 for F = 22049.5,
    where the phase advances by nearly half a cycle per sample, and F = 0.63: the coarse table at another rate."""
    import torch
    T, freqs = 1 << 24, (22049.5, 0.63)
    first, second = 5, T - 2
    x = torch.zeros((1, T), dtype=torch.float32, device="cuda")
    x[0, first] = x[0, second] = 1.0
    res = host(mod.MtfBatch(freqs, fs=44100).run(x))
    want = np.array([sh.two_sample_m(F, second - first, 1.0, 44100) for F in freqs])
    sh.compare(res, (want[None], np.array([2.0])), "T 2^24 at fs 44100")
    assert want.max() < 0.9                                          # the form is not 1 anywhere


# ---- E. the absolute scale ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [-40, 40])
def test_a_power_of_two_scale_moves_only_the_energy(mod, k):
    """x 2^k changes no rounding in X5: every e and every product and sum of e with the (unscaled) table entries scales by the
    exact power 2^(2 k), as long as nothing underflows or overflows (asserted: the smallest non-zero e and the largest sum stay
    far inside the normal doubles).  m = |S_j| / S0 keeps its bits; energy is 2^(2 k) times the unscaled energy exactly."""
    x = sh.seam_rows(5 * TL + 17, 65, True).astype(np.float64)
    nonzero = np.abs(x[x != 0])
    assert nonzero.min() ** 2 * 4.0 ** -40 > 1e-200 and (x ** 2).sum(axis=1).max() * 4.0 ** 40 < 1e200
    mb = mod.MtfBatch()
    base, res = host(mb.run(x)), host(mb.run(np.ldexp(x, k)))
    assert np.all(np.isfinite(base.m)) and base.m.min() < 0.95
    assert res.m.tobytes() == base.m.tobytes()
    assert res.energy.tobytes() == np.ldexp(base.energy, 2 * k).tobytes()
