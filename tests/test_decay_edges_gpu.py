"""DecayBatch where test_decay_gpu.py never took it: the tile loops of dk_totals and dk_scan past their first trip, live spans of
exactly 64 and 65 tiles, every class of block length, other sample rates, onset_db, noise_tail and margin_db off their defaults,
rows that given indices make dead, and the absolute scale.  The references are the longdouble restatements of
tests/decay_helpers.py; the cases are its builders, which test_decay_edges_cpu.py proves on the reference alone (the gap
condition at 1e-6, what is reached, which path a shape takes).  The bars are X3's (test_decay_gpu.py derives them for live spans
up to 2^17 samples, which every case here stays under): 1e-9 dB on the dB fields and the curve, 1e-8 relative on the decay
times, Ts, D50 and r2, the indices equal.  Every parity test prints its distances before it asserts."""
import ctypes
import math
import time

import numpy as np
import pytest

import decay_helpers as dh

pytestmark = pytest.mark.gpu

TL = dh.TILE
CURVE = dict(keep=("params", "curve"), curve_step=7)


@pytest.fixture(scope="module")
def mod(hip):
    from friture_amd import decay
    assert decay.TILE == TL and hip.frt_decay_tile() == TL
    return decay


def host(res):
    """A DecayResult with numpy fields."""
    return type(res)(*[v.cpu().numpy() if hasattr(v, "cpu") else v for v in res])


def same_bits(a, b, fields=dh.FLOATS + dh.INDICES + ("r2", "curve")):
    a, b = host(a), host(b)
    for f in fields:
        u, v = getattr(a, f), getattr(b, f)
        assert (u is None) == (v is None), f
        if u is not None:
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), f


def pick(res, rows):
    """The rows `rows` of a DecayResult with numpy fields."""
    res = host(res)
    return type(res)(*[None if v is None else v[rows] for v in res])


# ---- A. the tile loops past their first trip ----------------------------------------------------------------------------------------

def test_strided_probes_against_the_reference(mod):
    """Four rows of 66 TL + 5 samples: tile_groups = min(ceil(67 / 4), max(16, ceil(8192 / 4))) = 17 workgroups of 4 wavefronts
    cover the 67 tiles in one trip.  The batch tests below hold 520 rows to these four."""
    x, refs = dh.strided_case()
    assert not any(dh.strided(n, len(x)) for n in dh.live_tiles([r["onset"] for r in refs], [r["truncation"] for r in refs]))
    res = host(mod.DecayBatch(block=16).run(x, truncate=None, **CURVE))
    dh.compare(res, refs, "4 probes of 66 tiles and 5 samples")


def _strided_batch(mod, label, **kw):
    import torch
    x, refs = dh.strided_case()
    db = mod.DecayBatch(block=16)
    probes = db.run(x, truncate=None, **CURVE)
    batch = torch.from_numpy(np.array(x)).cuda().repeat(dh.STRIDED_ROWS // 4, 1)            # row i is probe i % 4
    assert batch.shape == (dh.STRIDED_ROWS, dh.STRIDED_T)
    torch.cuda.synchronize()
    began = time.perf_counter()
    res = db.run(batch, truncate=None, **CURVE, **kw)
    torch.cuda.synchronize()
    print(f"{label}: {dh.STRIDED_ROWS} rows of {dh.STRIDED_T} samples in {1e3 * (time.perf_counter() - began):.2f} ms")
    res, probes = host(res), host(probes)
    same_bits(res, type(probes)(*[np.concatenate([v] * (dh.STRIDED_ROWS // 4)) for v in probes]))
    dh.compare(pick(res, slice(dh.STRIDED_ROWS - 4, None)), refs, label)


def test_strided_batch_takes_a_second_trip(mod):
    """520 rows in one launch (the default scratch_bytes holds them all): tile_groups = max(16, ceil(8192 / 520)) = 16, 64
    wavefronts per row for 67 and 66 live tiles, so wavefronts 0 .. 2 (0, 1) come round again: load_tile and scan_tile run a second
    time on the same LDS turn buffer.  Every row has the bits of its probe, in every field and in the curve."""
    _, refs = dh.strided_case()
    per_row = (2 * -(-dh.STRIDED_T // 16) + 23 * -(-dh.STRIDED_T // TL)) * 8 + 112          # decay.hip: doubles and the row record
    assert (1 << 28) // per_row >= dh.STRIDED_ROWS                                           # one slab
    spans = dh.live_tiles([r["onset"] for r in refs], [r["truncation"] for r in refs])
    groups = dh.tile_groups(dh.STRIDED_ROWS, -(-dh.STRIDED_T // TL))
    assert groups == 16 and all(n > 4 * groups for n in spans) and spans.tolist() == [67, 66, 66, 67]
    _strided_batch(mod, "one launch of 520 rows, two trips")


def test_strided_batch_in_slabs_of_one_trip(mod):
    """The same 520 rows at a scratch_bytes of 101 rows per launch: tile_groups = min(17, max(16, ceil(8192 / 101))) = 17, one
    trip again (and the last slab of 15 rows likewise); the same bits."""
    per_row = (2 * -(-dh.STRIDED_T // 16) + 23 * -(-dh.STRIDED_T // TL)) * 8 + 112
    scratch = 101 * per_row + 8
    slab = scratch // per_row
    groups = [dh.tile_groups(rows, 67) for rows in (slab, dh.STRIDED_ROWS % slab)]
    assert slab == 101 and groups == [17, 17] and not 67 > 4 * min(groups)
    _strided_batch(mod, "slabs of 101 rows, one trip", scratch_bytes=scratch)


def test_live_spans_of_64_and_65_tiles(mod):
    """The lane edge of dk_offsets' walk from the last tile down (top - lane) and of dk_finish's j0 + lane stride: given onsets and
    truncations that leave exactly 64 and 65 live tiles."""
    x, onset, truncation, refs = dh.live_span_case()
    assert dh.live_tiles(onset, truncation).tolist() == [64, 65, 64, 65, 64, 65]
    res = host(mod.DecayBatch(block=16).run(x, onset=onset, truncate=truncation, **CURVE))
    dh.compare(res, refs, "live spans of 64 and 65 tiles")


# ---- B. off the defaults ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", dh.EDGE_BLOCKS)
def test_parity_at_every_class_of_block_length(mod, W):
    """dk_front<8> at its minimum (8), with a ragged group (9) and at its last length (63); dk_front<64> at its first (64), ragged
    (65, 100), at a tile and one more (512, 513), with two blocks (1000), one (2577 = T) and none (65536)."""
    db = mod.DecayBatch(block=W)
    for f32 in (False, True):
        x, refs = dh.block_case(W, f32)
        res = host(db.run(x, **CURVE))
        dh.compare(res, refs, f"block {W} {'float32' if f32 else 'float64'} x {len(x)}")
    if W >= dh.EDGE_T:
        assert np.all(res.truncation == dh.EDGE_T)
        assert np.all(np.isnan(res.dynamic_range)) if W > dh.EDGE_T else np.all(np.abs(res.dynamic_range) <= 1e-9)


@pytest.mark.parametrize("fs", dh.EDGE_FS)
def test_parity_at_other_sample_rates(mod, fs):
    """truncate="auto" on short rows; truncate=None on a row long enough for n50 and n80, with the onset found and with given
    onsets that put E[t0 + n50] on the first sample of a tile and on the last sample of the tile before."""
    db = mod.DecayBatch(fs=fs, block=16)
    for f32 in (False, True):
        x, refs = dh.fs_case(fs, f32)
        dh.compare(host(db.run(x)), refs, f"fs {fs} {'float32' if f32 else 'float64'} x {len(x)}, auto")
    x, onset, refs = dh.fs_long_case(fs)
    n50, n80 = dh.clarity_samples(fs)
    assert (onset[1] + n50) % TL == 0 and (onset[2] + n50) % TL == TL - 1 and np.all(onset + n80 < x.shape[1])
    res = host(db.run(x, onset=onset, truncate=None))
    dh.compare(res, refs, f"fs {fs}, T {x.shape[1]}, onsets {onset.tolist()}, n50 {n50}, n80 {n80}")
    assert np.all(np.isfinite(res.c50)) and np.all(np.isfinite(res.c80)) and np.all((res.d50 > 0) & (res.d50 < 1))
    same_bits(db.run(x[0], truncate=None), pick(res, 0))             # the onset that step 2 finds, given: the same row


@pytest.mark.parametrize("name,value", dh.EDGE_SETTINGS)
def test_parity_at_other_settings(mod, name, value):
    db = mod.DecayBatch(block=16, **{name: value})
    for f32 in (False, True):
        x, refs = dh.setting_case(name, value, f32)
        res = host(db.run(x))
        dh.compare(res, refs, f"{name} {value:g} {'float32' if f32 else 'float64'}")
        if name == "onset_db" and value == 0.0:
            assert np.array_equal(res.onset, res.peak)
        if name == "noise_tail" and value == 1.0:                    # the truncation lands just behind the onset
            assert all(math.isnan(r["t30"]) and math.isfinite(r["edt"]) for r in refs)
            assert np.all(np.isnan(res.t30)) and np.all(np.isfinite(res.edt))


# ---- D. dead rows by given indices ------------------------------------------------------------------------------------------------

def test_indices_out_of_range_in_device_arrays_make_dead_rows(mod):
    """X3, step 1: a given onset or truncation outside its range, which only device arrays can carry to the kernels, makes the row
    dead; it never faults and never affects its neighbours.  Six such rows around a good one, through frt_decay_run."""
    import torch
    from friture_amd import _lib
    x, onset, truncation, good, ref = dh.dead_index_case()
    R, T = x.shape
    nc = -(-T // 7)
    h = _lib.Handle("decay", 48000.0, 16, -20.0, 0.1, 10.0)
    vp = ctypes.c_void_p

    def run(rows, x, on, tr):
        params, idx, curve = np.full((rows, 15), 7.0), np.full((rows, 3), 7, np.int64), np.full((rows, nc), 7.0)
        rc = h.lib.frt_decay_run(h.h, vp(x.ctypes.data), 1, rows, T, T, on, 2, tr, 7, 1 << 20, vp(params.ctypes.data), vp(idx.ctypes.data),
                                 vp(curve.ctypes.data))
        return rc, params, idx, curve

    on_d, tr_d = torch.from_numpy(np.array(onset)).cuda(), torch.from_numpy(np.array(truncation)).cuda()
    rc, params, idx, curve = run(R, x, vp(on_d.data_ptr()), vp(tr_d.data_ptr()))
    assert rc == 0, h.lib.frt_last_error()
    bad = np.arange(R) != good
    assert np.all(np.isnan(params[bad])) and np.all(idx[bad] == -1) and np.all(np.isnan(curve[bad]))
    one = np.ascontiguousarray(x[good:good + 1])
    rc, p1, i1, c1 = run(1, one, vp(onset[good:good + 1].ctypes.data), vp(truncation[good:good + 1].ctypes.data))
    assert rc == 0 and not np.any(p1 == 7.0)
    assert params[good].tobytes() == p1[0].tobytes() and idx[good].tobytes() == i1[0].tobytes() and curve[good].tobytes() == c1[0].tobytes()
    p = params[good:good + 1]
    res = mod.DecayResult(p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4:8], *[p[:, j] for j in range(8, 15)], *[idx[good:good + 1, j] for j in range(3)],
                          curve[good:good + 1])
    dh.compare(res, [ref], "the good row between six dead ones")
    # the same six pairs in host arrays are refused before any launch
    for i in (0, 1, 2, 4):
        rc, params, _, _ = run(1, one, vp(onset[i:i + 1].ctypes.data), vp(truncation[i:i + 1].ctypes.data))
        assert rc == -1 and np.all(params == 7.0), i
    # a truncation at or below the onset, each inside its own range, passes the host's checks and is dead on the device
    for i in (5, 6):
        rc, params, idx, curve = run(1, one, vp(onset[i:i + 1].ctypes.data), vp(truncation[i:i + 1].ctypes.data))
        assert rc == 0 and np.all(np.isnan(params)) and np.all(idx == -1) and np.all(np.isnan(curve)), i


def test_an_onset_at_or_behind_the_automatic_truncation_makes_a_dead_row(mod):
    """X3, step 4: reachable from Python, since the truncation is found on the device.  The row is dead, nothing raises, and its
    neighbours keep the bits they have without it."""
    x, onset, refs = dh.late_onset_case()
    db = mod.DecayBatch(block=16)
    res = host(db.run(x, onset=onset, **CURVE))
    dh.compare(res, refs, "rows 1 and 3 dead by their onsets")
    for f in dh.FLOATS + ("r2", "curve"):
        assert np.all(np.isnan(getattr(res, f)[[1, 3]])), f
    for f in dh.INDICES:
        assert np.all(getattr(res, f)[[1, 3]] == -1), f
    live = [0, 2, 4]
    same_bits(pick(res, live), db.run(x[live], onset=onset[live], **CURVE))
    same_bits(pick(res, live), db.run(x[live], **CURVE))             # the onsets given there are the ones step 2 finds


# ---- E. the absolute scale ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [-40, 40])
def test_a_power_of_two_scale_moves_only_the_two_levels(mod, k):
    """x 2^k changes no rounding anywhere in X3: e, every sum of e, N0, the onset bound c max|x| and the truncation bound scale by
    an exact power of two, every comparison is between two values scaled alike, and E / E[t0], Ts, D50 and q / (W N0) are ratios
    of them.  At k = -40 the smallest non-zero e of these rows is far above the smallest normal double and at k = +40 the
    largest sum is far below the largest (both asserted): no underflow, no overflow.  So every output keeps its bits but level_db and noise_db, which move by 20 k log10(2) (their own
    log10 rounds: 1e-9 dB).  A stray absolute epsilon or a float32 intermediate would break this."""
    x = dh.block_case(16, True)[0].astype(np.float64)
    nonzero = np.abs(x[x != 0])
    assert nonzero.min() ** 2 * 4.0 ** -40 > 1e-200 and (x ** 2).sum(axis=1).max() * x.shape[1] * 4.0 ** 40 < 1e200
    db = mod.DecayBatch(block=16)
    base, res = host(db.run(x, **CURVE)), host(db.run(np.ldexp(x, k), **CURVE))
    assert np.all(np.isfinite(base.level_db)) and np.all(np.isfinite(base.noise_db)) and np.any(np.isfinite(base.t30))
    same_bits(res, base, tuple(f for f in dh.FLOATS + dh.INDICES + ("r2", "curve") if f not in ("level_db", "noise_db")))
    shift = 20 * k * math.log10(2)
    d = max(dh.db_distance(res.level_db, base.level_db + shift), dh.db_distance(res.noise_db, base.noise_db + shift))
    print(f"2^{k}: level_db and noise_db move by {shift:.6f} dB within {d:.3g} dB (bar 1e-09)")
    assert d <= 1e-9
